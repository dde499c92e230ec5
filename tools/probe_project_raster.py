#!/usr/bin/env python3
"""Development probe: single-pose projection of a W x R raster (rows of W points), kernel ms from HIP events around every
launch (best and median); the projection's grid form unless ALP_NO_POINTS_GRID is set.
python3 tools/probe_project_raster.py W R reps [f32|f64]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alproj_amd import _lib as L            # noqa: E402
from alproj_amd import synthetic as syn     # noqa: E402

W, R, reps = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
prec = sys.argv[4] if len(sys.argv) > 4 else "f32"
L.init(0)
n = W * R
xyz = np.empty((n, 3), dtype=np.float32)
xyz[:, 0] = np.tile(np.arange(W, dtype=np.float32), R)
xyz[:, 1] = np.repeat(np.arange(R - 1, -1, -1, dtype=np.float32), W)
xyz[:, 2] = np.random.default_rng(0).standard_normal(n, dtype=np.float32) * 50
side = max(W, R)
cam = syn.perturbed(syn.standoff_params(side))
cam = syn.local_params(cam, syn.ABS_ORIGIN_XZY)
pts = L.Points(xyz, [cam["x"], cam["y"], cam["z"]], prec)
pv = L.params_vector(cam)
ms = []
for r in range(reps):
    L.event_record(0)
    pts.project(pv)
    L.event_record(1)
    L.synchronize()
    ms.append(L.event_elapsed_ms(0, 1))
best, med = min(ms), float(np.median(ms))
print(f"W={W} R={R} N={n} {prec} row_length={pts.row_length()}: best {best:.4f} ms  median {med:.4f} ms  {n / best / 1e6:.1f} Gpts/s")
