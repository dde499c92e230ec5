#!/usr/bin/env python3
"""Development probe: single-pose projection of a W x R raster (float32, rows of W points), kernel ms from HIP events; the
projection's grid form unless ALP_NO_POINTS_GRID is set.  python3 tools/probe_project_raster.py W R reps"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alproj_amd import _lib as L            # noqa: E402
from alproj_amd import synthetic as syn     # noqa: E402

W, R, reps = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
L.init(0)
n = W * R
xyz = np.empty((n, 3), dtype=np.float32)
xyz[:, 0] = np.tile(np.arange(W, dtype=np.float32), R)
xyz[:, 1] = np.repeat(np.arange(R - 1, -1, -1, dtype=np.float32), W)
xyz[:, 2] = np.random.default_rng(0).standard_normal(n, dtype=np.float32) * 50
side = max(W, R)
cam = syn.perturbed(syn.standoff_params(side))
cam = syn.local_params(cam, syn.ABS_ORIGIN_XZY)
pts = L.Points(xyz, [cam["x"], cam["y"], cam["z"]], "f32")
pv = L.params_vector(cam)
best = 1e9
for r in range(reps):
    L.event_record(0)
    pts.project(pv)
    L.event_record(1)
    L.synchronize()
    best = min(best, L.event_elapsed_ms(0, 1))
print(f"W={W} R={R} N={n} row_length={pts.row_length()}: best {best:.4f} ms  {n / best / 1e6:.1f} Gpts/s")
