#!/usr/bin/env python3
"""Kernel time and HBM traffic of jacobian_kernel (alp_jacobian: the exact Jacobian, D columns) against residual_batch_kernel
(alp_residuals_batch: the D + 1 poses of the 2-point differences LsqOptimizer's default jac="batched" takes) at bench.py's f1
shape: 10 M GCP-like points in a float64 set, D = 21 (g5's targets) against 22 poses.  Either call stages its output through
launches of at most 256 MB (13 / 14 launches); the kernel sections are summed by the library's HIP-event timer
(alp_kernel_timing) and the whole call by the host clock, which includes the device-to-host copies.  One JSON line per path.

Traffic per point (what the kernels must move, not a counter reading): jacobian_kernel reads 24 B (three float64
coordinates) and writes 16 D B; residual_batch_kernel reads 40 B (coordinates and observed pixels) and writes 16 B per pose.

  python tools/probe_jacobian.py [--points 10000000] [--reps 5]
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/probe_jacobian.py     (per-kernel summary)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alproj_amd import _lib as L                     # noqa: E402
from alproj_amd import synthetic as syn              # noqa: E402

TARGETS_D21 = ["x", "y", "z", "fov", "pan", "tilt", "roll", "a1", "a2", "k1", "k2", "k3", "k4", "k5", "k6", "p1", "p2",
               "s1", "s2", "s3", "s4"]
LENS = dict(a1=0.02, a2=-0.01, k1=-0.05, k2=0.01, k3=0.002, k4=0.003, k5=-0.001, k6=0.0005, p1=0.001, p2=-0.002, s1=0.0005,
            s2=-0.0002, s3=-0.0003, s4=0.0001)


def timed(fn, reps):
    """best of `reps`: (kernel ms summed over the call's launches, launches, whole-call ms)"""
    best = None
    for _ in range(reps):
        L.kernel_time_ms()
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        k, n = L.kernel_time_ms()
        if best is None or k < best[0]:
            best = (k, n, wall)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    L.init(0)
    n, D = args.points, len(TARGETS_D21)
    p = dict(syn.truth_params(316), **LENS)
    xyz = syn.gcp_points(n, p, seed=3)
    pv = L.params_vector(p)
    cols = [L.PARAM_KEYS.index(t) for t in TARGETS_D21]
    cand = np.tile(pv, (D + 1, 1))
    cand[np.arange(1, D + 1), cols] += 1e-6
    with L.Points(xyz, [p["x"], p["y"], p["z"]], "f64") as pts:
        with L.Points(xyz, [p["x"], p["y"], p["z"]], "f64") as ref:
            ref.project(pv)
            u, v = ref.fetch()
        pts.set_observed(np.stack([u, v], 1))
        del u, v
        pts.jacobian(pv, cols)                  # warm: scratch, result pool
        pts.residuals_batch(cand)
        L.kernel_timing(True)
        rows = []
        for name, fn, nbytes in (
                ("jacobian_kernel", lambda: pts.jacobian(pv, cols), n * (24 + 16 * D)),
                ("residual_batch_kernel", lambda: pts.residuals_batch(cand), n * (40 + 16 * (D + 1)))):
            k, launches, wall = timed(fn, args.reps)
            rows.append(dict(kernel=name, points=n, columns=D if name == "jacobian_kernel" else D + 1, launches=launches,
                             kernel_ms=round(k, 4), call_ms=round(wall, 2), bytes=nbytes, kernel_tb_s=round(nbytes / k / 1e9, 3)))
        L.kernel_timing(False)
    for r in rows:
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
