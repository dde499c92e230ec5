#!/usr/bin/env python3
"""alp_normal_equations (normal_poses_kernel for one pose: J^T J, J^T r and the cost formed on the device) against the path it replaces, at
bench.py's f1 shape: 10 M GCP-like points in a float64 set, D = 21 (g5's targets).  One process, one run, one JSON line each:

  (a) "host_contraction": pts.jacobian + pts.residuals + J.T @ J and J.T @ r in numpy -- the (2N, D) matrix crosses PCIe
      (3.36 GB at 10 M points) and one host process contracts it;
  (b) "normal_equations": one pts.normal_equations call -- 2.4 KB cross PCIe;
  (c) the kernel sections of either, summed by the library's HIP-event timer (alp_kernel_timing): jacobian_kernel's 13
      launches next to normal_poses_kernel + reduce_normal_poses_kernel.
  --big N: one more line, (b) alone on N float32 points (100 M: the size of the bench's grid set).

The condition the change is held to: call_ms of (b) <= 0.5 x call_ms of (a).  The two results are compared as well (the
largest difference in units of the normalisers m max|J_i| max|J_j|, m max|J_i| max|r|).

  python tools/probe_normal.py [--points 10000000] [--reps 5] [--big 0] [--out profiles/normal_probe.jsonl]
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/probe_normal.py     (per-kernel summary, a run of its own)
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
    """best whole-call time of `reps`: (kernel ms summed over the call's launches, launches, whole-call ms, result)"""
    best = None
    for _ in range(reps):
        L.kernel_time_ms()
        t0 = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t0) * 1e3
        k, n = L.kernel_time_ms()
        if best is None or wall < best[2]:
            best = (k, n, wall, out)
    return best


def observed(xyz, p, pv, precision, sigma=1.0):
    """the set's own projection + noise, without a host-side projection of 10^7 .. 10^8 points"""
    with L.Points(xyz, [p["x"], p["y"], p["z"]], precision) as ref:
        ref.project(pv)
        u, v = ref.fetch(np.float32 if precision == "f32" else np.float64)
    rng = np.random.default_rng(5)
    u += rng.normal(0, sigma, len(u)).astype(u.dtype)
    v += rng.normal(0, sigma, len(v)).astype(v.dtype)
    return u, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L.init(0)
    rows = []
    p = dict(syn.truth_params(316), **LENS)
    pv = L.params_vector(p)
    cols = [L.PARAM_KEYS.index(t) for t in TARGETS_D21]
    D = len(cols)
    if args.points > 0:
        n = args.points
        xyz = syn.gcp_points(n, p, seed=3)
        with L.Points(xyz, [p["x"], p["y"], p["z"]], "f64") as pts:
            pts.set_observed_columns(*observed(xyz, p, pv, "f64"))

            def host_path():
                J = pts.jacobian(pv, cols)
                r = pts.residuals(pv)
                return J.T @ J, J.T @ r, 0.5 * float(r @ r), None, np.abs(J).max(axis=0), float(np.abs(r).max())

            pts.normal_equations(pv, cols)          # warm: scratch, result pool
            pts.jacobian(pv, cols)
            L.kernel_timing(True)
            kj, lj, _, _ = timed(lambda: pts.jacobian(pv, cols).shape, max(1, args.reps // 2))       # jacobian_kernel alone
            ka, la, wa, ref = timed(host_path, max(1, args.reps // 2))
            kb, lb, wb, got = timed(lambda: pts.normal_equations(pv, cols), args.reps)
            L.kernel_timing(False)
        m = 2 * n
        cj, rmax = ref[4], ref[5]
        err_G = float((np.abs(got[0] - ref[0]) / (m * np.outer(cj, cj))).max())
        err_g = float((np.abs(got[1] - ref[1]) / (m * cj * rmax)).max())
        rows.append(dict(path="host_contraction", points=n, columns=D, precision="f64", launches=la, kernel_ms=round(ka, 4),
                         jacobian_kernel_ms=round(kj, 4), jacobian_launches=lj, call_ms=round(wa, 2), pcie_bytes=n * 16 * (D + 1)))
        rows.append(dict(path="normal_equations", points=n, columns=D, precision="f64", launches=lb, kernel_ms=round(kb, 4),
                         call_ms=round(wb, 3), pcie_bytes=8 * (D * (D + 1) // 2 + D + 2), call_ratio=round(wb / wa, 5),
                         kernel_ratio_to_jacobian_kernel=round(kb / kj, 4), err_G=err_G, err_g=err_g,
                         cost_rel=abs(got[2] - ref[2]) / ref[2]))
        del xyz
    if args.big > 0:
        n = args.big
        xyz = syn.gcp_points(n, p, seed=4)          # float64 in: the origin is subtracted before the set narrows to float32
        with L.Points(xyz, [p["x"], p["y"], p["z"]], "f32") as pts:
            pts.set_observed_columns(*observed(xyz, p, pv, "f32"))
            del xyz
            pts.normal_equations(pv, cols)
            L.kernel_timing(True)
            kb, lb, wb, got = timed(lambda: pts.normal_equations(pv, cols), args.reps)
            L.kernel_timing(False)
        rows.append(dict(path="normal_equations", points=n, columns=D, precision="f32", launches=lb, kernel_ms=round(kb, 4),
                         call_ms=round(wb, 3), pcie_bytes=8 * (D * (D + 1) // 2 + D + 2), count=got[3],
                         mean_sq_residual=2 * got[2] / (2 * n)))
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
