#!/usr/bin/env python3
"""The device loop of the least-squares iteration (alp_lm_*, LsqOptimizer.optimize(method="normal", device_loop=True)) against
the host lockstep of the same library (optimize.normal_lm_batch on Points.normal_equations_batch), in one process, alternated.
One JSON line per configuration:

  small  n = 1127 float64 points, D = 9, linear loss, K = 1 / 8 / 64 / 256 starts drawn around the pose the observations were
         made with: the whole solve by the host lockstep and by the device loop with check_every = 1, 8, 32, the same starts;
         the median wall time of --reps repetitions after a warm-up, the rounds taken (the largest evaluation count of a start)
         and the wall time per round.
  large  n = --points (10 M) float64 points, D = 21, K = 8: the same, check_every = 8, --large-reps repetitions: where the
         evaluation dominates, the loop must cost nothing.

Which number is compared with which: the device loop against the host lockstep in the same run.  No ratio is fixed in advance.
Kernel time per round by kernel (lm_step_kernel, lm_select_kernel, normal_poses_kernel, reduce_normal_poses_kernel):
from a separate kernel-trace run of `--steps trace` (the device loop alone, K = 64, check_every = 8) under the profiler.

  python tools/probe_lm_device.py [--steps small,large] [--reps 15] [--out profiles/lm_device_probe.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alproj_amd import _lib as L                     # noqa: E402
from alproj_amd import optimize as aopt              # noqa: E402
from tools.probe_normal import TARGETS_D21           # noqa: E402
from tools.probe_normal_batch import TARGETS_D9, problem      # noqa: E402


def setup(n, targets, K, seed=3):
    xyz, origin, (u, v), pv, _, cols = problem(n, targets, 1, seed)
    centre = pv[cols]
    half = np.array([aopt.DEFAULT_BOUND_WIDTHS.get(t, 0.2) for t in targets])
    lower, upper = centre - half, centre + half
    X0 = np.empty((K, len(cols)))
    X0[0] = centre + 0.01 * half
    X0[1:] = centre + np.random.default_rng(seed).uniform(-0.1, 0.1, (K - 1, len(cols))) * half
    return xyz, origin, (u, v), pv, cols, lower, upper, X0


def host_solve(pts, pv, cols, lower, upper, X0):
    def sums(X):
        cand = np.tile(pv, (len(X), 1))
        cand[:, cols] = X
        return pts.normal_equations_batch(cand, cols)[:3]
    return aopt.normal_lm_batch(sums, X0, lower, upper)


def device_solve(pts, pv, cols, lower, upper, X0, check_every):
    with L.LmDevice(pts, pv, cols, lower, upper, X0) as loop:
        pending = len(X0)
        while pending:
            loop.run(check_every)
            pending = loop.wait()
        return loop.get()


def measure(n, targets, K, check_everys, reps):
    xyz, origin, (u, v), pv, cols, lower, upper, X0 = setup(n, targets, K)
    with L.Points(xyz, origin, "f64") as pts:
        pts.set_observed_columns(u, v)
        del xyz
        names = ["host"] + ["device_%d" % c for c in check_everys]
        fns = {"host": lambda: host_solve(pts, pv, cols, lower, upper, X0)}
        for c in check_everys:
            fns["device_%d" % c] = (lambda c=c: device_solve(pts, pv, cols, lower, upper, X0, c))
        out = {name: fns[name]() for name in names}                       # warm-up, and the results
        wall = {name: [] for name in names}
        for _ in range(reps):
            for name in names:
                t0 = time.perf_counter()
                fns[name]()
                wall[name].append((time.perf_counter() - t0) * 1e3)
    host = out["host"]
    dev = out[names[1]]
    rounds = {"host": max(r["evaluations"] for r in host)}
    for name in names[1:]:
        rounds[name] = int(out[name]["evaluations"].max())
    rec = dict(points=n, columns=len(cols), starts=K, reps=reps,
               host_status=[int(r["status"]) for r in host][:8], device_status=[int(s) for s in dev["status"]][:8],
               max_rel_cost_difference=float(max(abs(dev["cost"][k] - host[k]["cost"]) / host[k]["cost"] for k in range(K))))
    for name in names:
        med = float(np.median(wall[name]))
        rec[name] = dict(solve_ms=round(med, 4), rounds=rounds[name], ms_per_round=round(med / rounds[name], 5),
                         spread=round((max(wall[name]) - min(wall[name])) / med, 3))
    for name in names[1:]:
        rec[name]["host_over_device"] = round(rec["host"]["solve_ms"] / rec[name]["solve_ms"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="small,large")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--large-reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join("profiles", "lm_device_probe.jsonl"))
    args = ap.parse_args()
    L.init(0)
    steps = args.steps.split(",")
    if "trace" in steps:
        xyz, origin, (u, v), pv, cols, lower, upper, X0 = setup(1127, TARGETS_D9, 64)
        with L.Points(xyz, origin, "f64") as pts:
            pts.set_observed_columns(u, v)
            for _ in range(5):
                rec = device_solve(pts, pv, cols, lower, upper, X0, 8)
        print(json.dumps(dict(step="trace", solves=5, starts=64, rounds=int(rec["evaluations"].max()))))
        return
    lines = []
    if "small" in steps:
        for K in (1, 8, 64, 256):
            lines.append(dict(step="small", **measure(1127, TARGETS_D9, K, (1, 8, 32), args.reps)))
            print(json.dumps(lines[-1]), flush=True)
    if "large" in steps:
        lines.append(dict(step="large", **measure(args.points, TARGETS_D21, 8, (8,), args.large_reps)))
        print(json.dumps(lines[-1]), flush=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
