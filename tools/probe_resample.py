#!/usr/bin/env python3
"""LsqOptimizer.cross_validate / .bootstrap (K fits under the K rows of a weight table, one lockstep, the points uploaded once)
against the same fits as K sequential LsqOptimizer(weights=row).optimize(method="normal") calls -- what the parent commit can
already run -- in one process, alternated.  One JSON line per configuration:

  gcp    the 400 GCPs of tests/golden/g14_lsq.npz (trf_linear_d7: x, y, z, fov, pan, tilt, roll), float64:
         (a) cross_validate(folds=8) and bootstrap(n_boot=256), host lockstep and device_loop=True;
         (b) the 8 / 256 weighted single fits, one after the other.
  large  --points (10 M) synthetic float64 points, D = 7: cross_validate(folds=8), and bootstrap(n_boot=8) -- the stored table
         is capped at 1 GiB, which at 10 M float64 points is 13 rows --, against the 8 sequential fits.

Median wall time of --reps repetitions after a warm-up, the spread (max - min) / median, and (b) / (a).  No ratio is fixed in
advance: the comparison is (a) against (b) measured in the same process.  The single fits of (b) are also compared with the
folds' costs (max relative difference).

  python tools/probe_resample.py [--steps gcp,large] [--reps 7] [--out profiles/resample_probe.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from alproj_amd import _lib as L                     # noqa: E402
from alproj_amd import optimize as aopt              # noqa: E402
from alproj_amd import resample                      # noqa: E402
from alproj_amd import synthetic as syn              # noqa: E402

TARGETS = ["x", "y", "z", "fov", "pan", "tilt", "roll"]


def gcp_problem():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g14_lsq.npz"))
    keys = [str(k) for k in g["param_keys"]]
    case = "trf_linear_d7"
    return (pd.DataFrame(g["xyz"], columns=["x", "y", "z"]), pd.DataFrame(g["uv_" + str(g[f"{case}_uv"])], columns=["u", "v"]),
            dict(zip(keys, g[f"{case}_init"])))


def large_problem(n, seed=3):
    truth = syn.truth_params(316)
    xyz = syn.gcp_points(n, truth, seed=seed)
    with L.Points(xyz, [truth["x"], truth["y"], truth["z"]], "f64") as pts:
        pts.project(L.params_vector(truth))
        u, v = pts.fetch()
    rng = np.random.default_rng(seed)
    obj = pd.DataFrame(xyz, columns=["x", "y", "z"], copy=False)
    img = pd.DataFrame({"u": u + rng.normal(0, 1.0, n), "v": v + rng.normal(0, 1.0, n)}, copy=False)
    init = dict(truth, pan=truth["pan"] + 0.5, tilt=truth["tilt"] - 0.3, fov=truth["fov"] + 0.5, x=truth["x"] + 1.0)
    return obj, img, init


def lsq(obj, img, init, weights=None):
    o = aopt.LsqOptimizer(obj, img, init, weights=weights)
    o.set_target(TARGETS)
    return o


def sequential(obj, img, init, table, precision):
    costs = []
    for row in table:
        o = lsq(obj, img, init, row)
        o.optimize(method="normal", precision=precision)
        costs.append(o.result_["cost"])
    return np.array(costs)


def timed(fns, reps):
    out = {name: fn() for name, fn in fns.items()}                      # warm-up, and the results
    wall = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    stats = {name: dict(ms=round(float(np.median(w)), 3), spread=round((max(w) - min(w)) / float(np.median(w)), 3)) for name, w in wall.items()}
    return out, stats


def measure(obj, img, init, folds, n_boot, reps, precision="f64", seed=1):
    n = len(obj)
    train, _ = resample.fold_tables(resample.fold_labels(n, folds, seed))
    boot = resample.bootstrap_table(n, n_boot, seed)
    o = lsq(obj, img, init)
    # (the resampling calls draw their table inside the call; the sequential fits are handed theirs)
    fns = {"cv_host": lambda: o.cross_validate(folds=folds, seed=seed, precision=precision),
           "cv_device": lambda: o.cross_validate(folds=folds, seed=seed, precision=precision, device_loop=True),
           "cv_sequential": lambda: sequential(obj, img, init, train, precision),
           "boot_host": lambda: o.bootstrap(n_boot=n_boot, seed=seed, precision=precision),
           "boot_device": lambda: o.bootstrap(n_boot=n_boot, seed=seed, precision=precision, device_loop=True),
           "boot_sequential": lambda: sequential(obj, img, init, boot, precision)}
    out, stats = timed(fns, reps)
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.abs(b)))
    rec = dict(points=n, columns=len(TARGETS), folds=folds, n_boot=n_boot, reps=reps, **stats)
    rec["cv_held_out_rmse"] = float(out["cv_host"]["rmse"])
    rec["boot_dropped"] = int(out["boot_host"]["dropped"])
    rec["cv_cost_rel_to_sequential"] = {k: rel(np.array([r["cost"] for r in out["cv_" + k]["fold_results"]]), out["cv_sequential"])
                                        for k in ("host", "device")}
    rec["boot_cost_rel_to_sequential"] = {k: rel(np.array([r["cost"] for r in out["boot_" + k]["results"]]), out["boot_sequential"])
                                          for k in ("host", "device")}
    for what in ("cv", "boot"):
        for k in ("host", "device"):
            rec["%s_sequential_over_%s" % (what, k)] = round(stats[what + "_sequential"]["ms"] / stats["%s_%s" % (what, k)]["ms"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="gcp,large")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--large-reps", type=int, default=2)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--out", default=os.path.join("profiles", "resample_probe.jsonl"))
    args = ap.parse_args()
    L.init(0)
    lines = []
    steps = args.steps.split(",")
    if "gcp" in steps:
        lines.append(dict(step="gcp", **measure(*gcp_problem(), 8, 256, args.reps)))
        print(json.dumps(lines[-1]), flush=True)
    if "large" in steps:
        lines.append(dict(step="large", **measure(*large_problem(args.points), 8, 8, args.large_reps)))
        print(json.dumps(lines[-1]), flush=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
