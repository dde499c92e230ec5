#!/usr/bin/env python3
"""ms per CMA-ES generation, the host loop (CMAOptimizer.optimize, the default) against the device loop
(device_loop=True: alp_cma_run), at
  gcp9 / gcp12  the reference's own size as bench.py's cma_gcp_scale builds it: 1127 GCPs with 1 px noise, pop 50, D 9
                (phase 1) / D 12 (phase 2, distortion only, from the phase-1 result), float64, Huber f = 10
  cfg3          BASELINE config 3's shape: 10 M points, pop 256, D 9, float32
A generation's cost is the difference of two whole optimize() calls, (t(G) - t(G0)) / (G - G0), so that the upload of the
points and the final float64 error cancel.  One JSON line per shape.

  python tools/probe_cma_device.py [--only gcp9,gcp12,cfg3] [--gens 300] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alproj_amd import _lib as L                     # noqa: E402
from alproj_amd import synthetic as syn              # noqa: E402
from alproj_amd.optimize import CMAOptimizer         # noqa: E402

TARGETS_D12 = ["k1", "k2", "k3", "k4", "k5", "k6", "p1", "p2", "s1", "s2", "s3", "s4"]


def problem(n):
    tp = syn.truth_params(316)
    gx = syn.gcp_points(n, tp, seed=3)
    with L.Points(gx, [tp["x"], tp["y"], tp["z"]], "f64" if n <= 4_000_000 else "f32") as gp:
        gp.project(L.params_vector(tp))
        gu, gv = gp.fetch()
    guv = np.stack([gu, gv], 1) + np.random.default_rng(3).normal(0, 1.0, (n, 2))
    init = dict(tp, pan=tp["pan"] + 2, tilt=tp["tilt"] - 1.5, fov=tp["fov"] + 3, x=tp["x"] + 4)
    return pd.DataFrame(gx, columns=["x", "y", "z"]), pd.DataFrame(guv, columns=["u", "v"]), init


def per_generation(opt, gens, g0, reps, **kw):
    """best of `reps` of (t(gens) - t(g0)) / (gens - g0) in ms, and the final error of the last long call"""
    best = np.inf
    err = None
    for _ in range(reps):
        t0 = time.perf_counter()
        opt.optimize(generation=g0, **kw)
        t1 = time.perf_counter()
        _, err = opt.optimize(generation=gens, **kw)
        t2 = time.perf_counter()
        best = min(best, ((t2 - t1) - (t1 - t0)) / (gens - g0) * 1e3)
    return best, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="gcp9,gcp12,cfg3")
    ap.add_argument("--gens", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    L.init(0)
    only = args.only.split(",")
    g0 = max(2, args.gens // 10)
    if "gcp9" in only or "gcp12" in only:
        obj, img, init = problem(1127)
        kw = dict(sigma=1.0, population_size=50, f_scale=10.0, seed=7, progress=False)
        o = CMAOptimizer(obj, img, init)
        o.set_target(list(syn.TARGETS_D9))
        p1, _ = o.optimize(generation=args.gens, **kw)
        shapes = []
        if "gcp9" in only:
            shapes.append(("gcp9", o))
        if "gcp12" in only:
            o2 = CMAOptimizer(obj, img, p1)
            o2.set_target(TARGETS_D12)
            shapes.append(("gcp12", o2))
        for name, opt in shapes:
            host, e_host = per_generation(opt, args.gens, g0, args.reps, **kw)
            dev, e_dev = per_generation(opt, args.gens, g0, args.reps, device_loop=True, **kw)
            print(json.dumps({"shape": name, "points": 1127, "population": 50, "dims": len(opt.target_params), "precision": "f64",
                              "generations": args.gens, "host_loop_ms_per_generation": host, "device_loop_ms_per_generation": dev,
                              "device_over_host": dev / host, "final_px_host": e_host, "final_px_device": e_dev}), flush=True)
    if "cfg3" in only:
        obj, img, init = problem(10_000_000)
        o = CMAOptimizer(obj, img, init)
        o.set_target(list(syn.TARGETS_D9))
        kw = dict(sigma=1.0, population_size=256, f_scale=10.0, seed=7, precision="f32", progress=False)
        gens = max(g0 + 10, args.gens // 3)
        host, e_host = per_generation(o, gens, g0, 1, **kw)
        dev, e_dev = per_generation(o, gens, g0, 1, device_loop=True, **kw)
        print(json.dumps({"shape": "cfg3", "points": 10_000_000, "population": 256, "dims": 9, "precision": "f32", "generations": gens,
                          "host_loop_ms_per_generation": host, "device_loop_ms_per_generation": dev,
                          "host_generations_per_s": 1e3 / host, "device_generations_per_s": 1e3 / dev,
                          "final_px_host": e_host, "final_px_device": e_dev}), flush=True)


if __name__ == "__main__":
    main()
