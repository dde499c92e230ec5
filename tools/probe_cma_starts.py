#!/usr/bin/env python3
"""ms per CMA-ES generation of K seeded starts (CMAOptimizer.optimize(..., starts=K)) at the reference's own size (1127 GCPs
with 1 px noise, pop 50, float64, Huber f = 10; gcp9: D 9 phase 1, gcp12: D 12 phase 2 from the phase-1 result), for
  host        starts=K on the host loop: one evaluation of K x 50 candidates and K host tells per generation
  device      starts=K, device_loop=True: one draw, one evaluation and one K-workgroup tell launch per generation
  sequential  K single runs one after the other: K x the per-generation cost of one single run (starts=1), the faster of
              its host and device loops (both measured, reported in the K = 1 lines)
A generation's cost is the difference of two whole optimize() calls, (t(G) - t(G0)) / (G - G0), as in
tools/probe_cma_device.py: the upload of the points, the last generation and the final errors cancel.  One JSON line per
(shape, K, path).

  python tools/probe_cma_starts.py [--only gcp9,gcp12] [--ks 1,8,64,256] [--paths host,device] [--gens 300] [--reps 2]
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
from alproj_amd.optimize import CMAOptimizer         # noqa: E402
from tools.probe_cma_device import TARGETS_D12, problem     # noqa: E402


def per_generation(opt, gens, g0, reps, **kw):
    """best of `reps` of (t(gens) - t(g0)) / (gens - g0) in ms, and the final error of the last long call"""
    best, err = np.inf, None
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
    ap.add_argument("--only", default="gcp9,gcp12")
    ap.add_argument("--ks", default="1,8,64,256")
    ap.add_argument("--paths", default="host,device")
    ap.add_argument("--gens", type=int, default=300)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    L.init(0)
    only, paths = args.only.split(","), args.paths.split(",")
    ks = [int(k) for k in args.ks.split(",")]
    obj, img, init = problem(1127)
    kw = dict(sigma=1.0, population_size=50, f_scale=10.0, seed=7, progress=False)
    o = CMAOptimizer(obj, img, init)
    o.set_target(list(syn.TARGETS_D9))
    shapes = [("gcp9", o)] if "gcp9" in only else []
    if "gcp12" in only:
        p1, _ = o.optimize(generation=args.gens, device_loop=True, **kw)
        o2 = CMAOptimizer(obj, img, p1)
        o2.set_target(TARGETS_D12)
        shapes.append(("gcp12", o2))
    for name, opt in shapes:
        single = {}
        for K in ks:
            for path in paths:
                # the host loop's cost grows with K (K host tells per generation): fewer generations there
                gens = args.gens if (path == "device" or K <= 8) else max(40, args.gens * 8 // K)
                g0 = max(2, gens // 10)
                ms, err = per_generation(opt, gens, g0, args.reps, starts=K, device_loop=path == "device", **kw)
                if K == 1:
                    single[path] = ms
                line = {"shape": name, "points": 1127, "population": 50, "dims": len(opt.target_params), "precision": "f64",
                        "starts": K, "path": path, "generations": gens, "ms_per_generation": ms,
                        "us_per_start_generation": ms * 1e3 / K, "final_px_best": err,
                        "final_px_starts": [e for _, _, e in opt.start_results]}
                print(json.dumps(line), flush=True)
            if single:
                seq = K * min(single.values())
                print(json.dumps({"shape": name, "points": 1127, "population": 50, "dims": len(opt.target_params), "precision": "f64",
                                  "starts": K, "path": "sequential", "ms_per_generation": seq, "us_per_start_generation": seq * 1e3 / K,
                                  "measured_as": "K x one single run, the faster of its loops (%s)" % min(single, key=single.get)}),
                      flush=True)


if __name__ == "__main__":
    main()
