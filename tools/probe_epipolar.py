#!/usr/bin/env python3
"""The geometric match filter (alp_epipolar_ransac: 8-point hypotheses, every one scored on every match, the best refitted) at the
sizes image_match meets: n = 500, 5 000 and 50 000 matches at H = 16 384 hypotheses, and H = 1 024 and 131 072 at n = 5 000.
Not part of bench.py; reads nothing from outside the tree (the scenes are those of tests/epipolar_cases.py, 40 % outliers).

Per shape: two warm-up calls, then --reps calls of the whole filter and of each stage's own entry point.  Each call is timed as a
whole (host clock around the entry point: allocation, upload, kernels, results back) and its kernel sections by the library's
HIP-event timer (alp_kernel_timing).  One JSON line per shape, appended to --out:

  ransac.kernel_ms / call_ms   median of the repeats, with min and max (the spread): pack, normalisation, draw, solve, score, merge,
                               choice, the refit rounds and the final mask
  samples / solve8 / score     the same for the stage alone; solve8 and score include packing the points (and solve8 the
                               normalisation), which the whole filter does once
  refit_ms                     ransac - samples - solve8 - score kernel medians: the choice, the refit rounds and the mask, less
                               the packing counted twice
  errors_per_s                 H x n / the score stage's kernel time
  fraction_of_f64_peak         errors_per_s x 35 flop / 78.6e12: the error expression of include/alproj_hip.h counted by hand
                               (5 lines of 2 mul + 2 add = 20, s: 4, s^2: 1, two denominators of 2 mul + 1 add: 6, two
                               divisions: 2, max and compare: 2; a division counts as one)
  checked                      the mask is the restatement's under the returned F, and the first 64 counts agree with numpy

  python tools/probe_epipolar.py [--reps 7] [--shapes 500x16384,5000x16384,50000x16384,5000x1024,5000x131072] [--out profiles/epipolar_probe.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from alproj_amd import _lib as L                     # noqa: E402
import epipolar_cases as ec                          # noqa: E402

F64_PEAK_FLOP_PER_S = 78.6e12
ERROR_FLOP = 35
THRESHOLD = 3.0


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def timed(fn, reps):
    for _ in range(2):
        out = fn()
    L.kernel_time_ms()
    kernel, call, sections = [], [], 0
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        call.append((time.perf_counter() - t) * 1e3)
        ms, sections = L.kernel_time_ms()
        kernel.append(ms)
    return out, {"kernel_ms": spread(kernel), "call_ms": spread(call), "kernel_sections": sections}


def probe(n, H, reps):
    p1, p2, _, out = ec.scene(n, (2 * n) // 5, 0.5, 1)
    r, whole = timed(lambda: L.epipolar_ransac(p1, p2, THRESHOLD, hypotheses=H, seed=1), reps)
    samples, t_samples = timed(lambda: L.epipolar_samples(n, H, seed=1), reps)
    Fs, t_solve = timed(lambda: L.epipolar_solve8(p1, p2, samples), reps)
    (counts, plan), t_score = timed(lambda: L.epipolar_score(p1, p2, Fs, THRESHOLD), reps)
    checked = bool(np.array_equal(r["mask"], ec.inliers(r["F"], p1, p2, THRESHOLD)) and
                   np.array_equal(counts[:64], ec.counts(Fs[:64], p1, p2, THRESHOLD)) and
                   int(np.argmax(counts)) == r["info"]["chosen"])
    k = {name: t["kernel_ms"]["median"] for name, t in (("ransac", whole), ("samples", t_samples), ("solve8", t_solve), ("score", t_score))}
    rate = H * n / (k["score"] * 1e-3)
    return {"probe": "epipolar_ransac", "n": n, "H": H, "threshold": THRESHOLD, "outlier_share": 0.4, "reps": reps, "info": r["info"],
            "score_plan": plan, "ransac": whole, "samples": t_samples, "solve8": t_solve, "score": t_score,
            "refit_ms": round(k["ransac"] - k["samples"] - k["solve8"] - k["score"], 4),
            "share_of_ransac_kernels": {s: round(k[s] / k["ransac"], 4) for s in ("samples", "solve8", "score")},
            "errors_per_s": round(rate, 1), "fraction_of_f64_peak": round(rate * ERROR_FLOP / F64_PEAK_FLOP_PER_S, 4),
            "outside_kernels_share": round((whole["call_ms"]["median"] - k["ransac"]) / whole["call_ms"]["median"], 4),
            "inliers_kept": round(float(r["mask"][~out].mean()), 4), "outliers_kept": round(float(r["mask"][out].mean()), 4),
            "checked": checked}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="500x16384,5000x16384,50000x16384,5000x1024,5000x131072")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epipolar_probe.jsonl"))
    a = ap.parse_args()
    L.init(0)
    L.kernel_timing(True)
    for shape in a.shapes.split(","):
        n, H = (int(v) for v in shape.split("x"))
        line = json.dumps(probe(n, H, a.reps))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    L.kernel_timing(False)


if __name__ == "__main__":
    main()
