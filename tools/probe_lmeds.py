#!/usr/bin/env python3
"""The LMedS select (alp_epipolar_select: the rank-th smallest error of every hypothesis, 16 passes of a radix select that each
form every error again) next to the score kernel (alp_epipolar_score: one compare per error) at the same shape in the same
process, and the whole filters built on them.  Not part of bench.py; reads nothing from outside the tree (the scene is
tests/epipolar_cases.scene(n, 0.4 n, 0.5, 1)).

Shapes (n, H): (5 000, 16 384) the default call, (512, 256) one workgroup of one tile, (5 000, 163 840) the essential filter's
ten slots per sample (the slots of alp_epipolar_solve5, the unused NaN ones included).

Per shape: two warm-up calls, then --reps calls of each entry point; the kernel sections by the library's HIP-event timer
(alp_kernel_timing), median, min and max, and the ratio of the select's median to the score's.  A P-pass select cannot be faster
than P times the score.  One JSON line per shape and one per whole filter, written to --out.

  python tools/probe_lmeds.py [--reps 7] [--out profiles/lmeds_probe.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from alproj_amd import _lib as L                     # noqa: E402
import epipolar_cases as ec                          # noqa: E402

K = (ec.FOCAL, ec.WIDTH / 2.0, ec.HEIGHT / 2.0)
SHAPES = ((5000, 16384, 8), (512, 256, 8), (5000, 16384, 5))


def timed(fn, reps):
    for _ in range(2):
        out = fn()
    L.kernel_time_ms()
    kernel, call = [], []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        call.append((time.perf_counter() - t) * 1e3)
        kernel.append(L.kernel_time_ms()[0])
    return out, kernel, call


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lmeds_probe.jsonl"))
    a = ap.parse_args()
    L.init(0)
    L.kernel_timing(True)
    arch = L.device_info()["arch"]
    lines = []
    for n, samples, m in SHAPES:
        p1, p2, _, out = ec.scene(n, int(0.4 * n), 0.5, 1)
        if m == 8:
            Fs = L.epipolar_solve8(p1, p2, L.epipolar_samples(n, samples, 1))
        else:
            Fs = L.epipolar_solve5(p1, p2, L.epipolar_samples5(n, samples, 1), K[0], K[1:])[0]
        Fs = Fs.reshape(-1, 3, 3)
        H, rank = len(Fs), L.lmeds_rank(n, m)
        (counts, plan), score_k, score_c = timed(lambda: L.epipolar_score(p1, p2, Fs, 3.0), a.reps)
        (value, splan), select_k, select_c = timed(lambda: L.epipolar_select(p1, p2, Fs, rank), a.reps)
        passes = splan["passes"]
        ratio = statistics.median(select_k) / statistics.median(score_k)
        lines.append({"probe": "select_vs_score", "arch": arch, "n": n, "H": H, "m": m, "rank": rank, "passes": passes, "splits": splan["splits"],
                      "workgroups": splan["workgroups"], "hist_bytes": splan["hist_bytes"], "reps": a.reps,
                      "score_kernel_ms": stats(score_k), "select_kernel_ms": stats(select_k), "score_call_ms": stats(score_c),
                      "select_call_ms": stats(select_c), "select_over_score": round(ratio, 3), "select_over_passes_times_score": round(ratio / passes, 3),
                      "errors_per_s_score": round(n * H / statistics.median(score_k) * 1e3, 0),
                      "errors_per_s_select": round(passes * n * H / statistics.median(select_k) * 1e3, 0),
                      "finite_values": int((value < float("inf")).sum()), "best_count": int(counts.max())})
        print(json.dumps(lines[-1]), flush=True)
    n = 5000
    p1, p2, _, out = ec.scene(n, 2000, 0.5, 1)
    for name, fn in (("fundamental RANSAC threshold 3", lambda: L.epipolar_ransac(p1, p2, 3.0, hypotheses=16384, seed=1)),
                     ("fundamental LMEDS", lambda: L.epipolar_lmeds(p1, p2, L.lmeds_rank(n, 8), L.lmeds_scale2(n, 8), 1.0, hypotheses=16384, seed=1)),
                     ("essential RANSAC threshold 3", lambda: L.essential_ransac(p1, p2, K[0], K[1:], 3.0, hypotheses=16384, seed=1)),
                     ("essential LMEDS", lambda: L.essential_lmeds(p1, p2, K[0], K[1:], L.lmeds_rank(n, 5), L.lmeds_scale2(n, 5), 1.0, hypotheses=16384, seed=1))):
        r, kernel, call = timed(fn, a.reps)
        lines.append({"probe": "whole_filter", "arch": arch, "filter": name, "n": n, "samples": 16384, "refits": 4, "reps": a.reps,
                      "kernel_ms": stats(kernel), "call_ms": stats(call), "inliers_kept": round(float(r["mask"][~out].mean()), 4),
                      "outliers_kept": round(float(r["mask"][out].mean()), 4), "bound_px": round(r["bound"], 3) if "bound" in r else 3.0,
                      "refits_kept": r["info"]["refits_kept"]})
        print(json.dumps(lines[-1]), flush=True)
    L.kernel_timing(False)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
