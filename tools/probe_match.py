#!/usr/bin/env python3
"""alp_match_knn2 (the exact 2-nearest-neighbour search and ratio test of the reference's built-in matchers, gcp.py:55-70) at the
sizes the project is built for: 50 000 x 50 000 descriptors at L = 61 (AKAZE) and L = 128 (SIFT's length, as bytes), and
5 000 x 5 000.  Not part of bench.py; reads nothing from outside the tree (the descriptors are drawn here).

Per shape: two warm-up calls, then --reps calls.  Each call is timed as a whole (host clock around the entry point: allocation,
upload of both arrays, kernels, results back) and its kernel sections by the library's HIP-event timer (alp_kernel_timing: the
two packing launches, then the walk and the merge).  One JSON line per shape, appended to --out:

  kernel_ms / call_ms      median of the repeats, with min and max (the spread)
  mac_per_s                n_query x n_train x padded_len / kernel time: int8 multiply-adds at the length the MFMA contracts
  fraction_of_i8_peak      of 2.5e15 MAC/s: 256 CUs x 4 SIMDs x 1024 MAC per cycle (v_mfma_i32_32x32x32_i8: 32 cycles) x 2.4 GHz
  outside_kernels_share    (call_ms - kernel_ms) / call_ms: allocation, the upload and the results' way back
  checked                  the first 64 queries agree with the numpy restatement (tests/match_cases.py), bit for bit

  python tools/probe_match.py [--reps 7] [--shapes 50000x50000x61,50000x50000x128,5000x5000x61] [--out profiles/match_probe.jsonl]
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
import match_cases as mc                             # noqa: E402

I8_PEAK_MAC_PER_S = 256 * 4 * 1024 * 2.4e9


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def probe(n1, n2, length, reps, dtype):
    train = mc.random_bytes(n2, length, 1)
    query = mc.noisy_copies(train, n1, 2, noise=12)
    if dtype == "f32":
        train, query = train.astype(np.float32), query.astype(np.float32)
    for _ in range(2):
        r = L.match_knn2(query, train)
    L.kernel_time_ms()
    kernel, call, sections = [], [], 0
    for _ in range(reps):
        t = time.perf_counter()
        r = L.match_knn2(query, train)
        call.append((time.perf_counter() - t) * 1e3)
        ms, sections = L.kernel_time_ms()
        kernel.append(ms)
    want = mc.restate(query[:64], train)
    checked = all(np.array_equal(np.asarray(r[k][:64]).view(np.uint8), np.asarray(want[k]).view(np.uint8)) for k in ("idx", "dist2", "dist", "good"))
    k, c = statistics.median(kernel), statistics.median(call)
    padded = r["info"]["padded_len"]
    return {"probe": "match_knn2", "n_query": n1, "n_train": n2, "len": length, "dtype": dtype, "info": r["info"], "reps": reps,
            "kernel_sections": sections, "kernel_ms": spread(kernel), "call_ms": spread(call),
            "mac_per_s": round(n1 * n2 * padded / (k * 1e-3), 1), "fraction_of_i8_peak": round(n1 * n2 * padded / (k * 1e-3) / I8_PEAK_MAC_PER_S, 4),
            "mac_per_s_at_len": round(n1 * n2 * length / (k * 1e-3), 1), "outside_kernels_share": round((c - k) / c, 4),
            "upload_bytes": int(query.nbytes + train.nbytes), "n_good": r["n_good"], "checked": bool(checked)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="50000x50000x61,50000x50000x128,5000x5000x61")
    ap.add_argument("--dtype", default="u8", choices=("u8", "f32"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_probe.jsonl"))
    a = ap.parse_args()
    L.init(0)
    L.kernel_timing(True)
    for shape in a.shapes.split(","):
        n1, n2, length = (int(v) for v in shape.split("x"))
        line = json.dumps(probe(n1, n2, length, a.reps, a.dtype))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
    L.kernel_timing(False)


if __name__ == "__main__":
    main()
