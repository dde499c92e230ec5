#!/usr/bin/env python3
"""The essential-matrix match filter (alp_essential_ransac: 5-point samples, up to ten slots each, every slot scored on every match)
next to the fundamental filter (alp_epipolar_ransac) in the same process: n = 5 000 matches, the essential filter at
H = 16 384 and H = 2 048 samples, the fundamental one at H = 16 384.  Not part of bench.py; reads nothing from outside the tree
(the scene is tests/epipolar_cases.scene(5000, 2000, 0.5, 1): 40 % outliers, threshold 3, seed 1).

Per row: two warm-up calls, then --reps calls.  Each call is timed as a whole (host clock around the entry point: allocation,
upload, kernels, results back) and its kernel sections by the library's HIP-event timer (alp_kernel_timing); median, min and max.
The solver stage alone (alp_epipolar_solve5, which packs the points too) is timed the same way.  One line per row, written to --out.

  python tools/probe_essential.py [--reps 7] [--out profiles/essential_probe.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from alproj_amd import _lib as L                     # noqa: E402
import epipolar_cases as ec                          # noqa: E402

N, THRESHOLD, SEED = 5000, 3.0, 1
K = (ec.FOCAL, ec.WIDTH / 2.0, ec.HEIGHT / 2.0)


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


def row(name, kernel, call, extra=""):
    return (f"{name:<34} kernel ms median {statistics.median(kernel):8.3f} min {min(kernel):8.3f} max {max(kernel):8.3f}   "
            f"call ms median {statistics.median(call):8.3f} min {min(call):8.3f} max {max(call):8.3f}   {extra}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "essential_probe.txt"))
    a = ap.parse_args()
    L.init(0)
    p1, p2, _, out = ec.scene(N, 2000, 0.5, 1)
    lines = [f"scene(5000, 2000, 0.5, 1), threshold {THRESHOLD}, seed {SEED}, refits 4; 2 warm-up calls, {a.reps} timed; {L.device_info()['arch']}"]
    L.kernel_timing(True)
    for H in (16384, 2048):
        r, kernel, call = timed(lambda: L.essential_ransac(p1, p2, K[0], K[1:], THRESHOLD, hypotheses=H, seed=SEED), a.reps)
        lines.append(row(f"essential   H {H:>6} ({10 * H} slots)", kernel, call,
                         f"inliers kept {r['mask'][~out].mean():.4f} outliers kept {r['mask'][out].mean():.4f} splits {r['info']['splits']}"))
        samples = L.epipolar_samples5(N, H, SEED)
        (_, nsol), kernel, call = timed(lambda: L.epipolar_solve5(p1, p2, samples, K[0], K[1:]), a.reps)
        lines.append(row(f"  solve5 alone, H {H:>6}", kernel, call, f"mean solutions per sample {nsol.mean():.2f}"))
    r, kernel, call = timed(lambda: L.epipolar_ransac(p1, p2, THRESHOLD, hypotheses=16384, seed=SEED), a.reps)
    lines.append(row("fundamental H  16384", kernel, call,
                     f"inliers kept {r['mask'][~out].mean():.4f} outliers kept {r['mask'][out].mean():.4f} splits {r['info']['splits']}"))
    L.kernel_timing(False)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
