#!/usr/bin/env python3
"""The match filters of alp_epipolar.hip, the parent commit's library against this one: the same registers, the same bits, and
what a call costs.  As tools/probe_confirm.py does it: one process holds the parent's libalproj_hip.so twice (a copy under a
second name is a library of its own) and this one once; every step is a process of its own under its own time limit, and the
first step that fails ends the job.  --out is written anew; every step appends its section to it.

  usage  no GPU: the kernel-resource-usage remarks of the unit's kernels, the parent's compile log (--parent-log, the
         build/alp_epipolar.o.log of a build of the parent) next to this build's.  The hot kernels must keep VGPRs, AGPRs, scratch,
         LDS and occupancy; no kernel may use scratch or lose occupancy.
  bits   raw bytes, NaNs included, of F, mask, info[24] and stats[12] of the four whole filters and of the outputs of
         alp_epipolar_samples, _samples5, _solve8, _solve5, _score, _select and _mask, at every seam: n in 8, 9, 511, 512, 513,
         1025 (essential: 5 and 6 as well), H in 1, 255, 256, 257, splits 0 (planned), 1, 2 and the tile count, refits in 0, 1, 4,
         8, samples given and drawn; a keep_all case of every filter; the LMEDS_SCENES and LMEDS5_SCENES rows of tests/lmeds_cases.py.
         No LMEDS5_SCENES row keeps a refit in either essential filter, so the step asks instead that every filter keeps a refit in
         some compared call: the accept path of the essential filters is held by grid scenes of es.make_scene, by no named fixture.
  time   alternated round by round after a warm-up round, medians of the kernel sections (alp_kernel_timing) and of the whole
         call: the four filters at n = 5000, H = 16384, refits = 4, and alp_epipolar_score / _select at tools/probe_lmeds.py's
         three shapes.  Bound of a figure: the larger of the two parent instances' medians plus the distance between them.
         Not tools/probe_confirm.py's one process in the order parent_a, this, parent_b: three processes, one per rotation of
         the order in which the libraries are loaded and called, pooled (see step_time).  The last columns show what identical
         code does: the lowest and highest round of the two parent instances.

  python tools/probe_epipolar_parity.py --parent-lib PATH [--parent-log PATH] [--steps usage,bits,time] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
from alproj_amd import _lib as L                      # noqa: E402
import epipolar_cases as ec                           # noqa: E402
import essential_cases as es                          # noqa: E402
import lmeds_cases as lc                              # noqa: E402

STEP_LIMIT_S = {"usage": 60, "bits": 420, "time": 420}
HOT = ("epi_score_kernel", "epi_select_kernel", "epi_solve_kernel", "epi_solve5_kernel", "epi_accum_kernel", "epi_refit_kernel",
       "epi_select_merge_kernel")
FIELDS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
I32P, U8P, I64P = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int64)
FILTERS = ("alp_epipolar_ransac", "alp_essential_ransac", "alp_epipolar_lmeds", "alp_essential_lmeds")


# ------------------------------------------------------------------------------------------------------------ usage
def usage_of(log):
    """{kernel: {field: value}} of one compile log; a template's first integer argument is kept with the name"""
    out, cur = {}, None
    for line in open(log):
        if "remark:" not in line or "[-Rpass-analysis" not in line:
            continue
        body = line.split("remark:", 1)[1].split("[-Rpass")[0].strip()
        if body.startswith("Function Name:"):
            mangled = body.split(":", 1)[1].strip()
            m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", mangled)
            cur = mangled[m.end():m.end() + int(m.group(1))] if m else mangled
            t = re.search(r"ILi(\d+)E", mangled)
            cur += f"<{t.group(1)}>" if t else ""
            out[cur] = {}
        elif cur and ":" in body:
            k, v = body.split(":", 1)
            out[cur][k.strip()] = v.strip()
    return out


def step_usage(args, say):
    parent, this = usage_of(args.parent_log), usage_of(os.path.join(ROOT, "build", "alp_epipolar.o.log"))
    say("== kernel resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), parent -> this where they differ")
    say(f"{'kernel':<28}{'VGPRs':>9}{'AGPRs':>7}{'SGPRs':>9}{'scratch B':>11}{'LDS B':>9}{'waves/SIMD':>12}")
    bad = []
    for k in sorted(set(parent) | set(this)):
        a, b = parent.get(k, {}), this.get(k, {})
        row = [a.get(f, "-") if a.get(f, "-") == b.get(f, "-") else f"{a.get(f, '-')}->{b.get(f, '-')}" for f in FIELDS]
        say(f"{k:<28}{row[0]:>9}{row[1]:>7}{row[2]:>9}{row[3]:>11}{row[4]:>9}{row[5]:>12}")
        if k in HOT and any(a.get(f) != b.get(f) for f in FIELDS if f != "TotalSGPRs"):
            bad.append(k + ": a hot kernel moved")
        if b and (int(b[FIELDS[3]]) != 0 or (a and int(b[FIELDS[5]]) < int(a[FIELDS[5]]))):
            bad.append(k + ": scratch, or occupancy lost")
    say(f"condition: {', '.join(HOT)} keep every figure but SGPRs; no kernel uses scratch or loses occupancy: "
        f"{'holds' if not bad else 'FAILS: ' + '; '.join(bad)}")
    return 1 if bad else 0


# ------------------------------------------------------------------------------------------------------------ the C ABI
class Lib:
    """a libalproj_hip.so by path, through the C ABI alone; every method returns the raw bytes of what the call wrote"""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        for name, sig in L._SIGNATURES.items():
            if hasattr(self.lib, name):
                fn = getattr(self.lib, name)
                fn.argtypes, fn.restype = sig, L._RESTYPE.get(name, ctypes.c_int)
        self.ok(self.lib.alp_init(0))
        self.ok(self.lib.alp_kernel_timing(1))

    def ok(self, rc):
        if rc:
            raise RuntimeError(f"rc {rc}: {(self.lib.alp_last_error() or b'').decode(errors='replace')}")

    def kernel_ms(self):
        ms, n = ctypes.c_float(), ctypes.c_int()
        self.ok(self.lib.alp_kernel_time_ms(ctypes.byref(ms), ctypes.byref(n)))
        return ms.value

    def filter(self, name, p1, p2, samples, H, seed, K, criterion, refits, splits):
        """K: None or 3 doubles; criterion: (threshold,) or (rank, scale2, floor2) -> (F, mask, info, stats) as bytes"""
        F, mask = np.full(9, 7.0), np.full(len(p1), 7, dtype=np.uint8)
        info, stats = np.full(24, 7, dtype=np.int64), np.full(12, 7.0)
        a = [L.as_dp(p1), L.as_dp(p2), len(p1), samples.ctypes.data_as(I32P) if samples is not None else None, H, seed]
        a += [L.as_dp(K)] if K is not None else []
        a += list(criterion) + [refits, splits, L.as_dp(F), mask.ctypes.data_as(U8P), info.ctypes.data_as(I64P)]
        a += [L.as_dp(stats)] if len(criterion) == 3 else []
        self.ok(getattr(self.lib, name)(*a))
        return F.tobytes(), mask.tobytes(), info.tobytes(), stats.tobytes()

    def samples(self, width, n, H, seed):
        out = np.full((H, width), -7, dtype=np.int32)
        self.ok((self.lib.alp_epipolar_samples if width == 8 else self.lib.alp_epipolar_samples5)(n, H, seed, out.ctypes.data_as(I32P)))
        return (out.tobytes(),)

    def solve(self, p1, p2, samples, K):
        H = len(samples)
        if K is None:
            F = np.full((H, 9), 7.0)
            self.ok(self.lib.alp_epipolar_solve8(L.as_dp(p1), L.as_dp(p2), len(p1), samples.ctypes.data_as(I32P), H, L.as_dp(F)))
            return (F.tobytes(),)
        F, nsol = np.full((H, 90), 7.0), np.full(H, -7, dtype=np.int32)
        self.ok(self.lib.alp_epipolar_solve5(L.as_dp(p1), L.as_dp(p2), len(p1), samples.ctypes.data_as(I32P), H, L.as_dp(K), L.as_dp(F),
                                             nsol.ctypes.data_as(I32P)))
        return F.tobytes(), nsol.tobytes()

    def score(self, p1, p2, F, threshold, splits):
        counts, info = np.full(len(F), -7, dtype=np.int32), np.full(6, 7, dtype=np.int64)
        self.ok(self.lib.alp_epipolar_score(L.as_dp(p1), L.as_dp(p2), len(p1), L.as_dp(F), len(F), threshold, splits, counts.ctypes.data_as(I32P),
                                            info.ctypes.data_as(I64P)))
        return counts.tobytes(), info.tobytes()

    def select(self, p1, p2, F, rank, splits):
        value, info = np.full(len(F), 7.0), np.full(8, 7, dtype=np.int64)
        self.ok(self.lib.alp_epipolar_select(L.as_dp(p1), L.as_dp(p2), len(p1), L.as_dp(F), len(F), rank, splits, L.as_dp(value),
                                             info.ctypes.data_as(I64P)))
        return value.tobytes(), info.tobytes()

    def mask(self, p1, p2, F, threshold):
        mask, err = np.full(len(p1), 7, dtype=np.uint8), np.full(len(p1), 7.0)
        self.ok(self.lib.alp_epipolar_mask(L.as_dp(p1), L.as_dp(p2), len(p1), L.as_dp(F), threshold, mask.ctypes.data_as(U8P), L.as_dp(err)))
        return mask.tobytes(), err.tobytes()


def libraries(parent_lib, rotation=0):
    """[(role, library)] in the order in which they were loaded: parent_a, this, parent_b, rotated left by `rotation`"""
    with tempfile.TemporaryDirectory() as tmp:
        second = os.path.join(tmp, "libalproj_hip_parent_b.so")
        shutil.copy(parent_lib, second)
        order = [("parent_a", parent_lib), ("this", L.LIB_PATH), ("parent_b", second)]
        return [(role, Lib(path)) for role, path in order[rotation:] + order[:rotation]]


def criterion_of(name, n, m):
    """the filter's own numbers: threshold 3 px, or the median's rank and scale (n = m has no scale: 14, about its limit)"""
    if name.endswith("ransac"):
        return (3.0,)
    return (L.lmeds_rank(n, m), L.lmeds_scale2(n, m) if n > m else 14.0, 1.0)


# ------------------------------------------------------------------------------------------------------------ bits
def step_bits(args, say):
    libs = libraries(args.parent_lib)
    K = np.array(es.K_TRUE, dtype=np.float64)
    differing, cases, seen = [], 0, {"keep_all": 0, "stopped_early": 0}
    kept_a_refit = {name: 0 for name in FILTERS}       # calls of each filter that kept at least one refit

    def compare(what, call):
        nonlocal cases
        res = [call(lib) for _, lib in libs]
        cases += 1
        if any(r != res[0] for r in res[1:]) and len(differing) < 20:
            differing.append(what)
        return res[1]

    def whole(what, name, p1, p2, samples, H, seed, refits, splits, criterion=None):
        m = 5 if "essential" in name else 8
        cr = criterion or criterion_of(name, len(p1), m)
        r = compare(f"{name} {what}", lambda lib: lib.filter(name, p1, p2, samples, H, seed, K if m == 5 else None, cr, refits, splits))
        info = np.frombuffer(r[2], dtype=np.int64)
        seen["keep_all"] += int(info[5])
        kept_a_refit[name] += int(info[4] > 0)
        seen["stopped_early"] += int(info[3] < refits and not info[5])
        return info

    for m, make, ns in ((8, ec.scene, (8, 9, 511, 512, 513, 1025)), (5, es.make_scene, (5, 6, 8, 9, 511, 512, 513, 1025))):
        Kc = K if m == 5 else None
        for n in ns:
            p1, p2, Ftrue, _ = make(n, int(0.3 * n), 0.5, 3)
            tiles = (n + 511) // 512
            all_splits = sorted({0, 1, min(2, tiles), tiles})
            alone = n >= 8             # alp_epipolar_mask, _score and _select take 8 matches or more
            if alone:
                compare(f"mask n={n}", lambda lib: lib.mask(p1, p2, np.ascontiguousarray(Ftrue).reshape(9), 3.0))
            for H in (1, 255, 256, 257):
                rng = np.random.default_rng(100 * n + H)
                given = np.stack([rng.choice(n, m, replace=False) for _ in range(H)]).astype(np.int32)
                compare(f"samples{m} n={n} H={H}", lambda lib: lib.samples(m, n, H, 11))
                Fs = compare(f"solve{m} n={n} H={H}", lambda lib: lib.solve(p1, p2, given, Kc))[0]
                Fs = np.frombuffer(Fs, dtype=np.float64).reshape(-1, 9)
                for splits in all_splits:
                    if alone:
                        compare(f"score m={m} n={n} H={len(Fs)} splits={splits}", lambda lib: lib.score(p1, p2, Fs, 3.0, splits))
                        compare(f"select m={m} n={n} H={len(Fs)} splits={splits}", lambda lib: lib.select(p1, p2, Fs, L.lmeds_rank(n, m), splits))
                    for name in FILTERS:
                        if ("essential" in name) != (m == 5):
                            continue
                        for refits in (0, 1, 4, 8):
                            for samples in (given, None):
                                whole(f"n={n} H={H} splits={splits} refits={refits} samples={'given' if samples is not None else 'drawn'}",
                                      name, p1, p2, samples, H, 11, refits, splits)
    grid_cases = cases
    # keep_all: RANSAC on matches that are all outliers at the bound 0, which no eight (five) matches meet; LMedS on matches that are one point, whose
    # every sample is degenerate, every hypothesis NaN and every value infinite
    p1, p2, _, _ = ec.scene(64, 64, 0.5, 5)
    one = np.ascontiguousarray(np.tile([[100.0, 200.0]], (64, 1)))
    kept = {}
    for name in FILTERS:
        a, b, cr = (p1, p2, (0.0,)) if name.endswith("ransac") else (one, one, None)
        kept[name] = int(whole("keep_all", name, a, b, None, 256, 2, 4, 0, cr)[5])
    # the scenes of tests/lmeds_cases.py, on their own samples: refits kept by each filter, per scene
    scenes = {name: [] for name in FILTERS}
    for i, row in enumerate(lc.LMEDS_SCENES):
        q1, q2, _, samples = lc.fundamental_scene(*row)
        for name in ("alp_epipolar_ransac", "alp_epipolar_lmeds"):
            scenes[name].append(int(whole(f"LMEDS_SCENES[{i}]", name, q1, q2, samples, len(samples), 0, 4, 0)[4]))
    for i, row in enumerate(lc.LMEDS5_SCENES):
        q1, q2, _, samples = lc.essential_scene(*row)
        for name in ("alp_essential_ransac", "alp_essential_lmeds"):
            scenes[name].append(int(whole(f"LMEDS5_SCENES[{i}]", name, q1, q2, samples, len(samples), 0, 4, 0)[4]))
    say("== bits: raw bytes of every output, parent_a / this / parent_b in one process")
    say(f"cases compared: {cases} ({grid_cases} on the grid of seams); whole-filter calls that kept every match: {seen['keep_all']}, "
        f"that stopped before their last round: {seen['stopped_early']}")
    say(f"calls that kept at least one refit: {kept_a_refit}")
    say(f"keep_all flag of the keep_all cases: {kept}")
    say(f"refits kept on every LMEDS_SCENES / LMEDS5_SCENES row: {scenes}")
    ok = not differing and all(kept.values()) and all(kept_a_refit.values())
    say(f"cases with differing bytes: {differing if differing else 'none'}")
    say(f"condition: no differing byte, every keep_all case keeps all, every filter keeps a refit somewhere: {'holds' if ok else 'FAILS'}")
    return 0 if ok else 1


# ------------------------------------------------------------------------------------------------------------ time
def step_time(args, say):
    """One arrangement: the three libraries loaded, and called in every round, in the order parent_a, this, parent_b rotated by
    --rotation.  The place in that order has a cost of its own (a third copy of the parent in the middle place measured 1.5 %
    above its two neighbours on the largest select), so main() runs every rotation, each in a process of its own, and pools
    the rounds: every role has then held every place equally often.  Writes {figure: {role: [round medians]}} to --samples."""
    libs = libraries(args.parent_lib, args.rotation)
    this = dict(libs)["this"]
    K = np.array(es.K_TRUE, dtype=np.float64)
    figures, unequal = {}, []

    def measure(what, call):
        kernel, wall = {w: [] for w, _ in libs}, {w: [] for w, _ in libs}
        first = None
        for rnd in range(args.rounds + 1):
            for who, lib in libs:
                k, c = [], []
                for _ in range(args.reps):
                    lib.kernel_ms()
                    t0 = time.perf_counter()
                    res = call(lib)
                    c.append((time.perf_counter() - t0) * 1e3)
                    k.append(lib.kernel_ms())
                    first = res if first is None else first
                    if res != first and what not in unequal:
                        unequal.append(what)
                if rnd:
                    kernel[who].append(float(np.median(k)))
                    wall[who].append(float(np.median(c)))
        figures[what + "|kernel"], figures[what + "|call"] = kernel, wall

    n = 5000
    p1, p2, _, _ = ec.scene(n, 2000, 0.5, 1)
    for name in FILTERS:
        m = 5 if "essential" in name else 8
        cr = criterion_of(name, n, m)
        measure(f"{name} n=5000 H=16384 refits=4", lambda lib: lib.filter(name, p1, p2, None, 16384, 1, K if m == 5 else None, cr, 4, 0))
    for n, H, m in ((5000, 16384, 8), (512, 256, 8), (5000, 16384, 5)):
        p1, p2, _, _ = ec.scene(n, int(0.4 * n), 0.5, 1)
        samples = np.frombuffer(this.samples(m, n, H, 1)[0], dtype=np.int32).reshape(H, m)
        Fs = np.frombuffer(this.solve(p1, p2, samples, K if m == 5 else None)[0], dtype=np.float64).reshape(-1, 9)
        rank = L.lmeds_rank(n, m)
        measure(f"alp_epipolar_score n={n} H={len(Fs)}", lambda lib: lib.score(p1, p2, Fs, 3.0, 0))
        measure(f"alp_epipolar_select n={n} H={len(Fs)}", lambda lib: lib.select(p1, p2, Fs, rank, 0))
    with open(args.samples, "w") as f:
        json.dump({"order": [w for w, _ in libs], "figures": figures, "bytes_differ": unequal}, f)
    print(f"rotation {args.rotation}: {[w for w, _ in libs]}, {len(figures)} figures, outputs differing: {unequal or 'none'}", flush=True)
    return 1 if unequal else 0


def pool_times(args, say, parts):
    say(f"== time: medians (ms) over {len(parts)} arrangements x {args.rounds} alternated rounds of {args.reps} calls; the three libraries are loaded "
        "and called in the order parent_a, this, parent_b and in its two rotations, so that every role holds every place; "
        "bound = max(parent medians) + |parent_a - parent_b|")
    say(f"{'what':<46}{'figure':<8}{'parent_a':>10}{'parent_b':>10}{'bound':>10}{'this':>10}  holds   parent rounds: lowest  highest")
    failed = []
    for key in parts[0]["figures"]:
        what, fig = key.split("|")
        rounds = {role: sum((p["figures"][key][role] for p in parts), []) for role in ("parent_a", "parent_b", "this")}
        a, b, t = (float(np.median(rounds[role])) for role in ("parent_a", "parent_b", "this"))
        bound = max(a, b) + abs(a - b)
        both = rounds["parent_a"] + rounds["parent_b"]
        say(f"{what:<46}{fig:<8}{a:>10.4f}{b:>10.4f}{bound:>10.4f}{t:>10.4f}  {'yes' if t <= bound else 'NO':<5}{min(both):>25.4f}{max(both):>9.4f}")
        if not t <= bound:
            failed.append(f"{what} {fig}")
    say(f"condition: this median <= bound, every figure: {'holds' if not failed else 'FAILS: ' + '; '.join(failed)}")
    return 1 if failed else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-log", default=None)
    ap.add_argument("--steps", default="bits,time")
    ap.add_argument("--step", default=None, help="(internal) run this step in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epipolar_refactor_parity.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rotation", type=int, default=0, help="(internal) of the time step")
    ap.add_argument("--samples", default=None, help="(internal) where the time step leaves its rounds")
    args = ap.parse_args()
    if args.step:
        if args.step == "usage" and not args.parent_log or args.step != "usage" and not args.parent_lib:
            raise SystemExit("usage needs --parent-log, bits and time need --parent-lib")
        with open(args.out, "a") as f:
            def say(text):
                print(text, flush=True)
                f.write(text + "\n")
                f.flush()
            return {"usage": step_usage, "bits": step_bits, "time": step_time}[args.step](args, say)
    open(args.out, "w").close()
    with tempfile.TemporaryDirectory() as tmp:
        parts = []
        for step in args.steps.split(","):
            for rotation in range(3 if step == "time" else 1):
                cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--out", os.path.abspath(args.out), "--rounds", str(args.rounds),
                       "--reps", str(args.reps), "--rotation", str(rotation), "--samples", os.path.join(tmp, f"time{rotation}.json")]
                cmd += ["--parent-lib", os.path.abspath(args.parent_lib)] if args.parent_lib else []
                cmd += ["--parent-log", os.path.abspath(args.parent_log)] if args.parent_log else []
                try:
                    rc = subprocess.run(cmd, timeout=STEP_LIMIT_S[step]).returncode
                except subprocess.TimeoutExpired:
                    rc = 124
                if rc != 0:                    # nothing more is started on the GPU after a step that failed
                    print(f"step {step} failed: {rc}", flush=True)
                    return rc
                if step == "time":
                    parts.append(json.load(open(os.path.join(tmp, f"time{rotation}.json"))))
        if parts:
            with open(args.out, "a") as f:
                def say(text):
                    print(text, flush=True)
                    f.write(text + "\n")
                return pool_times(args, say, parts)
    return 0


if __name__ == "__main__":
    sys.exit(main())
