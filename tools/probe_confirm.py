#!/usr/bin/env python3
"""The argmin confirmation and the mend pass of a float32 point set, the parent commit's library against this one: the same
bits, and what a call costs.  One process holds the parent's libalproj_hip.so twice (a copy under a second name is a library of
its own) and this one once, as tools/probe_mend.py's `off` step does; every step is a process of its own under its own time
limit, and the first step that fails ends the job.  One JSON line per measurement.

  bits   every loss, the argmin and alp_eval_population_mended's four numbers of: the cases of tests/test_gpu_confirm_seams.py;
         the `seams` populations of tests/test_gpu_mend.py with mend on; one near-tie call with mend on.
  time   alternated round by round after a warm-up round, medians: the wall time of alp_eval_population with a near-tied pair
         (K = 2) and a full band (K = 16) on 4 000 and on --points float32 points; the kernel time (alp_eval_population_timing) of
         a mend-on evaluation of tools/probe_mend.py's `pays` population (2048 candidates, sigma = 1) on --points points.
         Bound of a figure: the larger of the two parent instances' medians plus the distance between them.

  python tools/probe_confirm.py --parent-lib PATH [--steps bits,time] [--points 10000000]
"""
import argparse
import ctypes
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import probe_mend as pm                               # noqa: E402
from alproj_amd import _lib as L                      # noqa: E402
from alproj_amd import synthetic as syn               # noqa: E402
from tests import confirm_cases as cc                 # noqa: E402
from tests import mend_cases as mc                    # noqa: E402

STEP_LIMIT_S = {"bits": 300, "time": 420}


class Lib(pm.RawLib):
    def points(self, xyz, origin, obs, w=None, mend=False):
        h = super().points(xyz, origin, obs)
        if w is not None:
            w = np.ascontiguousarray(w)
            self.ok(self.lib.alp_points_set_weights(h, w.ctypes.data_as(ctypes.c_void_p), L.dtype_code(w)))
        self.ok(self.lib.alp_points_set_mend(h, int(mend)))
        return h

    def destroy(self, h):
        self.ok(self.lib.alp_points_destroy(h))

    def evaluate(self, h, cand, kind, fs, want_argmin=True):
        """(losses, argmin, the four numbers of alp_eval_population_mended)"""
        cand = np.ascontiguousarray(cand, dtype=np.float64)
        losses, amin, info = np.empty(len(cand)), ctypes.c_int64(-1), (ctypes.c_int64 * 4)()
        self.ok(self.lib.alp_eval_population(h, L.as_dp(cand), len(cand), kind, fs, L.as_dp(losses), ctypes.byref(amin) if want_argmin else None))
        self.ok(self.lib.alp_eval_population_mended(h, info))
        return losses, int(amin.value), tuple(int(v) for v in info)

    def kernel_ms(self, h):
        k, a = ctypes.c_float(), ctypes.c_float()
        self.ok(self.lib.alp_eval_population_timing(h, ctypes.byref(k), ctypes.byref(a)))
        return k.value


def libraries(parent_lib):
    with tempfile.TemporaryDirectory() as tmp:
        second = os.path.join(tmp, "libalproj_hip_parent_b.so")
        shutil.copy(parent_lib, second)
        return [("parent_a", Lib(parent_lib)), ("this", Lib(L.LIB_PATH)), ("parent_b", Lib(second))]


def same(results):
    (l0, a0, i0) = results[0]
    return all(np.array_equal(l0.view(np.int64), l.view(np.int64)) and a0 == a and i0 == i for (l, a, i) in results[1:])


def step_bits(args):
    libs = libraries(args.parent_lib)
    cu = L.device_info()["cu_count"]
    differing, cases, replaced = [], 0, {}

    def compare(name, xyz, uv, w, mend, cand, kind, fs):
        nonlocal cases
        res = []
        for _, lib in libs:
            h = lib.points(xyz, cc.ORIGIN, uv, w, mend)
            res.append(lib.evaluate(h, cand, kind, fs))
            if lib is libs[1][1]:
                plain = lib.evaluate(h, cand, kind, fs, want_argmin=False)[0]
                replaced[name] = int(np.count_nonzero(plain.view(np.int64) != res[-1][0].view(np.int64)))
            lib.destroy(h)
        cases += 1
        if not same(res):
            differing.append(name)

    for n_name, n in cc.point_counts(cu).items():
        for weighted in (False, True):
            xyz, uv, w = cc.scene(n, weighted)
            for band in cc.BANDS:
                cand, _ = cc.population(band)
                for loss, (kind, fs) in cc.LOSSES.items():
                    compare(f"confirm n={n} {'weighted' if weighted else 'unweighted'} band={band} {loss}", xyz, uv, w, False, cand, kind, fs)
    confirm_cases = cases
    bands_seen = sorted(set(replaced.values()))
    xyz, uv = mc.scene()
    for v in mc.VARIANTS:
        tame, wild = mc.populations(v)
        for which, flagged in mc.flagged_sets().items():
            for loss, (kind, fs) in mc.LOSSES.items():
                compare(f"mend {v} {which} {loss}", xyz.astype(np.float32), uv.astype(np.float32), None, True, mc.mix(tame, wild, flagged), kind, fs)
    xyz, uv, w = cc.scene(1000, True)
    compare("near tie (band 16, weighted, huber) with mend on", xyz, uv, w, True, cc.population(16)[0], *cc.LOSSES["huber"])
    print(json.dumps({"step": "bits", "libraries": [n for n, _ in libs], "cu_count": cu, "cases": cases, "confirmation_cases": confirm_cases,
                      "losses_replaced_by_the_confirmation": bands_seen, "cases_with_differing_bits": differing,
                      "condition": "no differing bit", "holds": not differing}), flush=True)
    return 1 if differing else 0


def near_tie_population(base_vec, band):
    """cc.population's layout around another camera"""
    cand = np.tile(base_vec, (2 * band + 1, 1))
    near = np.arange(1, 2 * band, 2)
    cand[near, cc.K_PAN] += cc.NUDGE_DEG * np.arange(band)
    worse = np.setdiff1d(np.arange(len(cand)), near)
    cand[worse, cc.K_PAN] += np.random.default_rng(43).uniform(0.05, 0.5, len(worse))
    return cand


def figure(what, fig, ms, rounds, **more):
    a, b = float(np.median(ms["parent_a"])), float(np.median(ms["parent_b"]))
    med = float(np.median(ms["this"]))
    bound = max(a, b) + abs(a - b)
    allp = ms["parent_a"] + ms["parent_b"]
    print(json.dumps(dict({"step": "time", "what": what, "figure": fig, "rounds": rounds, "ms": ms, "parent_a_median_ms": round(a, 5),
                           "parent_b_median_ms": round(b, 5), "bound_ms": round(bound, 5), "this_median_ms": round(med, 5),
                           "this_over_parent_median": round(med / float(np.median(allp)), 4),
                           "bound_of_all_parent_rounds_ms": round(2 * max(allp) - min(allp), 5),
                           "condition": "this_median <= max(parent medians) + |parent_a median - parent_b median|",
                           "holds": bool(med <= bound)}, **more)), flush=True)


def step_time(args):
    libs = libraries(args.parent_lib)
    kind, fs = cc.LOSSES["huber"]
    sets = []
    xyz, uv, _ = cc.scene(4000, False)
    sets.append((4000, xyz, cc.ORIGIN, uv, L.params_vector(dict(cc.local_truth(), pan=cc.local_truth()["pan"] + 0.02)), 200))
    big, base, obs = pm.dsm(args.points)
    origin = [base["x"], base["y"], base["z"]]
    n_side = syn.grid_side(args.points)           # the near ties sit next to the pose that made dsm()'s observations
    truth = syn.local_params(syn.perturbed(syn.standoff_params(n_side)), syn.surface(n_side)["offsets"])
    sets.append((len(big), big, origin, obs, L.params_vector(dict(truth, pan=truth["pan"] + 0.02)), 10))
    for n, xyz, o, uv, base_vec, calls in sets:
        handles = [lib.points(xyz, o, uv) for _, lib in libs]
        for band in (2, cc.CONFIRM_MAX):
            cand = near_tie_population(base_vec, band)
            plain = libs[1][1].evaluate(handles[1], cand, kind, fs, want_argmin=False)[0]
            ms = {who: [] for who, _ in libs}
            first, equal, confirmed = None, True, 0
            for rnd in range(args.rounds + 1):
                for (who, lib), h in zip(libs, handles):
                    t = []
                    for _ in range(calls):
                        t0 = time.perf_counter()
                        res = lib.evaluate(h, cand, kind, fs)
                        t.append((time.perf_counter() - t0) * 1e3)
                    if rnd:
                        ms[who].append(round(float(np.median(t)), 5))
                    first = res if first is None else first
                    equal = equal and same([first, res])
                    confirmed = int(np.count_nonzero(res[0] != plain))
            assert confirmed == band, f"the confirmation replaced {confirmed} losses of a band meant to hold {band}"
            figure("alp_eval_population", "call_wall_ms", ms, args.rounds, points=n, candidates=len(cand), near_tied=band,
                   losses_replaced_by_the_confirmation=confirmed, calls_per_round=calls, bits_equal=bool(equal))
        if n == 4000:
            for (_, lib), h in zip(libs, handles):
                lib.destroy(h)
    # the mend pass on the large set
    opt, expand = pm.sampler(base, 21, 2048)
    cand = expand(opt.ask_population())
    for (_, lib), h in zip(libs, handles):
        lib.ok(lib.lib.alp_points_set_mend(h, 1))
    ms = {who: [] for who, _ in libs}
    first, equal = None, True
    for rnd in range(args.rounds + 1):
        for (who, lib), h in zip(libs, handles):
            t = []
            for _ in range(args.reps):
                res = lib.evaluate(h, cand, kind, fs, want_argmin=False)
                t.append(lib.kernel_ms(h))
            if rnd:
                ms[who].append(round(float(np.mean(t)), 4))
            first = res if first is None else first
            equal = equal and np.array_equal(first[0].view(np.int64), res[0].view(np.int64)) and first[2][0] == res[2][0]
    figure("mend-on evaluation", "kernel_ms", ms, args.rounds, points=len(big), candidates=len(cand), flagged=first[2][0],
           mend_grid=list(first[2][2:]), evaluations_per_round=args.reps, bits_equal=bool(equal))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--steps", default="bits,time")
    ap.add_argument("--step", default=None, help="(internal) run this step in this process")
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if args.step:
        L.init(0)
        return {"bits": step_bits, "time": step_time}[args.step](args)
    for step in args.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--parent-lib", os.path.abspath(args.parent_lib), "--points",
               str(args.points), "--rounds", str(args.rounds), "--reps", str(args.reps)]
        try:
            rc = subprocess.run(cmd, timeout=STEP_LIMIT_S[step]).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:                        # nothing more is started on the GPU after a step that failed
            print(json.dumps({"step": step, "failed": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
