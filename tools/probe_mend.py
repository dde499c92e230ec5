#!/usr/bin/env python3
"""What the mend pass of a float32 point set (alp_points_set_mend) costs and what it buys.  One JSON line per measurement; every
step is a process of its own under its own time limit, and the first step that fails ends the job.

  off    mend off costs nothing: kernel ms per evaluation (HIP events: alp_eval_population_timing) of this library with mend off
         against the parent commit's library (--parent-lib: built beside this one).  The parent's library is loaded TWICE (a
         copy under a second name is a library of its own: own code pages, own point set) and this one once, all three into ONE
         process on the same points, uploaded in the order parent A, this, parent B and evaluated A, this, B, A, this, B, ...
         The margin is the spread of parent against parent: every round of both of its instances.
         Shapes: 10 M x 2048 D = 21 and 10 M x 256 D = 9, a fixed generation-0 population at sigma = 1.
  pays   tools/probe_cma_nonfinite.py's loop -- 10 M, pop 2048, D = 21, sigma = 1, 12 generations, seed 1234 -- in float32 with
         mend off, float32 with mend on and float64: flagged and non-finite candidates and kernel ms per generation, summed.
  empty  the pass with nothing to do: kernel ms per evaluation with mend on against mend off on a population without a
         non-finite loss (sigma = 0.01), at both shapes; and ms per generation of the device loop at the GCP size (1127
         points, pop 50, D = 9, float32), mend on against mend off.

  python tools/probe_mend.py [--parent-lib PATH] [--steps off,pays,empty] [--points 10000000]
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
sys.path.insert(0, ROOT)
from alproj_amd import _lib as L                     # noqa: E402
from alproj_amd import synthetic as syn              # noqa: E402
from alproj_amd.cma import CMA                       # noqa: E402
from alproj_amd.optimize import bounds_to_array      # noqa: E402

STEP_LIMIT_S = {"off": 420, "pays": 420, "empty": 420}
SHAPES = {"10Mx2048_d21": (2048, 21), "10Mx256_d9": (256, 9)}
NEW_ENTRY_POINTS = ("alp_points_set_mend", "alp_eval_population_mended")


def dsm(n_points):
    """the DSM-shaped point set of tools/probe_cma_nonfinite.py: (xyz local float32, base params, observations)"""
    n_side = syn.grid_side(n_points)
    s = syn.surface(n_side)
    xyz = syn.vert_to_xyz_local(s["vert"])
    base = syn.local_params(syn.standoff_params(n_side), s["offsets"])
    truth = syn.local_params(syn.perturbed(syn.standoff_params(n_side)), s["offsets"])
    with L.Points(xyz, [base["x"], base["y"], base["z"]], "f32") as pts:
        pts.project(L.params_vector(truth))
        u, v = pts.fetch(np.float32)
    obs = np.stack([u, v], 1) + np.random.default_rng(1).normal(0, 1, (len(u), 2)).astype(np.float32)
    obs[~np.isfinite(obs)] = 0
    return xyz, base, obs


def sampler(base, dims, pop, sigma=1.0, seed=1234):
    targets = syn.TARGETS_D21 if dims == 21 else syn.TARGETS_D9
    bounds = bounds_to_array(base, targets)
    cols = [L.PARAM_KEYS.index(t) for t in targets]
    opt = CMA(mean=np.full(len(targets), 0.5), sigma=sigma, bounds=np.column_stack([np.zeros(len(targets)), np.ones(len(targets))]),
              population_size=pop, n_max_resampling=100, seed=seed, sampler=L.cma_sample)

    def expand(X):
        cand = np.tile(L.params_vector(base), (pop, 1))
        cand[:, cols] = X * (bounds[:, 1] - bounds[:, 0]) + bounds[:, 0]
        return cand

    return opt, expand


class RawLib:
    """a libalproj_hip.so by path, through the C ABI alone (the parent's has no mend entry points)"""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        for name, args in L._SIGNATURES.items():
            if hasattr(self.lib, name):
                fn = getattr(self.lib, name)
                fn.argtypes, fn.restype = args, L._RESTYPE.get(name, ctypes.c_int)
        self.ok(self.lib.alp_init(0))

    def ok(self, rc):
        if rc:
            raise RuntimeError(f"rc {rc}: {(self.lib.alp_last_error() or b'').decode(errors='replace')}")

    def points(self, xyz, origin, obs):
        h = ctypes.c_void_p()
        xyz, obs = np.ascontiguousarray(xyz), np.ascontiguousarray(obs)
        o = np.ascontiguousarray(origin, dtype=np.float64)
        self.ok(self.lib.alp_points_create(xyz.ctypes.data_as(ctypes.c_void_p), L.dtype_code(xyz), len(xyz), L.as_dp(o), L.ALP_F32,
                                           ctypes.byref(h)))
        self.ok(self.lib.alp_points_set_observed(h, obs.ctypes.data_as(ctypes.c_void_p), L.dtype_code(obs)))
        return h

    def kernel_ms(self, h, cand, reps):
        """mean kernel ms of `reps` evaluations (one more first, not counted)"""
        losses = np.empty(len(cand))
        k, a = ctypes.c_float(), ctypes.c_float()
        total = 0.0
        for r in range(reps + 1):
            self.ok(self.lib.alp_eval_population(h, L.as_dp(cand), len(cand), L.LOSS_HUBER, 10.0, L.as_dp(losses), None))
            self.ok(self.lib.alp_eval_population_timing(h, ctypes.byref(k), ctypes.byref(a)))
            total += k.value if r else 0.0
        return total / reps, losses


def step_off(args):
    if not args.parent_lib:
        raise SystemExit("the off step needs --parent-lib")
    xyz, base, obs = dsm(args.points)
    origin = [base["x"], base["y"], base["z"]]
    with tempfile.TemporaryDirectory() as tmp:
        second = os.path.join(tmp, "libalproj_hip_parent_b.so")
        shutil.copy(args.parent_lib, second)
        libs = [("parent_a", RawLib(args.parent_lib)), ("this_mend_off", RawLib(L.LIB_PATH)), ("parent_b", RawLib(second))]
    assert [hasattr(lib.lib, NEW_ENTRY_POINTS[0]) for _, lib in libs] == [False, True, False]
    handles = [lib.points(xyz, origin, obs) for _, lib in libs]
    for shape, (pop, dims) in SHAPES.items():
        opt, expand = sampler(base, dims, pop)
        cand = expand(opt.ask_population())
        ms = {who: [] for who, _ in libs}
        same, first = True, None
        for rnd in range(args.rounds + 1):
            for (who, lib), h in zip(libs, handles):
                t, losses = lib.kernel_ms(h, cand, args.reps)
                ms[who].append(round(t, 4))
                first = losses if first is None else first
                same = same and np.array_equal(first, losses, equal_nan=True)
        parents = ms["parent_a"] + ms["parent_b"]
        lo, hi = min(parents), max(parents)
        med = float(np.median(ms["this_mend_off"]))
        print(json.dumps({"step": "off", "shape": shape, "points": len(xyz), "evaluations_per_round": args.reps, "kernel_ms": ms,
                          "parent_min_ms": lo, "parent_max_ms": hi, "parent_spread_ms": round(hi - lo, 4), "this_median_ms": round(med, 4),
                          "this_over_parent_median": round(med / float(np.median(parents)), 5),
                          "inside_parent_spread": bool(lo <= med <= hi), "above_parent_max": bool(med > hi),
                          "losses_bit_equal": bool(same)}), flush=True)


def step_pays(args):
    xyz, base, obs = dsm(args.points)
    origin = [base["x"], base["y"], base["z"]]
    runs = {}
    for mode, prec, mend in (("f32_mend_off", "f32", False), ("f32_mend_on", "f32", True), ("f64", "f64", False)):
        with L.Points(xyz, origin, prec) as pts:
            pts.set_observed(obs)
            pts.set_mend(mend)
            opt, expand = sampler(base, 21, 2048)
            cand = expand(opt.ask_population())
            pts.eval_population(cand, L.LOSS_HUBER, 10.0, want_argmin=False)        # warm-up: the first launch of every kernel
            opt, expand = sampler(base, 21, 2048)
            rows = []
            for g in range(args.generations):
                X = opt.ask_population()
                losses, _ = pts.eval_population(expand(X), L.LOSS_HUBER, 10.0, want_argmin=False)
                rows.append({"kernel_ms": round(pts.eval_population_timing()[0], 3), "flagged": pts.eval_population_mended()[0],
                             "inf": int(np.isinf(losses).sum()), "nan": int(np.isnan(losses).sum()), "best": float(np.nanmin(losses))})
                opt.tell_population(X, losses)
            runs[mode] = rows
            print(json.dumps({"step": "pays", "mode": mode, "points": len(xyz), "population": 2048, "dims": 21, "sigma": 1.0,
                              "kernel_ms_sum": round(sum(r["kernel_ms"] for r in rows), 3), "generations": rows}), flush=True)
    on, f64 = runs["f32_mend_on"], runs["f64"]
    print(json.dumps({"step": "pays", "mode": "verdict",
                      "f32_mend_on_kernel_ms_sum": round(sum(r["kernel_ms"] for r in on), 3),
                      "f64_kernel_ms_sum": round(sum(r["kernel_ms"] for r in f64), 3),
                      "mend_on_below_f64": bool(sum(r["kernel_ms"] for r in on) < sum(r["kernel_ms"] for r in f64)),
                      "finite_wherever_f64_is": bool(all(a["inf"] + a["nan"] == 0 for a, b in zip(on, f64) if b["inf"] + b["nan"] == 0))}),
          flush=True)


def step_empty(args):
    xyz, base, obs = dsm(args.points)
    with L.Points(xyz, [base["x"], base["y"], base["z"]], "f32") as pts:
        pts.set_observed(obs)
        for shape, (pop, dims) in SHAPES.items():
            opt, expand = sampler(base, dims, pop, sigma=0.01)
            cand = expand(opt.ask_population())
            ms = {"mend_off": [], "mend_on": []}
            grid = None
            for rnd in range(2 * args.rounds + 1):
                on = rnd % 2 == 1
                pts.set_mend(on)
                total = 0.0
                for r in range(args.reps + 1):
                    losses, _ = pts.eval_population(cand, L.LOSS_HUBER, 10.0, want_argmin=False)
                    total += pts.eval_population_timing()[0] if r else 0.0
                assert np.isfinite(losses).all() and pts.eval_population_mended()[0] == 0
                ms["mend_on" if on else "mend_off"].append(round(total / args.reps, 4))
                grid = pts.eval_population_mended()[2:] if on else grid
            print(json.dumps({"step": "empty", "shape": shape, "points": len(xyz), "variant": pts.eval_population_info()[0],
                              "kernel_ms": ms, "mend_grid": grid,
                              "empty_pass_ms": round(float(np.median(ms["mend_on"]) - np.median(ms["mend_off"])), 4)}), flush=True)
    # the GCP size in the device loop: wall time of G generations, enqueued at once
    tp = syn.truth_params(316)
    gx = syn.gcp_points(1127, tp, seed=3)
    with L.Points(gx, [tp["x"], tp["y"], tp["z"]], "f64") as gp:
        gp.project(L.params_vector(tp))
        gu, gv = gp.fetch()
    guv = np.stack([gu, gv], 1) + np.random.default_rng(3).normal(0, 1.0, (1127, 2))
    init = dict(tp, pan=tp["pan"] + 2, tilt=tp["tilt"] - 1.5, fov=tp["fov"] + 3, x=tp["x"] + 4, **{k: 0.0 for k in syn.TARGETS_D21[9:]})
    b = bounds_to_array(init, syn.TARGETS_D9)
    idx = [L.PARAM_KEYS.index(t) for t in syn.TARGETS_D9]
    G = 1000
    with L.Points(gx, [init["x"], init["y"], init["z"]], "f32") as pts:
        pts.set_observed(guv)
        ms = {"mend_off": [], "mend_on": []}
        counts = []
        for rnd in range(2 * args.rounds + 1):
            on = rnd % 2 == 1
            pts.set_mend(on)
            host = CMA(mean=np.full(9, 0.5), sigma=0.05, bounds=np.column_stack([np.zeros(9), np.ones(9)]), population_size=50,
                       n_max_resampling=100, seed=7, sampler=L.cma_sample)
            with L.CmaDevice(pts, L.params_vector(init), idx, b[:, 0], b[:, 1], host) as loop:
                host.set_state(dict(host.get_state(), mean=(np.array([init[t] for t in syn.TARGETS_D9]) - b[:, 0]) / (b[:, 1] - b[:, 0])))
                loop.set_state(host.get_state())
                loop.run(20, L.LOSS_HUBER, 10.0)
                loop.wait()
                t0 = time.perf_counter()
                loop.run(G, L.LOSS_HUBER, 10.0)
                loop.wait()
                ms["mend_on" if on else "mend_off"].append(round((time.perf_counter() - t0) / G * 1e3, 5))
                if on:
                    counts.append(pts.eval_population_mended()[:2])
        print(json.dumps({"step": "empty", "shape": "gcp_device_loop", "points": 1127, "population": 50, "dims": 9, "precision": "f32",
                          "generations": G, "ms_per_generation": ms, "flagged_last_and_total": counts,
                          "empty_pass_ms": round(float(np.median(ms["mend_on"]) - np.median(ms["mend_off"])), 5)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--steps", default="off,pays,empty")
    ap.add_argument("--step", default=None, help="(internal) run this step in this process")
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--generations", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.step:
        L.init(0)
        {"off": step_off, "pays": step_pays, "empty": step_empty}[args.step](args)
        return 0
    for step in args.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--points", str(args.points), "--generations",
               str(args.generations), "--rounds", str(args.rounds), "--reps", str(args.reps)]
        if args.parent_lib:
            cmd += ["--parent-lib", os.path.abspath(args.parent_lib)]
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
