#!/usr/bin/env python3
"""alp_normal_equations_batch (normal_poses_kernel: the normal equations of B poses in one launch) against B single calls, and
the normal-equation entry points against the parent commit's.  One process, one JSON line per step:

  small  (a) the GCP size: n = 1127 float64 points, D = 9, B = 64.  One batch call against 64 sequential
             Points.normal_equations calls on the same handle: the median whole-call wall time of --reps repetitions after a
             warm-up.  Condition: batch <= 0.5 x sequential.  The host share of the batch call (the 64 folds, the upload of the
             plans) is reported beside it: wall time less the kernel section.
  large  (b) n = 10 M float64 points, D = 21, B = 8.  The kernel section (alp_kernel_timing) of the batch per pose against the
             single call's, alternated round by round in one process, for BOTH workgroup orders (ALP_NORMAL_BATCH_ORDER =
             stripe | pose: which grid index runs fastest).  Condition, for the order the library ships: the batch's median per
             pose is not above the single call's median by more than the single call's own spread, (max - min) / median.
  single (c) --parent-lib PATH: the parent's library (loaded twice, as tools/probe_mend.py does) and this one in one process.
             Bits: alp_normal_equations (every loss, D = 9 and 23; unweighted and weighted), alp_normal_equations_batch (B = 1, 8,
             64; unweighted and weighted), alp_normal_equations_batch_rows (repeated
             and permuted rows) and one round of the device loop with and without weight rows, read back through alp_lm_get, at
             n = 257 and 100 003, float64 and float32, linear and huber: no bit may differ between the three.  Time, alternated
             round by round: the whole call and the kernel section of alp_normal_equations and alp_normal_equations_batch at the
             GCP size, a round of the device loop with K = 64 there, and the kernel sections of the single, the batch and the
             rows call at --points; this library's median must lie inside the spread of the two parent instances' values.
  solve  (d) recorded only: LsqOptimizer.optimize(method="normal", starts=64, seed=1) on the g14 problem trf_linear_d7 against
             64 single-start runs from the same starts: wall time, kernel time, and the rest split into library calls and host
             solve.

  python tools/probe_normal_batch.py [--steps small,large,single,solve] [--parent-lib PATH] [--reps 30] [--rounds 7]
                                     [--out profiles/normal_batch_probe.jsonl]
"""
import argparse
import ctypes
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alproj_amd import _lib as L                     # noqa: E402
from alproj_amd import synthetic as syn              # noqa: E402
from tools.probe_normal import LENS, TARGETS_D21, observed      # noqa: E402

TARGETS_D9 = ["fov", "pan", "tilt", "roll", "a1", "a2", "k1", "k2", "k3"]
I32 = ctypes.POINTER(ctypes.c_int32)


def problem(n, targets, B, seed):
    """n GCP-like float64 points with observations, the pose they were made with and B poses around it"""
    p = dict(syn.truth_params(316), **LENS)
    pv = L.params_vector(p)
    xyz = syn.gcp_points(n, p, seed=seed)
    u, v = observed(xyz, p, pv, "f64")
    rng = np.random.default_rng(seed)
    cand = np.tile(pv, (B, 1))
    cand[:, L.PARAM_KEYS.index("pan")] += rng.uniform(-0.02, 0.02, B)
    cand[:, L.PARAM_KEYS.index("tilt")] += rng.uniform(-0.02, 0.02, B)
    return xyz, [p["x"], p["y"], p["z"]], (u, v), pv, cand, [L.PARAM_KEYS.index(t) for t in targets]


def spread(v):
    return (max(v) - min(v)) / float(np.median(v))


def step_small(args):
    n, B = 1127, 64
    xyz, origin, (u, v), pv, cand, cols = problem(n, TARGETS_D9, B, 3)
    with L.Points(xyz, origin, "f64") as pts:
        pts.set_observed_columns(u, v)
        batch = lambda: pts.normal_equations_batch(cand, cols)
        seq = lambda: [pts.normal_equations(c, cols) for c in cand]
        got, ref = batch(), seq()
        for _ in range(3):
            batch(), seq()
        L.kernel_timing(True)
        wall = {"batch": [], "sequential": []}
        kern = {"batch": [], "sequential": []}
        for _ in range(args.reps):
            for name, fn in (("batch", batch), ("sequential", seq)):
                L.kernel_time_ms()
                t0 = time.perf_counter()
                fn()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                kern[name].append(L.kernel_time_ms()[0])
        L.kernel_timing(False)
    err = max(float(np.abs(got[0][b] - ref[b][0]).max() / np.abs(ref[b][0]).max()) for b in range(B))
    mb, ms = float(np.median(wall["batch"])), float(np.median(wall["sequential"]))
    return dict(step="small", points=n, columns=len(cols), poses=B, reps=args.reps, batch_call_ms=round(mb, 4),
                sequential_calls_ms=round(ms, 4), ratio=round(mb / ms, 4), condition="ratio <= 0.5", holds=bool(mb <= 0.5 * ms),
                batch_kernel_ms=round(float(np.median(kern["batch"])), 4), sequential_kernel_ms=round(float(np.median(kern["sequential"])), 4),
                batch_host_and_copies_ms=round(mb - float(np.median(kern["batch"])), 4),
                batch_call_spread=round(spread(wall["batch"]), 3), sequential_spread=round(spread(wall["sequential"]), 3),
                max_rel_difference_of_G=err)


def step_large(args):
    n, B = args.points, 8
    xyz, origin, (u, v), pv, cand, cols = problem(n, TARGETS_D21, B, 3)
    shipped = None
    with L.Points(xyz, origin, "f64") as pts:
        pts.set_observed_columns(u, v)
        del xyz
        pts.normal_equations(pv, cols)
        ms = {"single": [], "stripe": [], "pose": [], "default": []}
        results = {}
        L.kernel_timing(True)
        for rnd in range(args.rounds + 1):
            for name in ms:
                if name == "single":
                    fn = lambda: pts.normal_equations(pv, cols)
                    per = 1
                else:
                    if name == "default":
                        os.environ.pop("ALP_NORMAL_BATCH_ORDER", None)
                    else:
                        os.environ["ALP_NORMAL_BATCH_ORDER"] = name
                    fn = lambda: pts.normal_equations_batch(cand, cols)
                    per = B
                L.kernel_time_ms()
                out = fn()
                k = L.kernel_time_ms()[0] / per
                if rnd:                                  # round 0 warms the scratch of every shape
                    ms[name].append(round(k, 4))
                results[name] = out
        os.environ.pop("ALP_NORMAL_BATCH_ORDER", None)
        L.kernel_timing(False)
    same_bits = all(np.array_equal(results["stripe"][k], results[o][k]) for o in ("pose", "default") for k in range(3))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    shipped = min(("stripe", "pose"), key=lambda o: abs(med[o] - med["default"]))
    sp = spread(ms["single"])
    return dict(step="large", points=n, columns=len(cols), poses=B, rounds=args.rounds, kernel_ms_per_pose=ms,
                median_ms_per_pose={k: round(v, 4) for k, v in med.items()}, single_spread=round(sp, 4),
                default_order_is_nearest_to=shipped, batch_over_single=round(med["default"] / med["single"], 4),
                condition="default <= single x (1 + single_spread)", holds=bool(med["default"] <= med["single"] * (1 + sp)),
                orders_give_the_same_bits=bool(same_bits))


class RawLib:
    """a libalproj_hip.so by path, through the C ABI alone"""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        for name, a in L._SIGNATURES.items():
            if hasattr(self.lib, name):
                fn = getattr(self.lib, name)
                fn.argtypes, fn.restype = a, L._RESTYPE.get(name, ctypes.c_int)
        self.ok(self.lib.alp_init(0))

    def ok(self, rc):
        if rc:
            raise RuntimeError(f"rc {rc}: {(self.lib.alp_last_error() or b'').decode(errors='replace')}")

    def points(self, xyz, origin, uv, precision=L.ALP_F64):
        h = ctypes.c_void_p()
        xyz, uv = np.ascontiguousarray(xyz), np.ascontiguousarray(uv)
        o = np.ascontiguousarray(origin, dtype=np.float64)
        self.ok(self.lib.alp_points_create(xyz.ctypes.data_as(ctypes.c_void_p), L.dtype_code(xyz), len(xyz), L.as_dp(o), precision,
                                           ctypes.byref(h)))
        self.ok(self.lib.alp_points_set_observed(h, uv.ctypes.data_as(ctypes.c_void_p), L.dtype_code(uv)))
        return h

    def set_weights(self, h, w):
        w = np.ascontiguousarray(w, dtype=np.float64)
        if w.ndim == 1:
            self.ok(self.lib.alp_points_set_weights(h, w.ctypes.data_as(ctypes.c_void_p), L.ALP_F64))
        else:
            self.ok(self.lib.alp_points_set_weight_table(h, w.ctypes.data_as(ctypes.c_void_p), len(w), L.ALP_F64))

    def normal(self, h, pv, cols, loss=0, rows=None):
        """the raw sums of alp_normal_equations (pv (25,)), alp_normal_equations_batch (pv (B, 25)) or, with `rows`, of
        alp_normal_equations_batch_rows"""
        idx = np.ascontiguousarray(cols, dtype=np.int32)
        d = len(idx)
        pv = np.ascontiguousarray(pv, dtype=np.float64)
        out = np.empty(pv.shape[:-1] + (d * (d + 1) // 2 + d + 2,))
        if pv.ndim == 1:
            self.ok(self.lib.alp_normal_equations(h, L.as_dp(pv), idx.ctypes.data_as(I32), d, loss, 1.0, L.as_dp(out)))
        elif rows is None:
            self.ok(self.lib.alp_normal_equations_batch(h, L.as_dp(pv), len(pv), idx.ctypes.data_as(I32), d, loss, 1.0, L.as_dp(out)))
        else:
            r = np.ascontiguousarray(rows, dtype=np.int32)
            self.ok(self.lib.alp_normal_equations_batch_rows(h, L.as_dp(pv), len(pv), r.ctypes.data_as(I32), idx.ctypes.data_as(I32), d, loss, 1.0,
                                                             L.as_dp(out)))
        return out

    def timed(self, fn, reps):
        """(median wall ms of a call, mean kernel ms of a call) over `reps` calls of fn after one more"""
        ms, cnt = ctypes.c_float(), ctypes.c_int()
        self.ok(self.lib.alp_kernel_timing(1))
        fn()
        self.ok(self.lib.alp_kernel_time_ms(ctypes.byref(ms), ctypes.byref(cnt)))
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t0) * 1e3)
        self.ok(self.lib.alp_kernel_time_ms(ctypes.byref(ms), ctypes.byref(cnt)))
        self.ok(self.lib.alp_kernel_timing(0))
        return float(np.median(wall)), ms.value / reps

    def lm_rounds(self, h, pv, cols, X0, rounds, loss=0, weight_rows=False):
        """a device loop from the starts X0 (K, D), unbounded: (wall ms per round of `rounds` rounds, enqueue to the end of the
        wait; the records read back through alp_lm_get, as one array)"""
        idx = np.ascontiguousarray(cols, dtype=np.int32)
        X0 = np.ascontiguousarray(X0, dtype=np.float64)
        K, D = X0.shape
        lo, hi = np.full(D, -np.inf), np.full(D, np.inf)
        loop = ctypes.c_void_p()
        create = self.lib.alp_lm_create_rows if weight_rows else self.lib.alp_lm_create
        self.ok(create(h, L.as_dp(np.ascontiguousarray(pv)), idx.ctypes.data_as(I32), D, L.as_dp(lo), L.as_dp(hi), L.as_dp(X0), K, loss, 1.0,
                       1e-10, 1e-10, 1e-10, 100 * D, ctypes.byref(loop)))
        pending = ctypes.c_int64()
        t0 = time.perf_counter()
        self.ok(self.lib.alp_lm_run(loop, rounds))
        self.ok(self.lib.alp_lm_wait(loop, ctypes.byref(pending)))
        ms = (time.perf_counter() - t0) * 1e3 / rounds
        x, trial = np.empty((K, D)), np.empty((K, D))
        cost, gn, mu, nu = (np.empty(K) for _ in range(4))
        it, ev = np.empty(K, dtype=np.int64), np.empty(K, dtype=np.int64)
        status = np.empty(K, dtype=np.int32)
        self.ok(self.lib.alp_lm_get(loop, L.as_dp(x), L.as_dp(cost), L.as_dp(gn), it.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                    ev.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), status.ctypes.data_as(I32), L.as_dp(trial), L.as_dp(mu),
                                    L.as_dp(nu)))
        self.ok(self.lib.alp_lm_destroy(loop))
        return ms, np.concatenate([x.ravel(), trial.ravel(), cost, gn, mu, nu, it, ev, status])


def weights_of(n, R, seed):
    """R rows of n weights: integer counts 0..3, uniform fractions, a 0/1 mask, in turn"""
    rng = np.random.default_rng(seed)
    kinds = (lambda: rng.integers(0, 4, n).astype(np.float64), lambda: rng.uniform(0, 3, n), lambda: (rng.uniform(0, 1, n) < 0.7).astype(np.float64))
    return np.array([kinds[r % 3]() for r in range(R)])


def same_bits(outs):
    return all(np.array_equal(outs[0].view(np.uint64), o.view(np.uint64)) for o in outs[1:])


def single_bits(libs, args):
    """the single call, every multi-pose call and a round of the device loop in the three libraries: rows that differ in any bit,
    by case"""
    differ, cases = [], 0
    cols23 = [k for k, name in enumerate(L.PARAM_KEYS) if name not in ("w", "h")]
    for n in (257, 100_003):
        xyz, origin, (u, v), pv, cand, cols = problem(n, TARGETS_D9, 64, 3)
        uv = np.column_stack([u, v])
        w = weights_of(n, 8, 5)
        for precision in (L.ALP_F64, L.ALP_F32):
            handles = [lib.points(xyz, origin, uv, precision) for _, lib in libs]
            X0 = cand[:8][:, cols]

            def case(what, fn):
                nonlocal cases
                cases += 1
                if not same_bits([fn(lib, h) for (_, lib), h in zip(libs, handles)]):
                    differ.append(f"n={n} {'f64' if precision == L.ALP_F64 else 'f32'} {what}")

            for weighted in (False, True):
                if weighted:
                    for (_, lib), h in zip(libs, handles):
                        lib.set_weights(h, w[1])
                for loss in (0, 1, 2, 3):                    # the single call: every loss, D = 9 and all 23 targets
                    for tc in (cols, cols23):
                        case(f"single D={len(tc)} loss={loss} weighted={weighted}", lambda lib, h: lib.normal(h, pv, tc, loss))
                for loss in (0, 2):                          # linear, huber
                    for B in (1, 8, 64):
                        case(f"batch B={B} loss={loss} weighted={weighted}", lambda lib, h: lib.normal(h, cand[:B], cols, loss))
                    case(f"lm round loss={loss} weighted={weighted}", lambda lib, h: lib.lm_rounds(h, pv, cols, X0, 1, loss)[1])
            for (_, lib), h in zip(libs, handles):
                lib.set_weights(h, w)
            for loss in (0, 2):
                for rows in ([3, 3, 0, 7, 1, 1, 5, 3], [7, 6, 5, 4, 3, 2, 1, 0], [2], list(np.random.default_rng(1).integers(0, 8, 64))):
                    case(f"rows {rows[:8]} loss={loss}", lambda lib, h: lib.normal(h, cand[:len(rows)], cols, loss, rows))
                case(f"lm round under weight rows loss={loss}", lambda lib, h: lib.lm_rounds(h, pv, cols, X0, 1, loss, True)[1])
            for (_, lib), h in zip(libs, handles):
                lib.ok(lib.lib.alp_points_destroy(h))
    return dict(step="single", what="bits", libraries=[who for who, _ in libs], cases=cases, cases_with_differing_bits=differ,
                condition="no differing bit", holds=not differ)


def single_times(libs, args):
    """this library's medians inside the spread of the two parent instances, alternated round by round"""
    rows = []

    def compare(what, handles, fn, **info):
        """fn(lib, handle) -> {figure: ms}; per figure the values of every round and library"""
        ms = {}
        for rnd in range(args.rounds + 1):
            for (who, lib), h in zip(libs, handles):
                for fig, t in fn(lib, h).items():
                    if rnd:                                  # round 0 warms the scratch of every shape
                        ms.setdefault(fig, {}).setdefault(who, []).append(round(t, 5))
        for fig, by in ms.items():
            parents = by["parent_a"] + by["parent_b"]
            lo, hi, med = min(parents), max(parents), float(np.median(by["this"]))
            rows.append(dict(step="single", what=what, figure=fig, rounds=args.rounds, ms=by, parent_min_ms=lo, parent_max_ms=hi,
                             this_median_ms=round(med, 5), this_over_parent_median=round(med / float(np.median(parents)), 4),
                             condition="parent_min <= this_median <= parent_max", inside_parent_spread=bool(lo <= med <= hi),
                             above_parent_max=bool(med > hi), **info))

    def call(fn, reps):
        return lambda lib, h: dict(zip(("call_wall_ms", "kernel_ms"), lib.timed(lambda: fn(lib, h), reps)))

    xyz, origin, (u, v), pv, cand, cols = problem(1127, TARGETS_D9, 64, 3)
    handles = [lib.points(xyz, origin, np.column_stack([u, v])) for _, lib in libs]
    compare("alp_normal_equations", handles, call(lambda lib, h: lib.normal(h, pv, cols), 50), points=1127, columns=9)
    compare("alp_normal_equations_batch", handles, call(lambda lib, h: lib.normal(h, cand, cols), 50), points=1127, columns=9, poses=64)
    X0 = cand[:, cols]
    compare("device loop", handles, lambda lib, h: {"wall_ms_per_round": lib.lm_rounds(h, pv, cols, X0, 8)[0]}, points=1127, columns=9,
            starts=64, rounds_per_run=8)
    for (_, lib), h in zip(libs, handles):
        lib.ok(lib.lib.alp_points_destroy(h))

    n = args.points
    xyz, origin, (u, v), pv, cand, cols = problem(n, TARGETS_D21, 8, 3)
    handles = [lib.points(xyz, origin, np.column_stack([u, v])) for _, lib in libs]
    del xyz
    w = weights_of(n, 2, 5)
    for (_, lib), h in zip(libs, handles):
        lib.set_weights(h, w)
    del w
    compare("alp_normal_equations", handles, call(lambda lib, h: lib.normal(h, pv, cols), 5), points=n, columns=21)
    compare("alp_normal_equations_batch", handles, call(lambda lib, h: lib.normal(h, cand, cols), 3), points=n, columns=21, poses=8)
    compare("alp_normal_equations_batch_rows", handles, call(lambda lib, h: lib.normal(h, cand, cols, 0, [0, 1, 1, 0, 0, 1, 0, 1]), 3),
            points=n, columns=21, poses=8)
    for (_, lib), h in zip(libs, handles):
        lib.ok(lib.lib.alp_points_destroy(h))
    return rows


def step_single(args):
    if not args.parent_lib:
        raise SystemExit("the single step needs --parent-lib")
    with tempfile.TemporaryDirectory() as tmp:
        second = os.path.join(tmp, "libalproj_hip_parent_b.so")
        shutil.copy(args.parent_lib, second)
        libs = [("parent_a", RawLib(args.parent_lib)), ("this", RawLib(L.LIB_PATH)), ("parent_b", RawLib(second))]
    return [single_bits(libs, args)] + single_times(libs, args)


def step_solve(args):
    import pandas as pd
    from alproj_amd import optimize as aopt
    g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "g14_lsq.npz"))
    case = "trf_linear_d7"
    keys = [str(k) for k in g["param_keys"]]
    init = dict(zip(keys, g[f"{case}_init"]))
    targets = [str(t) for t in g[f"{case}_targets"]]
    dfx = pd.DataFrame(g["xyz"], columns=["x", "y", "z"])
    dfu = pd.DataFrame(g["uv_" + str(g[f"{case}_uv"])], columns=["u", "v"])
    K = 64

    def fresh():
        o = aopt.LsqOptimizer(dfx, dfu, dict(init))
        o.set_target(targets)
        return o

    o = fresh()
    b = aopt.bounds_to_array(init, targets, None)
    X0 = o._start_matrix(K, 1, b[:, 0], b[:, 1])
    # the time inside the library calls, by wrapping the two bindings
    spent = {"lib": 0.0, "calls": 0}

    def timed(fn):
        def f(*a, **k):
            t0 = time.perf_counter()
            out = fn(*a, **k)
            spent["lib"] += time.perf_counter() - t0
            spent["calls"] += 1
            return out
        return f

    plain_b, plain_s = L.Points.normal_equations_batch, L.Points.normal_equations
    L.Points.normal_equations_batch, L.Points.normal_equations = timed(plain_b), timed(plain_s)
    out = {}
    try:
        fresh().optimize(method="normal", starts=4, seed=1)           # warm-up
        L.kernel_timing(True)
        for name in ("lockstep", "sequential"):
            spent.update(lib=0.0, calls=0)
            L.kernel_time_ms()
            t0 = time.perf_counter()
            if name == "lockstep":
                o = fresh()
                o.optimize(method="normal", starts=X0)
                evals = sum(r[2]["evaluations"] for r in o.start_results)
                best = o.result_["cost"]
            else:
                evals, best = 0, np.inf
                for x0 in X0:
                    s = fresh()
                    s.optimize(method="normal", starts=x0[None, :])
                    evals += s.result_["evaluations"]
                    best = min(best, s.result_["cost"])
            wall = (time.perf_counter() - t0) * 1e3
            k_ms, launches = L.kernel_time_ms()
            out[name] = dict(wall_ms=round(wall, 2), library_calls=spent["calls"], in_library_calls_ms=round(spent["lib"] * 1e3, 2),
                             kernel_ms=round(k_ms, 3), kernel_sections=launches,
                             copies_and_launch_ms=round(spent["lib"] * 1e3 - k_ms, 2), host_solve_and_rest_ms=round(wall - spent["lib"] * 1e3, 2),
                             evaluations=evals, best_cost=best)
        L.kernel_timing(False)
    finally:
        L.Points.normal_equations_batch, L.Points.normal_equations = plain_b, plain_s
    return dict(step="solve", problem=case, points=len(dfx), columns=len(targets), starts=K, **out,
                lockstep_over_sequential=round(out["lockstep"]["wall_ms"] / out["sequential"]["wall_ms"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="small,large,solve")
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 20
    L.init(0)
    rows = []
    for step in args.steps.split(","):
        r = {"small": step_small, "large": step_large, "single": step_single, "solve": step_solve}[step](args)
        for row in (r if isinstance(r, list) else [r]):
            print(json.dumps(row), flush=True)
            rows.append(row)
    if args.out:
        with open(args.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
