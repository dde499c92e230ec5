#!/usr/bin/env python3
"""alp_normal_equations_batch (normal_batch_kernel: the normal equations of B poses in one launch) against B single calls, and
the single entry point against the parent commit's.  One process, one JSON line per step:

  small  (a) the GCP size: n = 1127 float64 points, D = 9, B = 64.  One batch call against 64 sequential
             Points.normal_equations calls on the same handle: the median whole-call wall time of --reps repetitions after a
             warm-up.  Condition: batch <= 0.5 x sequential.  The host share of the batch call (the 64 folds, the upload of the
             plans) is reported beside it: wall time less the kernel section.
  large  (b) n = 10 M float64 points, D = 21, B = 8.  The kernel section (alp_kernel_timing) of the batch per pose against the
             single call's, alternated round by round in one process, for BOTH workgroup orders (ALP_NORMAL_BATCH_ORDER =
             stripe | pose: which grid index runs fastest).  Condition, for the order the library ships: the batch's median per
             pose is not above the single call's median by more than the single call's own spread, (max - min) / median.
  single (c) --parent-lib PATH: the parent's library (loaded twice, as tools/probe_mend.py does) and this one in one process,
             alternated, alp_normal_equations at both sizes: the results bit for bit, and this library's median kernel time
             inside the spread of the two parent instances.  normal_kernel's body moved into a device function both kernels
             call; its launch did not change.
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

    def points(self, xyz, origin, uv):
        h = ctypes.c_void_p()
        xyz, uv = np.ascontiguousarray(xyz), np.ascontiguousarray(uv)
        o = np.ascontiguousarray(origin, dtype=np.float64)
        self.ok(self.lib.alp_points_create(xyz.ctypes.data_as(ctypes.c_void_p), L.dtype_code(xyz), len(xyz), L.as_dp(o), L.ALP_F64,
                                           ctypes.byref(h)))
        self.ok(self.lib.alp_points_set_observed(h, uv.ctypes.data_as(ctypes.c_void_p), L.dtype_code(uv)))
        return h

    def normal(self, h, pv, cols, reps):
        """(mean kernel ms of `reps` calls after one more, the sums)"""
        idx = np.ascontiguousarray(cols, dtype=np.int32)
        d = len(idx)
        out = np.empty(d * (d + 1) // 2 + d + 2)
        ms, cnt = ctypes.c_float(), ctypes.c_int()
        self.ok(self.lib.alp_kernel_timing(1))
        self.ok(self.lib.alp_normal_equations(h, L.as_dp(pv), idx.ctypes.data_as(I32), d, 0, 1.0, L.as_dp(out)))
        self.ok(self.lib.alp_kernel_time_ms(ctypes.byref(ms), ctypes.byref(cnt)))
        for _ in range(reps):
            self.ok(self.lib.alp_normal_equations(h, L.as_dp(pv), idx.ctypes.data_as(I32), d, 0, 1.0, L.as_dp(out)))
        self.ok(self.lib.alp_kernel_time_ms(ctypes.byref(ms), ctypes.byref(cnt)))
        self.ok(self.lib.alp_kernel_timing(0))
        return ms.value / reps, out


def step_single(args):
    if not args.parent_lib:
        raise SystemExit("the single step needs --parent-lib")
    with tempfile.TemporaryDirectory() as tmp:
        second = os.path.join(tmp, "libalproj_hip_parent_b.so")
        shutil.copy(args.parent_lib, second)
        libs = [("parent_a", RawLib(args.parent_lib)), ("this", RawLib(L.LIB_PATH)), ("parent_b", RawLib(second))]
    assert [hasattr(lib.lib, "alp_normal_equations_batch") for _, lib in libs] == [False, True, False]
    rows = []
    for n, targets, reps in ((1127, TARGETS_D9, 50), (args.points, TARGETS_D21, 5)):
        xyz, origin, (u, v), pv, _, cols = problem(n, targets, 1, 3)
        uv = np.column_stack([u, v])
        handles = [lib.points(xyz, origin, uv) for _, lib in libs]
        ms = {who: [] for who, _ in libs}
        same, first = True, None
        for rnd in range(args.rounds + 1):
            for (who, lib), h in zip(libs, handles):
                t, out = lib.normal(h, pv, cols, reps)
                if rnd:
                    ms[who].append(round(t, 5))
                first = out if first is None else first
                same = same and np.array_equal(first, out, equal_nan=True)
        for (_, lib), h in zip(libs, handles):
            lib.ok(lib.lib.alp_points_destroy(h))
        parents = ms["parent_a"] + ms["parent_b"]
        lo, hi = min(parents), max(parents)
        med = float(np.median(ms["this"]))
        rows.append(dict(step="single", points=n, columns=len(cols), calls_per_round=reps, rounds=args.rounds, kernel_ms=ms,
                         parent_min_ms=lo, parent_max_ms=hi, this_median_ms=round(med, 5),
                         this_over_parent_median=round(med / float(np.median(parents)), 4), inside_parent_spread=bool(lo <= med <= hi),
                         above_parent_max=bool(med > hi), sums_bit_equal=bool(same)))
    return rows


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
