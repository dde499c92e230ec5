"""Restatements and helpers of the batched normal-equations path (alp_normal_equations_batch, normal_lm_batch,
LsqOptimizer.optimize(method="normal", starts=...)), shared by tests/test_normal_batch_solver.py (CPU) and
tests/test_gpu_normal_batch.py (GPU).  The oracle, the g14 problems and normal_grid are those of tests/normal_cases.py.

The launch rule of host/alp_plan.h: normal_batch_grid, restated:
    want    = min(cus * WG_PER_CU, MAX_BLOCKS)          the workgroups normal_grid aims at
    stripes = clamp(ceil(want / B), 1, groups)          a pose's share of them, groups = ceil(n / 256)
    per     = ceil(groups / stripes)                    whole groups of 256 points per stripe
    blocks  = ceil(groups / per)                        the stripes that hold a group; the launch is blocks x B workgroups
n = 0 or B < 1: (0, 0), no launch.

The integer rule of optimize(method="normal", starts=K, seed=s): start 0 = the initial target values, starts 1 .. K-1 =
np.random.default_rng(s).uniform(lower, upper, (K - 1, D)), every start clipped into the box."""
import numpy as np

from tests import normal_cases as nc

BATCH_MAX = 1024


def normal_batch_grid(n, B, cus):
    """(stripes per pose, groups of 256 points per stripe) of host/alp_plan.h: normal_batch_grid"""
    groups = -(-n // 256)
    if groups <= 0 or B < 1:
        return 0, 0
    want = min(cus * nc.WG_PER_CU, nc.MAX_BLOCKS)
    stripes = max(1, min(-(-want // B), groups))
    per = -(-groups // stripes)
    return -(-groups // per), per


def integer_starts(x_init, lower, upper, K, seed):
    X0 = np.empty((K, len(x_init)))
    X0[0] = x_init
    X0[1:] = np.random.default_rng(seed).uniform(lower, upper, (K - 1, len(x_init)))
    return np.clip(X0, lower, upper)


def remembered(fun):
    """``fun`` (values -> (G, g, cost)) with its results kept by the bits of ``values``: the lockstep solver and the runs it is
    compared with visit the same points, and the complex-step oracle takes 0.4 s a point.  ``calls`` counts what came new."""
    seen = {}

    def f(values):
        key = np.asarray(values, dtype=np.float64).tobytes()
        if key not in seen:
            seen[key] = fun(values)
            f.calls += 1
        return seen[key]

    f.calls = 0
    return f


def row_by_row(fun, log=None):
    """X (k, D) -> (G (k, D, D), g (k, D), cost (k,)): ``fun`` applied to every row; ``log`` (a list) receives a copy of
    every X"""

    def f(X):
        X = np.asarray(X, dtype=np.float64)
        assert X.ndim == 2 and len(X) >= 1
        if log is not None:
            log.append(X.copy())
        out = [fun(x) for x in X]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.float64)

    return f
