"""CMAOptimizer.optimize(..., starts=K) on the host: its refusals (before any device call), the seed rule, the best-start rule,
and the host multi-start against K single runs -- in one process and over gloo in world 2 and 3
(tests/_dist_cma_worker.py), the oracle standing in for the device's population evaluation."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

from alproj_amd import _lib
from alproj_amd import optimize as aopt
from alproj_amd import synthetic as syn
from oracle import ref_numpy as orc

HERE = os.path.dirname(os.path.abspath(__file__))


def _problem():
    truth = syn.truth_params(316)
    init = dict(truth, pan=truth["pan"] + 1.5, tilt=truth["tilt"] - 1.0, fov=truth["fov"] + 2, x=truth["x"] + 3)
    n = 1201
    xyz = syn.gcp_points(n, truth, seed=11)
    uv = orc.project_points(xyz, truth) + np.random.default_rng(11).normal(0, 0.8, (n, 2))
    return xyz, uv, init


class OraclePoints:
    """what alproj_amd._lib.Points is to CMAOptimizer, on the host: every candidate's loss from the oracle"""
    precision = _lib.ALP_F64

    def __init__(self, xyz, uv, log):
        self.xyz, self.uv, self.n, self.log = xyz, uv, len(xyz), log

    def eval_population(self, cand, kind, f_scale, want_argmin=True):
        losses = np.empty(len(cand))
        for i, c in enumerate(cand):
            proj = orc.project_points(self.xyz, orc.vector_to_params(c))
            losses[i] = orc.mean_distance(self.uv, proj) if kind == _lib.LOSS_MEAN_DIST else orc.huber(self.uv, proj, f_scale)
        self.log.append(("eval", len(cand), want_argmin))
        ok = ~np.isnan(losses)
        return losses, (int(np.flatnonzero(ok)[np.argmin(losses[ok])]) if ok.any() else 0)

    def close(self):
        pass


@pytest.fixture
def oracle_device(monkeypatch):
    """the optimiser on the oracle, world 1, with no device call possible"""
    xyz, uv, init = _problem()
    log = []
    monkeypatch.setattr(aopt.BaseOptimizer, "_device_points", lambda self, precision=None: OraclePoints(xyz, uv, log))
    monkeypatch.setattr(_lib, "comm_info", lambda: (0, 1))
    return pd.DataFrame(xyz, columns=["x", "y", "z"]), pd.DataFrame(uv, columns=["u", "v"]), init, log


@pytest.fixture
def no_device(monkeypatch):
    """any device call fails the test"""
    def touched(*a, **k):
        raise AssertionError("the device was touched before the refusal")
    monkeypatch.setattr(aopt.BaseOptimizer, "_device_points", touched)
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(_lib, "comm_info", touched)
    monkeypatch.setattr(_lib, "CmaDevice", touched)
    xyz, uv, init = _problem()
    o = aopt.CMAOptimizer(pd.DataFrame(xyz[:8], columns=["x", "y", "z"]), pd.DataFrame(uv[:8], columns=["u", "v"]), init)
    o.set_target(list(syn.TARGETS_D9))
    return o


KW = dict(sigma=1.0, f_scale=10.0, seed=1, progress=False)


@pytest.mark.parametrize("starts,population_size", [(0, 50), (-1, 50), (1025, 10), (2, 32769), (1024, 65), (64, 1025)])
def test_starts_refusals(no_device, starts, population_size):
    for device_loop in (False, True):
        with pytest.raises(ValueError):
            no_device.optimize(generation=10, population_size=population_size, starts=starts, device_loop=device_loop, **KW)


def test_starts_limits_are_inclusive(no_device):
    """1024 starts, and K * P = 65536, pass the checks: the refusal comes from the first device call"""
    for starts, pop in ((1024, 64), (16, 4096)):
        with pytest.raises(AssertionError, match="touched"):
            no_device.optimize(generation=10, population_size=pop, starts=starts, **KW)


def test_starts_with_each_device_loop_refusal(no_device):
    o = no_device
    kw = dict(KW, starts=2, device_loop=True)
    with pytest.raises(ValueError):
        o.optimize(generation=10, population_size=4097, **kw)
    with pytest.raises(ValueError):
        o.optimize(generation=0, population_size=50, **kw)
    targets = o.target_params
    o.set_target(list(targets) + ["w"])
    with pytest.raises(ValueError):
        o.optimize(generation=10, population_size=50, **kw)
    o.set_target(list(targets) + ["h"])
    with pytest.raises(ValueError):
        o.optimize(generation=10, population_size=50, **kw)
    allowed = [k for k in _lib.PARAM_KEYS if k not in ("w", "h")]
    o.set_target([allowed[i % len(allowed)] for i in range(33)])
    with pytest.raises(ValueError):
        o.optimize(generation=10, population_size=50, **kw)


def test_start_seeds():
    assert aopt.start_seeds(7, 4) == [7, 8, 9, 10]
    assert aopt.start_seeds(7, 1) == [7]
    top = (1 << 63) - 2
    assert aopt.start_seeds(top, 4) == [top, top + 1, 0, 1]
    drawn = aopt.start_seeds(None, 16)
    assert len(set(drawn)) == 16 and all(0 <= s < (1 << 63) for s in drawn)
    assert [s - drawn[0] for s in drawn] == list(range(16)) or 0 in drawn          # consecutive, unless it wrapped
    assert aopt.start_seeds(None, 4) != aopt.start_seeds(None, 4)


def test_best_start():
    nan, inf = np.nan, np.inf
    assert aopt.best_start([3.0, 1.0, 2.0]) == 1
    assert aopt.best_start([2.0, 1.0, 1.0, 5.0]) == 1                    # ties: the lowest start
    assert aopt.best_start([nan, 4.0, nan, 4.0]) == 1                    # NaN never wins
    assert aopt.best_start([nan, inf]) == 1
    assert aopt.best_start([nan, nan, nan]) == 0                         # all NaN: start 0
    assert aopt.best_start([5.0]) == 0


def test_host_multi_start_is_k_single_runs(oracle_device):
    obj, img, init, log = oracle_device
    o = aopt.CMAOptimizer(obj, img, init)
    o.set_target(list(syn.TARGETS_D9))
    kw = dict(generation=12, sigma=1.0, population_size=10, f_scale=10.0, progress=False)
    params, err = o.optimize(seed=41, starts=3, **kw)
    multi = list(o.start_results)
    # one evaluation of all 30 candidates per generation, each start's own on the last one (with its argmin), then the errors
    assert log == [("eval", 30, False)] * 11 + [("eval", 10, True)] * 3 + [("eval", 1, True)] * 3
    assert [s for s, _, _ in multi] == [41, 42, 43]
    for k in range(3):
        del log[:]
        p1, e1 = o.optimize(seed=41 + k, **kw)
        # a single run: one evaluation per generation, the argmin asked for only on the last, then the final error
        assert log == [("eval", 10, False)] * 11 + [("eval", 10, True)] + [("eval", 1, True)]
        assert o.start_results == [(41 + k, p1, e1)]
        assert multi[k][1] == p1 and multi[k][2] == e1
    b = aopt.best_start([e for _, _, e in multi])
    assert (params, err) == (multi[b][1], multi[b][2])
    assert err == min(e for _, _, e in multi)


@pytest.mark.parametrize("starts", [1, 4])
def test_host_multi_start_without_seed(oracle_device, starts):
    obj, img, init, _ = oracle_device
    o = aopt.CMAOptimizer(obj, img, init)
    o.set_target(["fov", "pan", "tilt"])
    params, err = o.optimize(generation=3, sigma=0.3, population_size=6, progress=False, starts=starts)
    seeds = [s for s, _, _ in o.start_results]
    assert len(o.start_results) == starts and len(set(seeds)) == starts
    assert all(isinstance(s, int) and 0 <= s < (1 << 63) for s in seeds)             # the drawn base seed, also for one start
    assert all((b - seeds[0]) % (1 << 63) == k for k, b in enumerate(seeds))
    assert (params, err) == o.start_results[aopt.best_start([e for _, _, e in o.start_results])][1:]


def _single_process_starts(seed, starts):
    xyz, uv, init = _problem()
    log = []
    saved = aopt.BaseOptimizer._device_points, _lib.comm_info
    aopt.BaseOptimizer._device_points = lambda self, precision=None: OraclePoints(xyz, uv, log)
    _lib.comm_info = lambda: (0, 1)
    try:
        o = aopt.CMAOptimizer(pd.DataFrame(xyz, columns=["x", "y", "z"]), pd.DataFrame(uv, columns=["u", "v"]), init)
        o.set_target(syn.TARGETS_D9)
        res = o.optimize(generation=15, sigma=0.3, population_size=12, f_scale=10.0, seed=seed, progress=False, starts=starts)
        return res, o.start_results
    finally:
        aopt.BaseOptimizer._device_points, _lib.comm_info = saved


@pytest.mark.parametrize("world", [2, 3])
def test_host_multi_start_over_gloo(tmp_path, world):
    """Nobody passes a seed: rank 0's base seed and every generation's 3 x 12 candidates must reach every rank, so that all
    ranks end with the same (params, error, start_results) -- the single-process run's from the same base seed."""
    from tests.test_dist_gloo import _free_port
    port = _free_port()
    outs = [str(tmp_path / f"s{r}.npz") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "_dist_cma_worker.py"), str(r), str(world), port, outs[r], "starts"],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    for p in procs:
        out, _ = p.communicate(timeout=900)
        assert p.returncode == 0, out.decode()[-3000:]
    res = [np.load(o) for o in outs]
    for r in res[1:]:
        for key in ("params", "seeds", "start_params", "start_errors"):
            np.testing.assert_array_equal(r[key], res[0][key])
        assert float(r["err"]) == float(res[0]["err"])
    expect = (["('bcast', 'uint64', (2,))"] + ["('bcast', 'float64', (36, 9))", "('eval', 36)"] * 14 + ["('bcast', 'float64', (36, 9))"]
              + ["('eval', 12)"] * 3 + ["('eval', 1)"] * 3)
    for r in res:
        assert list(r["log"]) == expect
    seeds = [int(s) for s in res[0]["seeds"]]
    assert seeds == [(seeds[0] + k) % (1 << 63) for k in range(3)]
    (params, err), single = _single_process_starts(seeds[0], 3)
    assert [s for s, _, _ in single] == seeds
    for k, (_, p, e) in enumerate(single):
        np.testing.assert_array_equal(res[0]["start_params"][k], [p[key] for key in syn.TARGETS_D9])
        assert abs(float(res[0]["start_errors"][k]) - e) <= 1e-12 * e
    np.testing.assert_array_equal(res[0]["params"], [params[key] for key in syn.TARGETS_D9])
    assert abs(float(res[0]["err"]) - err) <= 1e-12 * err
