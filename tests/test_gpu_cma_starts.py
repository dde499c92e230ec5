"""Multi-start CMA-ES (alp_cma_create_starts / _set_state_at / _get_state_at, CMAOptimizer.optimize(..., starts=K)): one batched
generation of K starts against K single-start handles, the K-workgroup tell against cma.py, K starts end to end against K
single runs and the handle's refusals (convergence and the world-1 communicator with several starts: tests/test_gpu_cma_device.py)."""
import numpy as np
import pytest

from alproj_amd import _lib as L
from alproj_amd import synthetic as syn
from alproj_amd.optimize import CMAOptimizer, best_start, bounds_to_array
from tests.test_gpu_cma_device import ALLOWED, VARIANT_CASES, _close, _gcp_problem, _h_margin, _host_cma, _random_state

pytestmark = pytest.mark.gpu

SEEDS5 = [11, 12, 99, 1234567, (1 << 40) + 3]


@pytest.fixture(scope="module")
def problem():
    L.init(0)
    return _gcp_problem()


@pytest.fixture(scope="module")
def small_points(problem):
    obj, img, init = problem
    pts = L.Points(obj.to_numpy()[:64], [init["x"], init["y"], init["z"]], "f64")
    pts.set_observed(img.to_numpy()[:64])
    yield pts
    pts.close()


def _order(losses):
    return np.argsort(np.where(np.isnan(losses), np.inf, losses), kind="stable")


def _assert_same_state(a, b):
    for key in ("mean", "C", "p_sigma", "pc", "B", "D"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert a["sigma"] == b["sigma"] and a["g"] == b["g"]


@pytest.mark.parametrize("variant,targets,precision,lens_free_start", VARIANT_CASES)
def test_batched_generation_matches_separate_handles(problem, variant, targets, precision, lens_free_start):
    obj, img, init = problem
    if lens_free_start:
        init = dict(init, **{k: 0.0 for k in syn.TARGETS_D21[9:]})
    opt = CMAOptimizer(obj, img, init)
    opt.set_target(list(targets))
    K, D, P = len(SEEDS5), len(targets), 50
    b = bounds_to_array(init, targets)
    lo, hi = b[:, 0], b[:, 1]
    idx = [L.PARAM_KEYS.index(t) for t in targets]
    m0 = (opt.target_params_init - lo) / (hi - lo)
    rng = np.random.default_rng(5)
    hosts = [_host_cma(D, P, s) for s in SEEDS5]
    states = []
    for k in range(K):
        st = _random_state(rng, D, eigs=rng.uniform(0.2, 1.5, D))
        st.update(mean=np.clip(m0 + rng.normal(0, 0.05, D), 0.05, 0.95), sigma=float(rng.uniform(0.1, 0.25)))
        states.append(st)
    tol = 1e-6 if precision == "f32" else (1e-10 if variant == "general" else 1e-12)
    unit = np.column_stack([np.zeros(D), np.ones(D)])
    with opt._device_points(precision) as pts:
        with L.CmaDevice(pts, L.params_vector(init), idx, lo, hi, hosts[0], seeds=SEEDS5) as loop:
            assert loop.K == K
            before = []
            for k in range(K):
                loop.set_state(states[k], start=k)
            for k in range(K):
                before.append(loop.get_state(eigen=True, start=k))
                assert before[k]["g"] == states[k]["g"]
            loop.run(1, L.LOSS_HUBER, 10.0)
            loop.wait()
            assert pts.eval_population_info()[0] == variant
            X, cand, losses = loop.fetch_last()
            assert X.shape == (K * P, D) and cand.shape == (K * P, L.NPARAM) and losses.shape == (K * P,)
            after = [loop.get_state(eigen=True, start=k) for k in range(K)]
        np.testing.assert_array_equal(cand, opt._candidate_matrix(X * (hi - lo) + lo))
        for k in range(K):
            rows = slice(k * P, (k + 1) * P)
            st = before[k]
            ref = L.cma_sample(st["mean"], st["sigma"], st["B"] * st["D"], unit, P, 100, SEEDS5[k], st["g"])
            np.testing.assert_array_equal(X[rows], ref)
            want, _ = pts.eval_population(cand[rows], L.LOSS_HUBER, 10.0, want_argmin=False)
            assert pts.eval_population_info()[0] == variant
            np.testing.assert_allclose(losses[rows], want, rtol=tol, atol=0)
            with L.CmaDevice(pts, L.params_vector(init), idx, lo, hi, hosts[k]) as single:
                single.set_state(states[k])
                _assert_same_state(single.get_state(eigen=True), st)
                if precision == "f32":
                    # a float32 loss moves by up to ~3e-8 between launch grids, enough to reorder: tell the batched losses
                    single.tell_host(X[rows], losses[rows])
                else:
                    single.run(1, L.LOSS_HUBER, 10.0)
                    single.wait()
                    Xs, cs, ls = single.fetch_last()
                    np.testing.assert_array_equal(Xs, X[rows])
                    np.testing.assert_array_equal(cs, cand[rows])
                    np.testing.assert_array_equal(_order(losses[rows]), _order(ls))
                _assert_same_state(single.get_state(eigen=True), after[k])
            assert after[k]["g"] == states[k]["g"] + 1


@pytest.mark.parametrize("P", [4, 50, 2048])
@pytest.mark.parametrize("D", [1, 9, 21, 25])
def test_batched_tell_parity(small_points, D, P):
    K = 3
    hosts, Xs, ls = [], [], []
    for k in range(K):
        for seed in range(10):                                      # a state not within 1e-9 of the h_sigma threshold
            rng = np.random.default_rng(7000 * D + 31 * P + 100 * k + seed)
            host = _host_cma(D, P, 50 + k)
            host.set_state(_random_state(rng, D))
            host._eigen()
            X = rng.random((P, D))
            losses = np.round(rng.random(P), 2)                     # ties
            perm = rng.permutation(P)
            losses[perm[0]] = np.nan
            if P > 2:
                losses[perm[1]], losses[perm[2]] = np.inf, -np.inf
            probe = _host_cma(D, P, 50 + k)
            probe.set_state(host.get_state())
            probe.tell_population(X, losses)
            if _h_margin(host, probe.get_state()) > 1e-9:
                break
        hosts.append(host)
        Xs.append(X)
        ls.append(losses)
    targets = [ALLOWED[i % len(ALLOWED)] for i in range(D)]
    with L.CmaDevice(small_points, np.zeros(L.NPARAM), targets, np.zeros(D), np.ones(D), hosts[0],
                     seeds=[50 + k for k in range(K)]) as loop:
        for k in range(K):
            loop.set_state(hosts[k].get_state(), start=k)
        order_d = loop.tell_host(np.concatenate(Xs), np.concatenate(ls))
        sds = [loop.get_state(eigen=True, start=k) for k in range(K)]
    for k in range(K):
        host = hosts[k]
        order_h = host.tell_population(Xs[k], ls[k])
        host._eigen()
        np.testing.assert_array_equal(order_d[k * P:(k + 1) * P], order_h)
        sd, sh = sds[k], host.get_state()
        assert sd["g"] == sh["g"]
        for key in ("mean", "p_sigma", "pc"):
            _close(sd[key], sh[key], 1e-13)
        assert abs(sd["sigma"] - sh["sigma"]) <= 1e-13 * sh["sigma"]
        cmax = float(np.max(np.abs(sh["C"])))
        _close(sd["C"], sh["C"], 1e-12, cmax)
        B, d = sd["B"], sd["D"]
        _close((B * d) @ (B * d).T, sd["C"], 1e-12, cmax)
        _close(B.T @ B, np.eye(D), 1e-13, 1.0)
        _close(np.sort(d ** 2), np.linalg.eigh(sh["C"])[0], 1e-12, cmax)


@pytest.mark.parametrize("device_loop", [True, False])
def test_starts_are_single_runs(problem, device_loop):
    obj, img, init = problem
    o = CMAOptimizer(obj, img, init)
    o.set_target(list(syn.TARGETS_D9))
    kw = dict(generation=60, sigma=1.0, population_size=50, f_scale=10.0, progress=False, device_loop=device_loop)
    K = 4
    params, err = o.optimize(seed=7, starts=K, **kw)
    multi = list(o.start_results)
    assert [s for s, _, _ in multi] == [7 + k for k in range(K)]
    for k in range(K):
        p1, e1 = o.optimize(seed=7 + k, **kw)
        assert o.start_results == [(7 + k, p1, e1)]
        assert multi[k][1] == p1, k
        assert abs(multi[k][2] - e1) <= 1e-12 * e1, (k, multi[k][2], e1)
    b = best_start([e for _, _, e in multi])
    assert (params, err) == (multi[b][1], multi[b][2])


def test_multi_start_handle_refusals(problem):
    obj, img, init = problem
    D, P, K = 9, 50, 3
    host = _host_cma(D, P, 1)
    pts = L.Points(obj.to_numpy()[:100], [init["x"], init["y"], init["z"]], "f64")
    pts.set_observed(img.to_numpy()[:100])
    targets = [ALLOWED[i] for i in range(D)]
    loop = L.CmaDevice(pts, L.params_vector(init), targets, np.zeros(D), np.ones(D), host, seeds=[1, 2, 3])
    st = host.get_state()
    for bad in (-1, K):
        with pytest.raises(L.AlprojHipError) as e:
            loop.set_state(st, start=bad)
        assert e.value.code == -1
        with pytest.raises(L.AlprojHipError) as e:
            loop.get_state(start=bad)
        assert e.value.code == -1
    loop.run(2, L.LOSS_HUBER, 10.0)
    with pytest.raises(L.AlprojHipError) as e:
        loop.run(1, L.LOSS_HUBER, 10.0)
    assert e.value.code == -6
    with pytest.raises(L.AlprojHipError) as e:
        loop.get_state(start=1)
    assert e.value.code == -6
    loop.wait()
    assert loop.get_state(start=2)["g"] == 2
    pts.close()
    with pytest.raises(L.AlprojHipError) as e:
        loop.run(1, L.LOSS_HUBER, 10.0)
    assert e.value.code == -6
    loop.close()
    # the ABI's own bounds: K in [1, 1024], K * P <= 65536
    with L.Points(obj.to_numpy()[:100], [init["x"], init["y"], init["z"]], "f64") as p2:
        p2.set_observed(img.to_numpy()[:100])
        for seeds, hp in (([], host), (list(range(1025)), host), (list(range(17)), _host_cma(D, 4096, 1))):
            with pytest.raises(L.AlprojHipError) as e:
                L.CmaDevice(p2, L.params_vector(init), targets, np.zeros(D), np.ones(D), hp, seeds=seeds)
            assert e.value.code == -1
