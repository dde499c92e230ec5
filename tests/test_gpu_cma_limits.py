"""The CMA-ES device loop at its limits.
(A) Every draw of alp_cma_sample and of the device loop against the numpy restatement of tests/cma_cases.py: the try index
    exactly, x to a few ulp, at the dmax boundaries, around the 64-try ballot window, for seeds and generations past 2^32 and
    for K starts.
(B) The tell and the warm-started eigendecomposition along trajectories against cma.py re-synchronised every generation, every
    eigenvalue held to mpmath, and the tell at K = 1024 and P = 4096.
(C) The batched population launch of K starts: its grid, every point counted once on it, its losses against per-start launches
    and the float64 oracle, and candidate buffers regrown under a live handle.
The tests print what they measured; each bound states the measured value it was set from and its margin."""
import mpmath
import numpy as np
import pytest

from alproj_amd import _lib as L
from alproj_amd import synthetic as syn
from alproj_amd.optimize import CMAOptimizer, bounds_to_array
from oracle import ref_numpy as orc
from tests import cma_cases as cc
from tests import popeval_cases as pc
from tests.test_gpu_cma_device import ALLOWED, TARGETS_D12, _close, _gcp_problem, _h_margin, _host_cma, _random_state
from tests.test_gpu_points import f32_loss_tolerance
from tests.test_gpu_popeval_grid import CROSS_GRID_RTOL, F32_STORED_INPUT_RTOL, F64_RTOL

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def problem():
    L.init(0)
    return _gcp_problem()


@pytest.fixture(scope="module")
def small_points(problem):
    obj, img, init = problem
    pts = L.Points(obj.to_numpy()[:64], [init["x"], init["y"], init["z"]], "f64")
    pts.set_observed(img.to_numpy()[:64])
    yield pts, L.params_vector(init)
    pts.close()


# ================================================================== A. the draw
DRAW_DIMS = (1, 2, 3, 12, 13, 24, 25, 31, 32)
N_MAX = (0, 1, 63, 64, 65, 128)
# x against the restatement, in units of eps (|mean| + sigma |BD| |z|) per coordinate: ocml's log / sin / cos against libm's and
# the fma chain of make_x against numpy's products
DRAW_ULPS = 8.0                              # measured 1.75 at most (D 24, unbounded)


def _draw_case(D, box):
    rng = np.random.default_rng(100 + D)
    a = rng.normal(size=(D, D))
    d2, b = np.linalg.eigh(a @ a.T / D + 0.1 * np.eye(D))
    BD = b * np.sqrt(d2)
    mean, sigma = rng.uniform(-1, 1, D), 0.7
    seed = (D << 32) + 977 * D + 5                  # both words of the key set
    if box == "unbounded":
        return mean, sigma, BD, None, seed
    std = sigma * np.sqrt((BD ** 2).sum(1))
    if box == "moderate":                           # ~3 % of the tries inside: accepted tries spread past the 64-lane window
        z = cc.normals(D, np.arange(4)[None, :], np.arange(2000)[:, None], 0, seed + 1).reshape(-1, D)
        c = np.quantile(np.abs(sigma * (z @ BD.T) / std).max(axis=1), 0.03)
    else:                                           # hopeless: almost every candidate ends clipped
        c = 1e-3
    return mean, sigma, BD, np.column_stack([mean - c * std, mean + c * std]), seed


def _ulps(x, xr, scale):
    return np.abs(x - xr) / (EPS * scale)


@pytest.mark.parametrize("box", ["unbounded", "moderate", "hopeless"])
@pytest.mark.parametrize("D", DRAW_DIMS)
def test_sampler_draws_match_the_restatement(problem, D, box):
    mean, sigma, BD, bounds, seed = _draw_case(D, box)
    P = 300
    gen = (1 << 32) + 3 * D                          # the kernel takes the generation modulo 2^32
    worst, near, total = 0.0, 0, 0
    tries = {}
    for n_max in (N_MAX if bounds is not None else (0, 100)):
        x, t = L.cma_sample(mean, sigma, BD, bounds, P, n_max, seed, gen, return_tries=True)
        xr, tr, sc, nf = cc.sample(mean, sigma, BD, bounds, P, n_max, seed, gen)
        keep = ~nf
        near += int(nf.sum())
        total += P
        np.testing.assert_array_equal(t[keep], tr[keep], err_msg=f"n_max {n_max}")
        worst = max(worst, float(_ulps(x[keep], xr[keep], sc[keep]).max(initial=0.0)))
        if bounds is not None:
            assert ((x >= bounds[:, 0]) & (x <= bounds[:, 1])).all()
        tries[n_max] = tr
    np.testing.assert_array_equal(L.cma_sample(mean, sigma, BD, bounds, P, 65, seed, gen & 0xFFFFFFFF),
                                  L.cma_sample(mean, sigma, BD, bounds, P, 65, seed, gen))
    print(f"[cma draw] D {D} {box}: max {worst:.2f} eps-units; {near} of {total} candidates decided within {cc.NEAR_FACE} "
          f"of a face" + (f"; tries at n_max 128: <64 {int((tries[128] < 64).sum())}, 64..127 "
                          f"{int(((tries[128] >= 64) & (tries[128] < 128)).sum())}, clipped {int((tries[128] == 128).sum())}"
                          if bounds is not None else ""))
    assert worst <= DRAW_ULPS
    assert near <= max(1, total // 1000)
    if box == "unbounded":
        assert all((t == 0).all() for t in tries.values())
    elif box == "moderate":
        assert (tries[128] < 64).any() and (tries[128] >= 64).any()
    else:
        assert (tries[128] == 128).mean() > 0.5 and (tries[0] == 0).all()


def _loop_draw_deviation(X, befores, seeds, P, n_max):
    """(max eps-units, near-face count) of fetch_last's X of K starts against each start's restated draw"""
    D = X.shape[1]
    unit = np.column_stack([np.zeros(D), np.ones(D)])
    worst, near = 0.0, 0
    for k, st in enumerate(befores):
        xr, _, sc, nf = cc.sample(st["mean"], st["sigma"], st["B"] * st["D"], unit, P, n_max, seeds[k], st["g"])
        rows = X[k * P:(k + 1) * P]
        near += int(nf.sum())
        worst = max(worst, float(_ulps(rows[~nf], xr[~nf], sc[~nf]).max(initial=0.0)))
    return worst, near


# ================================================================== B. the tell
def _mp_eigvalsh(C, dps=40):
    with mpmath.workdps(dps):
        E = mpmath.eigsy(mpmath.matrix(C.tolist()), eigvals_only=True)
        return np.sort(np.array([float(e) for e in E]))


# Bounds of the trajectories, relative (mean, p_sigma, pc: to max(1, max |host|); sigma: to sigma; C and B D^2 B^T: to max|C|):
# FLOOR + ALPHA eps cond(C) per generation.  The negative weights' w_io and p_sigma go through C^-1/2 on both sides, so neither
# is exact there: on the ellipsoid (condition up to 2.2e10) the MI355X measured p_sigma 3.1e-8, sigma 2.6e-9, C 4.0e-9 against
# cma.py, 0.55 - 6.5 eps cond at most; on the GCP problem (condition 2.6e5) 7.5e-13, 2.4e-14 and 1.1e-14.  ALPHA is about ten
# times the measured eps-cond multiple; the floors are test_tell_parity's.
TRAJ_FLOOR = {"mean": 1e-13, "p_sigma": 1e-13, "pc": 1e-13, "sigma": 1e-13, "C": 1e-12, "B D2 B^T - C": 1e-12}
TRAJ_ALPHA = {"mean": 0.0, "p_sigma": 64.0, "pc": 0.0, "sigma": 8.0, "C": 8.0, "B D2 B^T - C": 8.0}
# ||B^T B - I||max: 4.9e-15 (ellipsoid) and 6.9e-15 (GCP) measured after 300 and 200 warm-started generations
ORTH_TOL = 2e-14
# every d^2 against mpmath's eigenvalue of cma.py's symmetrised C: EIG_D_EPS D eps lambda_max (measured 1.8 on the GCP problem)
# plus D max|dC|, Weyl's bound for the device decomposing its own C, which is within that (2-norm) of cma.py's
EIG_D_EPS = 8.0


class TellGauge:
    """the device's tell + eigen against cma.py's, generation after generation: the largest deviation of each quantity (raw,
    in units of eps cond(C), and as a fraction of its bound)"""

    def __init__(self):
        self.raw, self.per_cond, self.frac = {}, {}, {}
        self.cond = 0.0
        self.eig_checks = 0

    def put(self, key, err, tol, cond=None):
        self.raw[key] = max(self.raw.get(key, 0.0), float(err))
        self.frac[key] = max(self.frac.get(key, 0.0), float(err) / tol)
        if cond is not None:
            self.per_cond[key] = max(self.per_cond.get(key, 0.0), float(err) / (EPS * cond))

    def compare(self, sd, sh, d_host, C_pre, mp=False):
        D = len(sh["mean"])
        cond = float((d_host.max() / d_host.min()) ** 2)
        self.cond = max(self.cond, cond)

        def bound(key):
            return TRAJ_FLOOR[key] + TRAJ_ALPHA[key] * EPS * cond

        for key in ("mean", "p_sigma", "pc"):
            self.put(key, np.max(np.abs(sd[key] - sh[key])) / max(1.0, float(np.max(np.abs(sh[key])))), bound(key), cond)
        self.put("sigma", abs(sd["sigma"] - sh["sigma"]) / sh["sigma"], bound("sigma"), cond)
        cmax = float(np.max(np.abs(sh["C"])))
        dC = float(np.max(np.abs(sd["C"] - sh["C"])))
        self.put("C", dC / cmax, bound("C"), cond)
        B, d = sd["B"], sd["D"]
        self.put("B^T B - I", np.max(np.abs(B.T @ B - np.eye(D))), ORTH_TOL)
        self.put("B D2 B^T - C", np.max(np.abs((B * d ** 2) @ B.T - C_pre)) / cmax, bound("B D2 B^T - C"), cond)
        if mp:
            lam = _mp_eigvalsh(C_pre)
            lmax = float(np.max(np.abs(lam)))
            tol = EIG_D_EPS * D * EPS * lmax + D * dC
            order = np.argsort(d ** 2)
            neg, pos = lam < -tol, lam > tol
            assert np.all(d[order][neg] == np.sqrt(1e-8)), "a negative eigenvalue not clamped"
            self.put("d^2 - eig", np.max(np.abs(d[order][pos] ** 2 - lam[pos]), initial=0.0) / (D * EPS * lmax), tol / (D * EPS * lmax))
            self.eig_checks += 1

    def report(self, label):
        print(f"[cma tell] {label}: max condition {self.cond:.3e}, {self.eig_checks} mpmath checks; max "
              + ", ".join(f"{k} {v:.3e}" for k, v in self.raw.items()) + "; in eps cond: "
              + ", ".join(f"{k} {v:.3g}" for k, v in self.per_cond.items()) + "; of the bound: "
              + ", ".join(f"{k} {v:.3g}" for k, v in self.frac.items()))


def _check_gauge(g, label, min_cond):
    g.report(label)
    bad = {k: v for k, v in g.frac.items() if v > 1.0}
    assert not bad, (label, bad)
    assert g.cond >= min_cond, (label, g.cond)
    assert g.eig_checks >= 4


def _sym(C):
    return (C + C.T) / 2


def test_tell_trajectory_ill_conditioned(small_points):
    """300 tells on a rotated ellipsoid of condition 1e10, from three states: C near the inverse Hessian (condition 1e10),
    repeated eigenvalues, a cluster 1e-12 wide.  Every generation cma.py takes the device's state and both tell the same X and
    losses; the device keeps its own warm-started B throughout."""
    pts, tmpl = small_points
    D, P, K, G = 13, 16, 3, 300
    rng = np.random.default_rng(2024)
    R = np.linalg.qr(rng.normal(size=(D, D)))[0]
    h = 1e10 ** (np.arange(D) / (D - 1))
    xs = rng.uniform(0.3, 0.7, D)

    def f(X):
        return ((((X - xs) @ R) ** 2) * h).sum(1)

    Rp = np.linalg.qr(R + 1e-3 * rng.normal(size=(D, D)))[0]
    Q = np.linalg.qr(rng.normal(size=(D, D)))[0]
    eigs = [1.0 / h, np.array([0.5] * 5 + [1.0] * 4 + [2.0] * 4), np.concatenate([1 + 1e-12 * np.arange(6), np.logspace(-3, 0.5, 7)])]
    frames = [Rp, Q, Q]
    hosts = [_host_cma(D, P, 40 + k) for k in range(K)]
    gauge = TellGauge()
    with L.CmaDevice(pts, tmpl, [ALLOWED[i] for i in range(D)], np.zeros(D), np.ones(D), hosts[0], seeds=[40, 41, 42]) as loop:
        for k in range(K):
            C = (frames[k] * eigs[k]) @ frames[k].T
            loop.set_state({"mean": xs + 0.05 * rng.normal(size=D), "sigma": 0.1, "C": _sym(C), "p_sigma": np.zeros(D),
                            "pc": np.zeros(D), "g": 0}, start=k)
        sts = [loop.get_state(eigen=True, start=k) for k in range(K)]
        for g in range(G):
            Xs = [st["mean"] + st["sigma"] * (rng.normal(size=(P, D)) @ (st["B"] * st["D"]).T) for st in sts]
            ls = [f(X) for X in Xs]
            order_d = loop.tell_host(np.concatenate(Xs), np.concatenate(ls))
            for k in range(K):
                host = hosts[k]
                host.set_state(sts[k])
                order_h = host.tell_population(Xs[k], ls[k])
                np.testing.assert_array_equal(order_d[k * P:(k + 1) * P], order_h, err_msg=f"generation {g}, start {k}")
                C_pre = _sym(host._C)
                host._eigen()
                sts[k] = loop.get_state(eigen=True, start=k)
                gauge.compare(sts[k], host.get_state(), host._D, C_pre, mp=g % 50 == 0 or g == G - 1)
    _check_gauge(gauge, "ellipsoid 1e10, D 13, 300 generations", 1e10)     # measured 2.2e10


def test_run_trajectory_gcp_d21(problem):
    """about 200 generations of run(1) on the D = 21 GCP problem in float64: each generation's draw against the restatement,
    its tell against cma.py's on the device's losses"""
    obj, img, init = problem
    targets = syn.TARGETS_D21
    opt = CMAOptimizer(obj, img, init)
    opt.set_target(list(targets))
    D, P, G = len(targets), 50, 200
    b = bounds_to_array(init, targets)
    lo, hi = b[:, 0], b[:, 1]
    host = _host_cma(D, P, 17)
    host.set_state(dict(host.get_state(), mean=(opt.target_params_init - lo) / (hi - lo), sigma=0.3))
    gauge = TellGauge()
    draw_worst, draw_near = 0.0, 0
    with opt._device_points("f64") as pts:
        with L.CmaDevice(pts, L.params_vector(init), [L.PARAM_KEYS.index(t) for t in targets], lo, hi, host) as loop:
            loop.set_state(host.get_state())
            st = loop.get_state(eigen=True)
            for g in range(G):
                host.set_state(st)
                loop.run(1, L.LOSS_HUBER, 10.0)
                loop.wait()
                X, _, losses = loop.fetch_last()
                w, n = _loop_draw_deviation(X, [st], [17], P, 100)
                draw_worst, draw_near = max(draw_worst, w), draw_near + n
                host.tell_population(X, losses)
                C_pre = _sym(host._C)
                host._eigen()
                st = loop.get_state(eigen=True)
                gauge.compare(st, host.get_state(), host._D, C_pre, mp=g % 50 == 49 or g == 0)
    print(f"[cma draw] run(1) D 21, {G} generations: max {draw_worst:.2f} eps-units, {draw_near} near a face")
    assert draw_worst <= DRAW_ULPS and draw_near <= max(1, G * P // 1000)
    _check_gauge(gauge, "GCP D 21 run(1), 200 generations", 1e5)           # measured 2.6e5


@pytest.mark.parametrize("K,P,D", [(1024, 64, 9), (16, 4096, 21)])
def test_many_starts_tell_and_draw(small_points, K, P, D):
    """K = 1024 workgroups and P = CMA_MAX_P: per-start tell parity for every start (generations around 2^32), then one
    device generation whose draws are held to the restatement"""
    pts, tmpl = small_points
    rng = np.random.default_rng(K + P + D)
    seeds = [(k << 32) + 7 * k + 1 for k in range(K)]
    hosts, Xs, ls, states = [], [], [], []
    for k in range(K):
        while True:                                                 # a state not within 1e-9 of the h_sigma threshold
            st = _random_state(rng, D)
            st["g"] = (1 << 32) - 2 + k % 3
            X = rng.random((P, D))
            losses = np.round(rng.random(P), 2)                     # ties
            perm = rng.permutation(P)
            losses[perm[0]], losses[perm[1]], losses[perm[2]] = np.nan, np.inf, -np.inf
            probe = _host_cma(D, P, seeds[k])
            probe.set_state(st)
            probe.tell_population(X, losses)
            if _h_margin(probe, probe.get_state()) > 1e-9:
                break
        host = _host_cma(D, P, seeds[k])
        host.set_state(st)
        host._eigen()
        hosts.append(host)
        states.append(st)
        Xs.append(X)
        ls.append(losses)
    with L.CmaDevice(pts, tmpl, [ALLOWED[i] for i in range(D)], np.zeros(D), np.ones(D), hosts[0], seeds=seeds) as loop:
        assert loop.K == K
        for k in range(K):
            loop.set_state(states[k], start=k)
        order_d = loop.tell_host(np.concatenate(Xs), np.concatenate(ls))
        sds = [loop.get_state(eigen=True, start=k) for k in range(K)]
        loop.run(1, L.LOSS_HUBER, 10.0)
        loop.wait()
        X, _, _ = loop.fetch_last()
        assert pts.eval_population_info()[1:] == cc.batched_grid(pts.n, K * P, "f64", False, L.device_info()["cu_count"])
    for k in range(K):
        host = hosts[k]
        order_h = host.tell_population(Xs[k], ls[k])
        host._eigen()
        np.testing.assert_array_equal(order_d[k * P:(k + 1) * P], order_h, err_msg=f"start {k}")
        sd, sh = sds[k], host.get_state()
        assert sd["g"] == sh["g"]
        for key in ("mean", "p_sigma", "pc"):
            _close(sd[key], sh[key], 1e-13)
        # sigma *= exp(a) with a = c_sigma / d_sigma (|p_sigma| / chi_n - 1): the error of |p_sigma| is amplified by
        # c_sigma / d_sigma |p_sigma| / chi_n (up to 7.7 among these random states, one of which measured 1.7e-13)
        amp = max(1.0, host._c_sigma / host._d_sigma * np.linalg.norm(sh["p_sigma"]) / host._chi_n)
        assert abs(sd["sigma"] - sh["sigma"]) <= 1e-13 * amp * sh["sigma"], (k, sd["sigma"], sh["sigma"], amp)
        cmax = float(np.max(np.abs(sh["C"])))
        _close(sd["C"], sh["C"], 1e-12, cmax)
        B, d = sd["B"], sd["D"]
        _close(B.T @ B, np.eye(D), 1e-13, 1.0)
        _close(np.sort(d ** 2), np.linalg.eigh(sh["C"])[0], 1e-12, cmax)
    worst, near = _loop_draw_deviation(X, sds, seeds, P, hosts[0]._n_max_resampling)
    print(f"[cma draw] K {K} x P {P}, D {D}: max {worst:.2f} eps-units, {near} of {K * P} near a face")
    assert worst <= DRAW_ULPS and near <= max(1, K * P // 1000)


# ================================================================== C. the batched population launch
VARIANT_TARGETS = {"general": syn.TARGETS_D21, "lens_free": syn.TARGETS_D9, "shared_pose": TARGETS_D12}


def _check_batched_grid(pts, R, prec, variant):
    v, s, c = pts.eval_population_info()
    assert v == variant
    assert s * R * 8 <= cc.BATCHED_PARTIALS_BYTES, (s, R)
    assert (s, c) == cc.batched_grid(pts.n, R, prec, variant == "lens_free", L.device_info()["cu_count"]), (s, c)
    return s, c


def _starts_loop(pts, variant, K, P, sigma, rng, exact=False):
    """a device loop of K starts of one kernel variant around the truth; exact: lower == upper == the truth for every target,
    so that every candidate of every start is exactly the truth (x * 0 + lo = lo)"""
    t = pc.truth(variant)
    targets = VARIANT_TARGETS[variant]
    idx = [L.PARAM_KEYS.index(k) for k in targets]
    v = L.params_vector(t)
    if exact:
        lo = hi = v[idx]
    else:
        b = orc.bounds_to_array(t, targets)
        lo, hi = b[:, 0], b[:, 1]
    D = len(idx)
    host = _host_cma(D, P, 1)
    loop = L.CmaDevice(pts, v, idx, lo, hi, host, seeds=[1000 + k for k in range(K)])
    m0 = 0.5 if exact else (v[idx] - lo) / (hi - lo)
    for k in range(K):
        st = _random_state(rng, D, eigs=rng.uniform(0.2, 1.5, D))
        st.update(mean=np.clip(m0 + rng.normal(0, 0.01, D), 0.05, 0.95), sigma=sigma)
        loop.set_state(st, start=k)
    return loop


def _large_set(n, prec, variant, seed):
    """n GCP-like points whose observations are the device's own projection of the truth"""
    t = pc.truth(variant)
    xyz = syn.gcp_points(n, pc.truth("general"), seed=seed)
    pts = L.Points(xyz, pc.origin(), prec)
    pts.project(L.params_vector(t))
    u, v = pts.fetch()
    return pts, np.column_stack([u, v])


COVERAGE_CASES = [("ragged67", "f64", "general", 16, 256), ("ragged67", "f64", "shared_pose", 16, 256),
                  ("ragged67", "f64", "lens_free", 16, 256), ("ragged67", "f32", "lens_free", 16, 256),
                  ("million", "f32", "general", 16, 4096)]


@pytest.mark.parametrize("where,prec,variant,K,P", COVERAGE_CASES)
def test_batched_grid_counts_every_point_once(problem, where, prec, variant, K, P):
    """the marked-point probe of tests/test_gpu_popeval_grid.py on the grid the batched launch reports: every candidate of every
    start is the truth, marked points are off by unit * 4^k pixels, and loss * n spells out how often each was counted"""
    rng = np.random.default_rng(5)
    if where == "ragged67":
        xyz = pc.point_set()[0]
        pts = L.Points(xyz, pc.origin(), prec)
        exact = orc.project_points(xyz, pc.truth(variant))
    else:
        pts, exact = _large_set(1_000_000, prec, variant, 21)
    n = pts.n
    per_call, unit = (10, 1.0) if prec == "f64" else (6, 2.0 ** 14)
    try:
        pts.set_observed(exact)
        with _starts_loop(pts, variant, K, P, 0.2, rng, exact=True) as loop:
            loop.run(1, L.LOSS_MEAN_DIST, 0.0)
            loop.wait()
            s, c = _check_batched_grid(pts, K * P, prec, variant)
            marks = pc.mark_positions(s, cc.GROUP_V[(prec, variant == "lens_free")], n)
            if where == "million":                 # the first two, a middle and the last two non-empty stripes
                keep = [b for i, b in enumerate(pc.stripe_bounds(s, n)) if i in (0, 1, s // 2) or b[1] >= n - 2 * 16 * 256]
                marks = [m for m in marks if any(b0 <= m < b1 for b0, b1 in keep)]
            calls = 0
            for k0 in range(0, len(marks), per_call):
                chunk = marks[k0:k0 + per_call]
                uv = exact.copy()
                uv[chunk, 0] += unit * 4.0 ** np.arange(len(chunk))
                pts.set_observed(uv)
                loop.run(1, L.LOSS_MEAN_DIST, 0.0)
                loop.wait()
                assert pts.eval_population_info()[1:] == (s, c)
                _, cand, losses = loop.fetch_last()
                assert (cand == cand[0]).all()
                assert np.array_equal(losses.view(np.int64), np.full(K * P, losses[0]).view(np.int64)), chunk
                counts = pc.mark_counts(losses[0] * n, len(chunk), unit)
                assert counts == [1] * len(chunk), (s, c, chunk, counts, losses[0] * n / unit)
                calls += 1
    finally:
        pts.close()
    print(f"[batched coverage] {where} {prec} {variant}: grid {s} x {c}, {len(marks)} marks in {calls} generations")
    assert calls >= 2


VALUE_CASES = [("gcp", "f64", "general", 256, 8, L.LOSS_HUBER), ("gcp", "f32", "lens_free", 256, 8, L.LOSS_MEAN_DIST),
               ("ragged67", "f64", "shared_pose", 256, 16, L.LOSS_HUBER), ("ragged67", "f32", "general", 256, 16, L.LOSS_MEAN_DIST),
               ("tenmillion", "f32", "general", 16, 4096, L.LOSS_HUBER), ("million", "f64", "lens_free", 32, 1024, L.LOSS_MEAN_DIST)]


@pytest.mark.parametrize("where,prec,variant,K,P,kind", VALUE_CASES)
def test_batched_losses(problem, where, prec, variant, K, P, kind):
    """every batched loss against a launch of its start's slice alone; on the GCP and 67-row sets the first and last candidate
    of every start and the tile slots 127 / 128 / 129 against the float64 oracle (float32: also the oracle on the stored inputs)"""
    rng = np.random.default_rng(11)
    fs = 10.0 if kind == L.LOSS_HUBER else 0.0
    oracle = where in ("gcp", "ragged67")
    if oracle:
        xyz, uv = pc.point_set(1127 if where == "gcp" else pc.N, seed=67)
        pts = L.Points(xyz, pc.origin(), prec)
    else:
        pts, uv = _large_set(10_000_000 if where == "tenmillion" else 1_000_000, prec, variant, 9)
        uv = uv + np.random.default_rng(9).normal(0, 1.0, uv.shape)
    R = K * P
    try:
        pts.set_observed(uv)
        with _starts_loop(pts, variant, K, P, 0.02, rng) as loop:
            loop.run(1, kind, fs)
            loop.wait()
            s, c = _check_batched_grid(pts, R, prec, variant)
            _, cand, losses = loop.fetch_last()
        worst_cross = 0.0
        for k in range(K):
            rows = slice(k * P, (k + 1) * P)
            want, _ = pts.eval_population(cand[rows], kind, fs, want_argmin=False)
            assert pts.eval_population_info()[0] == variant
            d = pc_rel(losses[rows], want)
            worst_cross = max(worst_cross, d)
            assert d <= CROSS_GRID_RTOL[prec], (k, d)
    finally:
        pts.close()
    msg = f"[batched losses] {where} {prec} {variant} K {K} x P {P}: grid {s} x {c}; against per-start launches {worst_cross:.3e}"
    if oracle:
        sel = np.unique(np.concatenate([np.arange(K) * P, np.arange(K) * P + P - 1,
                                        [i for i in range(R) if i % pc.TC in (0, 1, pc.TC - 1)]]))
        assert len(sel) >= 512
        ref = pc.oracle_losses(xyz, uv, cand[sel])["huber" if kind == L.LOSS_HUBER else "mean_dist"]
        got = losses[sel]
        worst = float(pc_rel(got, ref))
        if prec == "f64":
            assert worst <= F64_RTOL, worst
        else:
            tol = f32_loss_tolerance(xyz, cand[sel])
            assert np.all(np.abs(got - ref) <= tol * np.abs(ref)), worst
            xyz32, uv32 = pc.local_inputs_f32(xyz, uv, pc.origin())
            ref32 = pc.oracle_losses(xyz32, uv32, cand[sel], pc.origin())["huber" if kind == L.LOSS_HUBER else "mean_dist"]
            w32 = float(pc_rel(got, ref32))
            assert w32 <= F32_STORED_INPUT_RTOL[variant], w32
            msg += f"; stored-input oracle {w32:.3e}"
        msg += f"; float64 oracle ({len(sel)} candidates) {worst:.3e}"
    print(msg)


def pc_rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def test_candidate_buffers_regrown_under_a_live_handle(problem):
    """a larger alp_eval_population between the creation of a 4-start loop and its run(2) regrows the point set's candidate
    records (the lens-free ones move with cand_cap): the generations are bit for bit those of a fresh handle from the same states"""
    obj, img, init = problem
    K, P = 4, 50

    def outcome(loop):
        loop.run(2, L.LOSS_HUBER, 10.0)
        loop.wait()
        return loop.fetch_last(), [loop.get_state(eigen=True, start=k) for k in range(K)]

    with L.Points(obj.to_numpy(), [init["x"], init["y"], init["z"]], "f64") as pts:
        pts.set_observed(img.to_numpy())
        a = _starts_loop(pts, "lens_free", K, P, 0.1, np.random.default_rng(3))
        big = np.tile(L.params_vector(pc.truth("lens_free")), (1000, 1))
        pts.eval_population(big, L.LOSS_HUBER, 10.0)              # 1000 > round_up(K P, 256) = 256 records: regrown
        got, sa = outcome(a)
        assert pts.eval_population_info()[0] == "lens_free"
        a.close()
        b = _starts_loop(pts, "lens_free", K, P, 0.1, np.random.default_rng(3))       # the same states, B started cold
        want, sb = outcome(b)
        b.close()
    for x, y in zip(got, want):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))
    for p, q in zip(sa, sb):
        for key in ("mean", "C", "p_sigma", "pc", "B", "D"):
            np.testing.assert_array_equal(p[key], q[key])
        assert p["sigma"] == q["sigma"] and p["g"] == q["g"]
