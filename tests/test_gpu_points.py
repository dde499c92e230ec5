"""GPU parity tests of the point-set path (projection, losses, residuals, population
evaluation) -- every call goes through the C ABI of libalproj_hip.so via ctypes and is checked
against the CPU oracle and the golden vectors generated from the reference.

Tolerances (north_star: 1e-5 relative, argmin bit-exact):
  * precision "f64": rtol 1e-10 on well-conditioned points (observed ~1e-13), 1e-7 on every
    point incl. those next to the camera plane -- the parity mode
  * precision "f32": |d| <= 1e-5 * max(|ref|, image width): float32 evaluates the distortion
    polynomial in coordinates normalised by the image half-size, so its error is ~1e-7 of the
    image size (~1e-3 px), not of the individual value; ill-conditioned points (|Z_cam| tiny)
    are excluded for f32 and covered by f64.
"""
import os

import numpy as np
import pandas as pd
import pytest

from oracle import ref_numpy as orc
from tests.popeval_cases import oracle_r2, pole_a2_steps

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")


def load(name):
    return np.load(os.path.join(G, name), allow_pickle=False)


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


def well_conditioned(xyz, p, frac=0.02):
    """points whose |depth| along the optical axis is at least `frac` of their distance (the
    reference's camera looks down -Z_cam; its pixel maths is symmetric in the sign of Z_cam)."""
    E = orc.extrinsic_mat(p["pan"], p["tilt"], p["roll"], p["x"], p["y"], p["z"])
    cam = (E[:3, :3] @ xyz.T).T + E[:3, 3]
    dist = np.linalg.norm(cam, axis=1)
    return np.abs(cam[:, 2]) > frac * dist


def f32_loss_tolerance(xyz, cand):
    """1e-5 relative for candidates whose distortion denominators stay away from zero over the
    points; candidates with a pole of the rational distortion model inside the point set
    (|den| < 0.25: garbage poses whose loss is dominated by exploding pixels) amplify the
    float32 rounding by 1/|den| and only get 1e-5/|den|^2 (capped at 2e-2)."""
    tol = []
    for c in cand:
        _, den = orc.conditioning(xyz, orc.vector_to_params(c))
        tol.append(1e-5 if den >= 0.25 else min(2e-2, 1e-5 / max(den, 1e-3) ** 2))
    return np.array(tol)


def f32_report(got, ref, w):
    """What float32 achieves against the float64 reference: max |d| in pixels, the fraction of
    values that also pass the STRICT relative bound |d| <= 1e-5 |ref|, and the smallest |ref| that
    passes it everywhere above.  The float32 floor is set by the INPUT, not the arithmetic: a
    coordinate stored in float32 at distance D from the origin is uncertain by D * 2^-24, which
    moves its pixel by up to fx * 2^-24 ~ 2e-4 px (fx ~ 3659 px) whatever the kernel does; strict
    relative 1e-5 is therefore only attainable for |u|, |v| >~ 20 px, and the bound the float32
    mode is held to is 1e-5 of max(|ref|, image width).  The float64 mode meets the strict bound."""
    d = np.abs(got - ref)
    fin = np.isfinite(ref) & np.isfinite(got)
    strict = d[fin] <= 1e-5 * np.abs(ref[fin])
    return dict(max_abs_px=float(d[fin].max()) if fin.any() else 0.0, strict_rel_pass_fraction=float(strict.mean()) if fin.any() else 1.0,
                max_rel_to_width=float((d[fin] / np.maximum(np.abs(ref[fin]), w)).max()) if fin.any() else 0.0)


def assert_f32_close(got, ref, w, label=None):
    tol = 1e-5 * np.maximum(np.abs(ref), w)
    bad = np.abs(got - ref) > tol
    assert not bad.any(), f"{bad.sum()} values off; worst {np.abs(got - ref).max()} px"
    rep = f32_report(got, ref, w)
    if label:
        print(f"[f32 parity] {label}: max |d| = {rep['max_abs_px']:.3e} px, strict 1e-5-relative pass fraction = "
              f"{rep['strict_rel_pass_fraction']:.6f}, max |d| / max(|ref|, w) = {rep['max_rel_to_width']:.3e}")
    return rep


# ------------------------------------------------------------------ projection
def _project(L, xyz, p, pv, prec):
    with L.Points(xyz, [p["x"], p["y"], p["z"]], prec) as pts:
        pts.project(pv)
        u, v = pts.fetch()
    return np.stack([u, v], 1)


def test_project_f64_golden(L):
    g = load("g3_project.npz")
    for i, pv in enumerate(g["params"]):
        p = orc.vector_to_params(pv)
        # GCP-like points inside the image: the strict bound
        got = _project(L, g[f"xyz_inview_{i}"], p, pv, "f64")
        np.testing.assert_allclose(got, g[f"uv_inview_{i}"], rtol=1e-9, atol=1e-9)
        # a box around the camera: points behind it, next to the camera plane (rounding noise
        # amplified by 1/Z_cam in the reference too) and far outside the image, where the
        # distortion polynomial cancels catastrophically
        keep = [0, 1] + list(range(3, 1000))                     # drop the at-camera point
        got = _project(L, g[f"xyz_{i}"][keep], p, pv, "f64")
        np.testing.assert_allclose(got, g[f"uv_{i}"][keep], rtol=1e-7, atol=1e-7)


def test_project_f32_golden(L):
    g = load("g3_project.npz")
    for i, pv in enumerate(g["params"]):
        p = orc.vector_to_params(pv)
        got = _project(L, g[f"xyz_inview_{i}"], p, pv, "f32")
        rep = assert_f32_close(got, g[f"uv_inview_{i}"], p["w"], label=f"g3 inview set {i}")
        assert rep["strict_rel_pass_fraction"] > 0.99 and rep["max_abs_px"] < 5e-3


def test_project_c1_dsm_316(L):
    """BASELINE config 1's workload (the 316 x 316 = 100 k-vertex synthetic DSM, single pose) through
    the device path in both precisions, every vertex against the oracle."""
    from alproj_amd import synthetic as syn
    n = 316
    s = syn.surface(n)
    xyz = syn.vert_to_xyz_abs(s["vert"], s["offsets"])
    for cam in (syn.standoff_params(n), syn.perturbed(syn.standoff_params(n))):
        ref = orc.project_points(xyz, cam)
        got64 = _project(L, xyz, cam, L.params_vector(cam), "f64")
        # part of this DSM lies far outside the image (v up to 1.4e4 px), where the distortion
        # polynomial cancels: the reference's own rounding there is ~1e-8 px (cf. test_project_f64_golden)
        np.testing.assert_allclose(got64, ref, rtol=1e-9, atol=1e-7)
        got32 = _project(L, xyz, cam, L.params_vector(cam), "f32")
        # this small DSM seen from 0.65 grid lengths away fills a corner of the image with many |u|, |v| under
        # 100 px: the strict-relative fraction is reported, the absolute error is what is bounded
        assert_f32_close(got32, ref, cam["w"], label="c1 316x316 DSM (all vertices, most of them outside the image)")
        inside = (ref[:, 0] >= 0) & (ref[:, 0] < cam["w"]) & (ref[:, 1] >= 0) & (ref[:, 1] < cam["h"])
        if inside.any():
            assert np.abs(got32[inside] - ref[inside]).max() < 5e-3


def test_project_known_answers_and_nan(L):
    g = load("g3_project.npz")
    pv = g["params_known"]
    p = orc.vector_to_params(pv)
    with L.Points(g["xyz_known"], [p["x"], p["y"], p["z"]], "f64") as pts:
        pts.project(pv)
        u, v = pts.fetch()
    assert abs(u[0] - 2858.677447353897) < 1e-7 and abs(v[0] - 1922.6842974827396) < 1e-7
    assert abs(u[3] - 2495.822292923295) < 1e-7 and abs(v[3] - 2100.8565488830186) < 1e-7   # behind camera
    assert np.isnan(u[4]) and np.isnan(v[4])                                                # at camera (Q7)


def test_project_python_api(L):
    from alproj_amd import optimize as opt
    g = load("g3_project.npz")
    p = orc.vector_to_params(g["params"][1])
    xyz = g["xyz_1"][3:]
    df = opt.project(pd.DataFrame(xyz, columns=["x", "y", "z"]), p)
    assert list(df.columns) == ["u", "v"] and len(df) == len(xyz)
    np.testing.assert_allclose(df.to_numpy(), g["uv_1"][3:], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("n", [0, 1, 3, 255, 256, 257, 1023, 1025, 4099])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_project_ragged_sizes(L, n, prec):
    from alproj_amd import synthetic as syn
    p = syn.truth_params(316)
    xyz = syn.gcp_points(max(n, 1), p, seed=n + 7)[:n]
    with L.Points(xyz, [p["x"], p["y"], p["z"]], prec) as pts:
        pts.project(L.params_vector(p))
        u, v = pts.fetch()
    assert u.shape == (n,)
    if n:
        ref = orc.project_points(xyz, p)
        if prec == "f64":
            np.testing.assert_allclose(np.stack([u, v], 1), ref, rtol=1e-9, atol=1e-9)
        else:
            assert_f32_close(np.stack([u, v], 1), ref, p["w"])


# ------------------------------------------------------------------ stand-alone losses / residuals
def test_losses_golden(L):
    from alproj_amd import optimize as opt
    g = load("g4_losses.npz")
    dfo = pd.DataFrame(g["obs"], columns=["u", "v"])
    dfp = pd.DataFrame(g["proj"], columns=["u", "v"])
    assert opt.rmse(dfo, dfp) == pytest.approx(float(g["rmse"]), rel=1e-13)
    assert opt.huber_loss(dfo, dfp) == pytest.approx(float(g["huber_default"]), rel=1e-13)
    assert opt.huber_loss(dfo, dfp, 1000.0) == pytest.approx(float(g["huber_1000"]), rel=1e-13)
    assert opt.huber_loss(dfo, dfp, 0.5) == pytest.approx(float(g["huber_0p5"]), rel=1e-13)


def test_float32_observations_into_a_float64_set(L):
    """alp_points_set_observed with float32 pixels on a float64 point set (the one aos_to_planes instantiation the suite
    had not launched): the observations are widened exactly"""
    from alproj_amd import synthetic as syn
    truth = syn.truth_params(316)
    xyz = syn.gcp_points(3001, truth, seed=5)
    uv32 = (orc.project_points(xyz, truth) + np.random.default_rng(5).normal(0, 1.0, (3001, 2))).astype(np.float32)
    cand = np.stack([L.params_vector(truth), L.params_vector(dict(truth, pan=truth["pan"] + 0.3))])
    with L.Points(xyz, [truth["x"], truth["y"], truth["z"]], "f64") as a, L.Points(xyz, [truth["x"], truth["y"], truth["z"]], "f64") as b:
        a.set_observed(uv32)
        b.set_observed(uv32.astype(np.float64))
        la, _ = a.eval_population(cand, L.LOSS_HUBER, 10.0)
        lb, _ = b.eval_population(cand, L.LOSS_HUBER, 10.0)
        np.testing.assert_array_equal(la, lb)
        np.testing.assert_array_equal(a.residuals(cand[1]), b.residuals(cand[1]))
    ref = orc.huber(uv32.astype(np.float64), orc.project_points(xyz, orc.vector_to_params(cand[1])), 10.0)
    assert la[1] == pytest.approx(ref, rel=1e-9)
    # ... and float32 pixels on a float32 set are taken as they are (the same planes as their float64 copy rounds to)
    with L.Points(xyz, [truth["x"], truth["y"], truth["z"]], "f32") as a, L.Points(xyz, [truth["x"], truth["y"], truth["z"]], "f32") as b:
        a.set_observed(uv32)
        b.set_observed(uv32.astype(np.float64))
        np.testing.assert_array_equal(a.eval_population(cand, L.LOSS_HUBER, 10.0)[0], b.eval_population(cand, L.LOSS_HUBER, 10.0)[0])


def test_losses_take_either_table_layout(L):
    """rmse / huber_loss (optimize.py:157-212) through alp_loss_uv_columns: row-major pairs, two columns (what project()
    returns), DataFrames of either build, a mix of both -- the same bits every time, and the reference's value"""
    from alproj_amd import optimize as opt
    rng = np.random.default_rng(8)
    n = 70_001
    obs = rng.uniform(0, 5000, (n, 2))
    prj = obs + rng.normal(0, 6.0, (n, 2))
    forms_o = [obs, np.asfortranarray(obs), pd.DataFrame(obs, columns=["u", "v"]), pd.DataFrame({"u": obs[:, 0], "v": obs[:, 1]}),
               pd.DataFrame({"v": obs[:, 1], "k": 1, "u": obs[:, 0]})]
    # `projected` is taken BY POSITION like the reference's projected.to_numpy() (optimize.py:175, 203): an unlabelled frame,
    # other labels, a third column behind the two
    forms_p = [prj, np.asfortranarray(prj), pd.DataFrame(prj, columns=["u", "v"]), pd.DataFrame({"u": prj[:, 0].copy(), "v": prj[:, 1].copy()}, copy=False),
               pd.DataFrame(prj), pd.DataFrame(prj, columns=["col", "row"]), pd.DataFrame({"u": prj[:, 0], "v": prj[:, 1], "extra": 7.0})]
    want_r, want_h = orc.mean_distance(obs, prj), orc.huber(obs, prj, 10.0)
    seen = set()
    for a in forms_o:
        for b in forms_p:
            seen.add((opt.rmse(a, b), opt.huber_loss(a, b, 10.0)))
    assert len(seen) == 1
    r, h = seen.pop()
    assert r == pytest.approx(want_r, rel=1e-13) and h == pytest.approx(want_h, rel=1e-13)
    # a frame ordered [v, u] is read as it lies (position 0 against the observed u), as the reference reads it
    swapped = pd.DataFrame({"v": prj[:, 1], "u": prj[:, 0]})
    assert opt.rmse(obs, swapped) == pytest.approx(orc.mean_distance(obs, prj[:, ::-1]), rel=1e-13)
    with pytest.raises(IndexError):
        opt.rmse(obs, pd.DataFrame({"u": prj[:, 0]}))
    with pytest.raises(ValueError):
        opt.rmse(obs, prj[:-1])
    assert np.isnan(opt.rmse(np.zeros((0, 2)), np.zeros((0, 2))))


def test_residuals_golden(L):
    from alproj_amd import optimize as opt
    g = load("g8_residuals.npz")
    p = orc.vector_to_params(g["params"])
    r = opt.compute_residuals(pd.DataFrame(g["xyz"], columns=["x", "y", "z"]),
                              pd.DataFrame(g["uv_obs"], columns=["u", "v"]), p)
    assert r.shape == g["residuals"].shape
    np.testing.assert_allclose(r, g["residuals"], rtol=1e-9, atol=1e-9)


# ------------------------------------------------------------------ population evaluation
def _cand_matrix(L, init, tgt, bounds, X):
    base = L.params_vector(init)
    cand = np.tile(base, (len(X), 1))
    cols = [L.PARAM_KEYS.index(t) for t in tgt]
    cand[:, cols] = X * (bounds[:, 1] - bounds[:, 0]) + bounds[:, 0]
    return cand


@pytest.mark.parametrize("name", ["d9", "d12", "d21"])
@pytest.mark.parametrize("prec,rtol", [("f64", 1e-8), ("f32", 1e-5)])
def test_population_golden(L, name, prec, rtol):
    g = load("g5_population.npz")
    init = orc.vector_to_params(g["params_init"])
    tgt = [str(t) for t in g[f"{name}_targets"]]
    cand = _cand_matrix(L, init, tgt, g[f"{name}_bounds"], g[f"{name}_X"])
    with L.Points(g["xyz"], [init["x"], init["y"], init["z"]], prec) as pts:
        pts.set_observed(g["uv_obs"])
        for tag, kind, fs in (("md", L.LOSS_MEAN_DIST, 0.0), ("hub", L.LOSS_HUBER, 10.0)):
            losses, amin = pts.eval_population(cand, kind, fs)
            ref = g[f"{name}_{tag}"]
            tol = np.full(len(ref), rtol)
            if prec == "f32":
                tol = f32_loss_tolerance(g["xyz"], cand)
            assert np.all(np.abs(losses - ref) <= tol * np.abs(ref)), np.abs(losses / ref - 1).max()
            assert amin == int(np.argmin(ref))          # argmin bit-exact (first index on the tie)
            assert losses[3] == losses[7]               # identical candidates -> identical sums


@pytest.mark.parametrize("prec,rtol", [("f64", 1e-9), ("f32", 1e-5)])
def test_first_phase_population_golden(L, prec, rtol):
    """g19: the REFERENCE's own losses of its first optimisation phase (example.py:19-22, 51-54: no lens coefficients, targets
    x, y, z, fov, pan, tilt, roll, a1, a2; 140 candidates = two tiles, the second ragged) -- the population the lens-free kernel
    variant exists for; argmin bit-exact (the truth at row 11, a tie between rows 3 and 7)"""
    g = load("g19_first_phase.npz")
    init = orc.vector_to_params(g["params_init"])
    tgt = [str(t) for t in g["targets"]]
    cand = _cand_matrix(L, init, tgt, g["bounds"], g["X"])
    with L.Points(g["xyz"], [init["x"], init["y"], init["z"]], prec) as pts:
        pts.set_observed(g["uv_obs"])
        for tag, kind, fs in (("md", L.LOSS_MEAN_DIST, 0.0), ("hub", L.LOSS_HUBER, 10.0)):
            losses, amin = pts.eval_population(cand, kind, fs)
            assert pts.eval_population_info()[0] == "lens_free"
            np.testing.assert_allclose(losses, g[tag], rtol=rtol)
            assert amin == int(np.argmin(g[tag])) == 11
            assert losses[3] == losses[7]


def test_population_golden_wild_f64(L):
    """stress set: points mostly outside the image, losses ~1e10 dominated by a few exploding
    distortion polynomials -- float64 mode still tracks the reference"""
    g = load("g5_population.npz")
    init = orc.vector_to_params(g["params_init"])
    tgt = [str(t) for t in g["d21_targets"]]
    cand = _cand_matrix(L, init, tgt, g["d21_bounds"], g["d21_X"])
    with L.Points(g["wild_xyz"], [init["x"], init["y"], init["z"]], "f64") as pts:
        pts.set_observed(g["wild_uv_obs"])
        for tag, kind, fs in (("md", L.LOSS_MEAN_DIST, 0.0), ("hub", L.LOSS_HUBER, 10.0)):
            losses, amin = pts.eval_population(cand, kind, fs)
            ref = g[f"wild_d21_{tag}"]
            np.testing.assert_allclose(losses, ref, rtol=1e-7)
            assert amin == int(np.argmin(ref))


def test_points_from_columns_as_they_lie(L):
    """alp_points_create_columns / alp_points_set_observed_columns (ABI 6): the reference's `obj_points[["x", "y", "z"]]` and
    `img_points[["u", "v"]]` reach the device column by column, without the host-side interleaving -- and give the very planes
    the row-major upload gives: identical projections, residuals and losses whatever the layout of the table"""
    from alproj_amd import optimize as opt
    from alproj_amd import synthetic as syn
    truth = syn.truth_params(316)
    init = dict(truth, pan=truth["pan"] + 0.7, fov=truth["fov"] - 1.0)
    n = 40_003
    xyz = syn.gcp_points(n, truth, seed=21)
    uv = orc.project_points(xyz, truth) + np.random.default_rng(21).normal(0, 1.0, (n, 2))
    origin = [truth["x"], truth["y"], truth["z"]]
    cand = np.stack([L.params_vector(init), L.params_vector(truth)])
    for prec in ("f64", "f32"):
        with L.Points(xyz, origin, prec) as a:
            a.set_observed(uv)
            a.project(L.params_vector(init))
            ua, va = a.fetch()
            la, _ = a.eval_population(cand, L.LOSS_HUBER, 10.0)
            ra = a.residuals(L.params_vector(init))
        forms = {
            "F-ordered arrays": (np.asfortranarray(xyz), np.asfortranarray(uv)),
            "float32 columns": None,
        }
        for name, pair in forms.items():
            if pair is None:
                if prec == "f64":
                    continue
                x32 = [np.ascontiguousarray((xyz[:, k] - origin[k]).astype(np.float32)) for k in range(3)]
                with L.Points.from_columns(*x32, [0.0, 0.0, 0.0], prec) as b, \
                        L.Points(np.stack(x32, 1), [0.0, 0.0, 0.0], prec) as c:
                    local = dict(init, x=init["x"] - origin[0], y=init["y"] - origin[1], z=init["z"] - origin[2])
                    for q in (b, c):
                        q.project(L.params_vector(local))
                    np.testing.assert_array_equal(b.fetch()[0], c.fetch()[0])
                    np.testing.assert_array_equal(b.fetch()[1], c.fetch()[1])
                continue
            with L.Points(pair[0], origin, prec) as b:
                b.set_observed(pair[1])
                b.project(L.params_vector(init))
                ub, vb = b.fetch()
                lb, _ = b.eval_population(cand, L.LOSS_HUBER, 10.0)
                np.testing.assert_array_equal(ub, ua, err_msg=name)
                np.testing.assert_array_equal(vb, va, err_msg=name)
                np.testing.assert_array_equal(lb, la, err_msg=name)
                np.testing.assert_array_equal(b.residuals(L.params_vector(init)), ra, err_msg=name)
        with L.Points.from_columns(xyz[:, 0], xyz[:, 1], xyz[:, 2], origin, prec) as b:       # strided views: made contiguous per column
            b.set_observed_columns(uv[:, 0].copy(), uv[:, 1].copy())
            lb, _ = b.eval_population(cand, L.LOSS_HUBER, 10.0)
            np.testing.assert_array_equal(lb, la)
    # the reference's signatures over every table layout: one result
    frames = {
        "from a row-major array": (pd.DataFrame(xyz, columns=["x", "y", "z"]), pd.DataFrame(uv, columns=["u", "v"])),
        "built column by column": (pd.DataFrame({"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2]}), pd.DataFrame({"u": uv[:, 0], "v": uv[:, 1]})),
        "more columns, another order, an integer column": (
            pd.DataFrame({"id": np.arange(n), "z": xyz[:, 2], "x": xyz[:, 0], "name": "p", "y": xyz[:, 1]}),
            pd.DataFrame({"v": uv[:, 1], "w": 1.0, "u": uv[:, 0]})),
    }
    ref_uv = ref_res = None
    for name, (fo, fi) in frames.items():
        got = opt.project(fo, init)
        res = opt.compute_residuals(fo, fi, init)
        assert list(got.columns) == ["u", "v"] and got["u"].dtype == np.float64 and len(got) == n
        if ref_uv is None:
            ref_uv, ref_res = got, res
            np.testing.assert_allclose(got.to_numpy(), orc.project_points(xyz, init), rtol=1e-9, atol=1e-9)
        else:
            assert got.equals(ref_uv), name
            np.testing.assert_array_equal(res, ref_res, err_msg=name)
    with pytest.raises(ValueError):
        L.Points.from_columns(xyz[:, 0], xyz[:10, 1], xyz[:, 2], origin)
    with L.Points.from_columns(np.zeros(0), np.zeros(0), np.zeros(0), origin) as e:
        assert e.n == 0


@pytest.mark.parametrize("mode,threads", [("host", "1"), ("host", "5"), ("host", None), ("device", None), (None, None)])
@pytest.mark.parametrize("n", [1, 70_001, (8 << 20) + 3, 2 * (8 << 20)], ids=["one", "below_the_thread_threshold", "two_chunks_ragged", "two_chunks_exact"])
def test_fetch_in_the_other_element_type(L, n, mode, threads, monkeypatch):
    """alp_projected_fetch with a change of type (a float32 set fetched as the reference's float64, and the reverse): the
    pipelined host conversion (any thread count, chunk borders, ragged tails) and the device conversion both give exactly
    the stored values widened / narrowed -- NaN and infinities included"""
    from alproj_amd import synthetic as syn
    if mode:
        monkeypatch.setenv("ALP_FETCH_CONVERT", mode)
    if threads:
        monkeypatch.setenv("ALP_HOST_THREADS", threads)
    truth = syn.truth_params(316)
    rng = np.random.default_rng(n)
    xyz = np.array([truth["x"], truth["y"], truth["z"]]) + rng.uniform(-900, 900, (n, 3))
    xyz[n // 2] = [truth["x"], truth["y"], truth["z"]]            # the camera itself: NaN (quirk Q7)
    for prec, other in (("f32", np.float64), ("f64", np.float32)):
        with L.Points(xyz, [truth["x"], truth["y"], truth["z"]], prec) as pts:
            pts.project(L.params_vector(truth))
            own = np.float32 if prec == "f32" else np.float64
            u0, v0 = pts.fetch(own)
            u1, v1 = pts.fetch(other)
            assert u1.dtype == other and np.isnan(u0[n // 2])
            with np.errstate(over="ignore"):
                np.testing.assert_array_equal(u1, u0.astype(other))
                np.testing.assert_array_equal(v1, v0.astype(other))
            del u0, v0, u1, v1


@pytest.mark.parametrize("n,P", [(1, 1), (63, 3), (256, 256), (257, 257), (2048, 300), (2049, 5), (5000, 513)])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_population_ragged(L, n, P, prec):
    """sizes around the 256-point tile, the 256/128-candidate LDS tile and the V-group tail"""
    from alproj_amd import synthetic as syn
    truth = syn.truth_params(316)
    init = syn.base_params(316)
    xyz = syn.gcp_points(n, truth, seed=n)
    rng = np.random.default_rng(P)
    uv = orc.project_points(xyz, truth) + rng.normal(0, 1.0, (n, 2))
    bounds = orc.bounds_to_array(init, syn.TARGETS_D21)
    X = rng.uniform(0.35, 0.65, (P, 21))
    cand = _cand_matrix(L, init, syn.TARGETS_D21, bounds, X)
    with L.Points(xyz, [init["x"], init["y"], init["z"]], prec) as pts:
        pts.set_observed(uv)
        losses, amin = pts.eval_population(cand, L.LOSS_HUBER, 10.0)
    sel = np.unique(np.concatenate([[0, P - 1, P // 2], rng.integers(0, P, 6)]))
    ref = np.array([orc.huber(uv, orc.project_points(xyz, orc.vector_to_params(cand[i])), 10.0) for i in sel])
    tol = np.full(len(sel), 1e-8) if prec == "f64" else f32_loss_tolerance(xyz, cand[sel])
    assert np.all(np.abs(losses[sel] - ref) <= tol * np.abs(ref)), np.abs(losses[sel] / ref - 1).max()
    assert losses.shape == (P,) and np.isfinite(losses).all()
    assert amin == int(np.argmin(losses))


def test_population_nan_semantics(L):
    """a point AT the camera poisons that candidate's mean like np.mean does (Q7); NaN never
    wins the argmin"""
    from alproj_amd import synthetic as syn
    p = syn.base_params(316)
    xyz = syn.gcp_points(100, p, seed=3)
    uv = orc.project_points(xyz, p)
    cands = np.stack([L.params_vector(p), L.params_vector(dict(p, x=p["x"] + 1.0))])
    xyz[5] = [p["x"], p["y"], p["z"]]            # candidate 0's camera position exactly
    with L.Points(xyz, [p["x"], p["y"], p["z"]], "f64") as pts:
        pts.set_observed(uv)
        losses, amin = pts.eval_population(cands, L.LOSS_MEAN_DIST, 0.0)
    assert np.isnan(losses[0]) and np.isfinite(losses[1]) and amin == 1


@pytest.mark.parametrize("variant", ["shared_pose", "general"])
@pytest.mark.parametrize("kind,fs", [(0, 0.0), (1, 10.0)], ids=["mean_dist", "huber"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_pole_of_one_lens_denominator_is_an_infinite_loss(L, prec, kind, fs, variant):
    """optimize.py:112-116 at a vertex where EXACTLY ONE denominator of the rational lens model is zero: the reference's
    coordinate on that axis is +-inf, the other finite, the candidate's loss +inf.  The kernel shares one reciprocal between
    the two denominators (0 * inf = NaN on the finite axis).  float64 (the parity mode) puts that right: +inf, never NaN; float32
    keeps NaN (documented).  Either way: never the argmin, and CMA.tell's order the same as with the oracle's inf.

    Construction.  k4 = -0.5, k5 = k6 = 0: den_y = (1 + a2) - r2 / 2 is zero iff 1 + a2 == r2 / 2 bit for bit (the product
    -0.5 r2 is exact), den_x = 1 - r2 / 2 is not.  r2 of the chosen out-of-frame vertex is known to a few ulps only (the
    device's own folding of the pose and, for float32, its rounded coordinates), so the population steps 1 + a2 ulp by ulp
    through r2 / 2 +- W ulps: one of the candidates sits exactly on the device's pole.  The oracle's own pole is r2_oracle / 2."""
    from alproj_amd import synthetic as syn
    from alproj_amd.cma import CMA
    truth = dict(syn.truth_params(316), k4=-0.5, k5=0.0, k6=0.0)
    xyz = syn.gcp_points(400, truth, seed=31, margin=-0.25)            # a quarter of the frame beyond each edge
    r2 = oracle_r2(xyz, truth)
    i0 = int(np.argmin(np.abs(r2 - 1.4)))                               # den_x = 1 - r2/2 ~ 0.3 there
    assert 1.2 < r2[i0] < 1.6
    # nobody else near a pole of either denominator of the SANE candidates (den_x = 1 - r2/2, den_y = 1 + a2 - r2/2)
    keep = (np.abs(1 - r2 / 2) > 0.25) & (np.abs(1 + truth["a2"] - r2 / 2) > 0.25)
    keep[i0] = True
    i = int(np.count_nonzero(keep[:i0]))
    xyz, r2 = xyz[keep], r2[keep]
    assert len(xyz) > 100
    uv = orc.project_points(xyz, truth) + np.random.default_rng(31).normal(0, 1.0, (len(xyz), 2))
    assert np.isfinite(uv).all()
    a2 = pole_a2_steps(r2[i], -0.5, prec)                               # 1 + a2 steps ulp by ulp through r2 / 2
    cand = np.tile(L.params_vector(truth), (len(a2) + 2, 1))
    cand[2:, L.PARAM_KEYS.index("a2")] = a2
    cand[1, L.PARAM_KEYS.index("a1")] += 0.01                           # two sane candidates in front
    if variant == "general":
        cand[0, L.PARAM_KEYS.index("pan")] += 0.01                      # one pose differs: the general kernel variant
    with L.Points(xyz, [truth["x"], truth["y"], truth["z"]], prec) as pts:
        pts.set_observed(uv)
        losses, amin = pts.eval_population(cand, kind, fs)
        hit = np.flatnonzero(~np.isfinite(losses))
        assert len(hit) >= 1, "no candidate landed on the device's pole: widen W"
        if prec == "f64":
            assert np.all(np.isposinf(losses[hit])), losses[hit]        # the parity mode: +inf like the reference, not NaN
        # (float32 mode: NaN or inf -- it keeps the shared reciprocal's NaN at an exact pole, include/alproj_hip.h: the second
        # walk that mends it cannot mend the float32 overflows of a wild population and doubled their kernel time)
        assert amin in (0, 1) and amin == int(np.argmin(np.where(np.isnan(losses), np.inf, losses)))
        # the two sane candidates are untouched by the second walk their wave made for the pole candidate's sake
        ref2 = np.array([orc.loss_of(xyz, uv, orc.vector_to_params(c), kind, fs) for c in cand[:2]])
        # (float32: the losses here are the 1-px noise itself -- 1.0 px mean distance, 1.0 Huber -- so the float32 pixel floor of
        # ~2e-4 px, amplified by denominators down to 0.25, is 2e-4 of the LOSS; candidate 0 is exact to 1.8e-4 in the worst case seen)
        np.testing.assert_allclose(losses[:2], ref2, rtol=1e-9 if prec == "f64" else 1e-3)
        # small population: [sane, sane, ON the pole]; the oracle sits on ITS pole (r2 as numpy forms it)
        small = cand[[0, 1, int(hit[0])]]
        l_dev, amin_small = pts.eval_population(small, kind, fs)
    o_pole = cand[int(hit[0])].copy()
    o_pole[L.PARAM_KEYS.index("a2")] = r2[i] / 2 - 1.0
    l_ref = np.array(list(ref2) + [orc.loss_of(xyz, uv, orc.vector_to_params(o_pole), kind, fs)])
    assert np.isposinf(l_ref[2]), "the oracle's own pole candidate must be infinite (optimize.py:115)"
    assert (np.isposinf(l_dev[2]) if prec == "f64" else not np.isfinite(l_dev[2])) and amin_small == int(np.argmin(l_ref))
    orders = []
    for values in (l_dev, l_ref):
        es = CMA(mean=np.full(3, 0.5), sigma=0.2, bounds=np.tile([0.0, 1.0], (3, 1)), population_size=3, seed=1)
        sol = [(np.full(3, 0.1 * (k + 1)), float(v)) for k, v in enumerate(values)]
        es.tell(sol)
        orders.append([round(s[0][0] * 10) - 1 for s in sol])
    assert orders[0] == orders[1] and orders[0][-1] == 2               # same order; the pole candidate last


def test_residuals_are_observed_minus_project_bit_for_bit_f64(L):
    """optimize.py:233-236: compute_residuals IS (img_points - project(...)).flatten(); the float64 kernel keeps the identity
    to the bit (it runs alp_project's arithmetic), also next to the camera plane and at a pole"""
    from alproj_amd import synthetic as syn
    truth = dict(syn.truth_params(316), k4=-0.5, k5=0.01, k6=0.002)
    xyz = syn.gcp_points(5000, truth, seed=41, margin=-0.3)
    uv = np.random.default_rng(41).uniform(0, 5000, (5000, 2))
    with L.Points(xyz, [truth["x"], truth["y"], truth["z"]], "f64") as pts:
        pts.set_observed(uv)
        vec = L.params_vector(truth)
        pts.project(vec)
        u, v = pts.fetch()
        res = pts.residuals(vec)
        batch = pts.residuals_batch(np.stack([vec, vec]))
    want = (uv - np.stack([u, v], 1)).ravel()
    assert np.array_equal(res, want)
    assert np.array_equal(batch[0], want) and np.array_equal(batch[1], want)


@pytest.mark.parametrize("kind,fs", [(0, 0.0), (1, 10.0)], ids=["mean_dist", "huber"])
@pytest.mark.parametrize("prec,rtol_oracle,rtol_general", [("f64", 1e-9, 1e-12), ("f32", 1e-5, 2e-6)])
def test_population_lens_free_variant(L, prec, rtol_oracle, rtol_general, kind, fs, monkeypatch):
    """Populations in which no candidate has a lens coefficient other than a1, a2 -- the reference's first phase
    (example.py:51-54: targets x, y, z, fov, pan, tilt, roll, a1, a2 around k = p = s = 0; BASELINE config 3) -- take the kernel
    variant that runs on pose rows with the lens folded in (16 + 2 instead of 45 + 3 vector instructions per evaluation).
    Same losses as the oracle and as the general variant (forced by ALP_POP_NO_LENS_FREE, or by one candidate with a lens),
    same argmin; ragged point count, two candidate tiles with a ragged second one."""
    from alproj_amd import synthetic as syn
    truth = dict(syn.truth_params(316), **{k: 0.0 for k in L.DIST_KEYS[2:]})
    init = dict(syn.base_params(316), **{k: 0.0 for k in L.DIST_KEYS[2:]})
    n, P = 3001 + 6 * 256, 130
    xyz = syn.gcp_points(n, truth, seed=51)
    uv = orc.project_points(xyz, truth) + np.random.default_rng(51).normal(0, 1.0, (n, 2))
    rng = np.random.default_rng(52)
    bounds = orc.bounds_to_array(init, syn.TARGETS_D9)
    X = rng.uniform(0.45, 0.55, (P, 9))
    cand = np.tile(L.params_vector(init), (P, 1))
    cols = [L.PARAM_KEYS.index(t) for t in syn.TARGETS_D9]
    cand[:, cols] = X * (bounds[:, 1] - bounds[:, 0]) + bounds[:, 0]
    cand[7] = L.params_vector(truth)                                    # the winner
    with L.Points(xyz, [init["x"], init["y"], init["z"]], prec) as pts:
        pts.set_observed(uv)
        losses, amin = pts.eval_population(cand, kind, fs)
        assert pts.eval_population_info()[0] == "lens_free"
        monkeypatch.setenv("ALP_POP_NO_LENS_FREE", "1")
        general, amin_g = pts.eval_population(cand, kind, fs)
        assert pts.eval_population_info()[0] == "general"
        monkeypatch.delenv("ALP_POP_NO_LENS_FREE")
        with_lens = np.vstack([cand, cand[:1]])
        with_lens[-1, L.PARAM_KEYS.index("k1")] = 1e-3                  # one candidate with a lens: the whole call goes general
        mixed, _ = pts.eval_population(with_lens, kind, fs)
        assert pts.eval_population_info()[0] == "general"
        one, amin_1 = pts.eval_population(cand[7:8], kind, fs)          # a population of one
        assert pts.eval_population_info()[0] == "lens_free" and amin_1 == 0
    sel = np.unique(np.concatenate([[0, 7, P - 1, 127, 128], rng.integers(0, P, 8)]))
    ref = np.array([orc.loss_of(xyz, uv, orc.vector_to_params(c), kind, fs) for c in cand[sel]])
    np.testing.assert_allclose(losses[sel], ref, rtol=rtol_oracle)
    np.testing.assert_allclose(losses, general, rtol=rtol_general)
    np.testing.assert_allclose(mixed[:P], general, rtol=0, atol=0)      # the same general kernel: the same bits
    np.testing.assert_allclose(one, losses[7:8], rtol=rtol_general)
    assert amin == amin_g == 7 == int(np.argmin(losses))


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_lens_free_variant_keeps_the_references_nan_and_inf(L, prec):
    """What the folded rows cannot say, the second walk of the kernel (general arithmetic on the general records) restores:
    a vertex AT the camera makes that candidate's mean NaN (Q7: 0 / 0 and k . inf = NaN in optimize.py:112-116 even with k = 0),
    a candidate with a2 = -1 divides by zero (inf).  Neither wins; the other candidates are untouched."""
    from alproj_amd import synthetic as syn
    p = dict(syn.base_params(316), **{k: 0.0 for k in L.DIST_KEYS[2:]})
    xyz = syn.gcp_points(700, p, seed=53)
    uv = orc.project_points(xyz, p) + np.random.default_rng(53).normal(0, 1.0, (700, 2))
    cands = np.stack([L.params_vector(p), L.params_vector(dict(p, x=p["x"] + 1.0)), L.params_vector(dict(p, a2=-1.0, x=p["x"] + 2.0)),
                      L.params_vector(dict(p, pan=p["pan"] + 0.1))])
    xyz[5] = [p["x"], p["y"], p["z"]]            # candidate 0's (and 3's) camera position exactly
    with np.errstate(all="ignore"):
        ref = np.array([orc.loss_of(xyz, uv, orc.vector_to_params(c), 0, 0.0) for c in cands])
    assert np.isnan(ref[0]) and np.isfinite(ref[1]) and np.isposinf(ref[2]) and np.isnan(ref[3])
    with L.Points(xyz, [p["x"], p["y"], p["z"]], prec) as pts:
        pts.set_observed(uv)
        losses, amin = pts.eval_population(cands, L.LOSS_MEAN_DIST, 0.0)
        assert pts.eval_population_info()[0] == "lens_free"
    assert np.isnan(losses[0]) and np.isnan(losses[3]) and np.isposinf(losses[2]) and amin == 1
    assert losses[1] == pytest.approx(ref[1], rel=1e-9 if prec == "f64" else 1e-5)


@pytest.mark.parametrize("prec,rtol", [("f64", 1e-12), ("f32", 2e-6)])
def test_population_shared_pose_path(L, prec, rtol):
    """distortion-only populations (every candidate shares the 3x4 pose matrix) take a kernel
    variant that hoists the transform out of the candidate loop: same losses as the general
    variant, which is forced by appending one candidate with another pan"""
    from alproj_amd import synthetic as syn
    truth = syn.truth_params(316)
    xyz = syn.gcp_points(3000, truth, seed=8)
    rng = np.random.default_rng(8)
    uv = orc.project_points(xyz, truth) + rng.normal(0, 1.0, (3000, 2))
    cand = np.tile(L.params_vector(truth), (130, 1))
    cand[:, 7:21] += rng.uniform(-0.01, 0.01, (130, 14))          # a1, a2, k1..s4 only
    other = cand[:1].copy()
    other[0, 4] += 0.5                                             # pan
    with L.Points(xyz, [truth["x"], truth["y"], truth["z"]], prec) as pts:
        pts.set_observed(uv)
        for kind, fs in ((L.LOSS_HUBER, 10.0), (L.LOSS_MEAN_DIST, 0.0)):
            shared, amin_s = pts.eval_population(cand, kind, fs)
            general, amin_g = pts.eval_population(np.vstack([cand, other]), kind, fs)
            np.testing.assert_allclose(shared, general[:130], rtol=rtol)
            ref = np.array([orc.loss_of(xyz, uv, orc.vector_to_params(c), kind, fs) for c in cand[:5]])
            np.testing.assert_allclose(shared[:5], ref, rtol=1e-9 if prec == "f64" else 1e-5)
            assert amin_s == int(np.argmin(shared))


def test_population_needs_observed(L):
    from alproj_amd import synthetic as syn
    p = syn.base_params(316)
    xyz = syn.gcp_points(10, p)
    with L.Points(xyz, [p["x"], p["y"], p["z"]], "f32") as pts:
        with pytest.raises(L.AlprojHipError) as e:
            pts.eval_population(L.params_vector(p)[None, :], L.LOSS_MEAN_DIST, 0.0)
        assert e.value.code == -6


def _near_tie_case(L):
    """GCP set + candidate pairs whose float64 losses differ by ~1e-7 relative: far below what
    float32 losses resolve (~1e-6..1e-5), so the float32 argmin alone would be a coin toss."""
    from alproj_amd import synthetic as syn
    truth = syn.truth_params(316)
    xyz = syn.gcp_points(4000, truth, seed=21)
    uv = orc.project_points(xyz, truth) + np.random.default_rng(21).normal(0, 1.0, (4000, 2))
    base = L.params_vector(dict(truth, pan=truth["pan"] + 0.02))
    return truth, xyz, uv, base


@pytest.mark.parametrize("kind,fs", [(0, 0.0), (1, 10.0)], ids=["mean_dist", "huber"])
def test_argmin_confirmation_on_near_ties(L, kind, fs):
    """north star: argmin pose index bit-exact.  Two candidates ~1e-7 apart (relative loss), in both
    orders and among worse ones: the float32 set must return the float64 oracle's argmin."""
    truth, xyz, uv, base = _near_tie_case(L)
    rng = np.random.default_rng(5)
    origin = [truth["x"], truth["y"], truth["z"]]
    trials = 0
    with L.Points(xyz, origin, "f32") as pts:
        pts.set_observed(uv)
        for t in range(60):
            if trials >= 8:
                break
            a = base.copy()
            b = base.copy()
            b[4] += rng.choice([-1, 1]) * 10.0 ** rng.uniform(-8.0, -6.5)      # pan: a tiny nudge
            worse = np.tile(base, (6, 1))
            worse[:, 4] += rng.uniform(0.05, 0.5, 6)
            order = [a, b] if t % 2 == 0 else [b, a]
            cand = np.vstack([worse[:3], order[0], worse[3:5], order[1], worse[5:]])
            ref = np.array([orc.loss_of(xyz, uv, orc.vector_to_params(c), kind, fs) for c in cand])
            gap = abs(ref[3] - ref[6]) / ref.min()
            if not (0 < gap < 2e-6):
                continue
            trials += 1
            losses, amin = pts.eval_population(cand, kind, fs)
            assert amin == int(np.argmin(ref)), (t, gap, losses[[3, 6]], ref[[3, 6]])
            # the confirmed candidates carry float64-arithmetic losses (float32 coordinates remain)
            np.testing.assert_allclose(losses[[3, 6]], ref[[3, 6]], rtol=2e-7)
    assert trials >= 6


def test_argmin_confirmation_band_larger_than_its_capacity(L):
    """40 identical candidates (more than the 16 the confirmation evaluates): first index wins."""
    truth, xyz, uv, base = _near_tie_case(L)
    cand = np.tile(base, (40, 1))
    cand[7, 4] += 0.3
    with L.Points(xyz, [truth["x"], truth["y"], truth["z"]], "f32") as pts:
        pts.set_observed(uv)
        losses, amin = pts.eval_population(cand, L.LOSS_HUBER, 10.0)
    assert amin == 0 and losses[7] > losses[0]


def test_second_enqueue_before_wait_is_refused(L):
    truth, xyz, uv, base = _near_tie_case(L)
    cand = np.tile(base, (4, 1))
    with L.Points(xyz, [truth["x"], truth["y"], truth["z"]], "f32") as pts:
        pts.set_observed(uv)
        pts.eval_population_enqueue(cand, L.LOSS_HUBER, 10.0)
        with pytest.raises(L.AlprojHipError) as e:
            pts.eval_population_enqueue(cand, L.LOSS_HUBER, 10.0)
        assert e.value.code == -6
        losses, amin = pts.eval_population_wait(4)
        assert amin == 0 and np.all(losses == losses[0])
        pts.eval_population_enqueue(cand, L.LOSS_HUBER, 10.0)          # fine again after the wait
        pts.eval_population_wait(4)


# ------------------------------------------------------------------ full-size properties
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_dsm_10m_properties(L, prec):
    """BASELINE config 2/3 size (10 M vertices): (a) a strided sample of the projection equals
    the oracle on the same float32 vertices; (b) shard additivity: N * loss(all) ==
    N1 * loss(first part) + N2 * loss(rest) -- the identity the multi-GPU all-reduce relies on."""
    from alproj_amd import synthetic as syn
    n_side = syn.grid_side(10_000_000)
    s = syn.surface(n_side)
    xyz_l = syn.vert_to_xyz_local(s["vert"])
    truth = syn.local_params(syn.perturbed(syn.standoff_params(n_side)), s["offsets"])
    base = syn.local_params(syn.standoff_params(n_side), s["offsets"])
    N = len(xyz_l)
    origin = [base["x"], base["y"], base["z"]]
    pv = L.params_vector(truth)
    with L.Points(xyz_l, origin, prec) as pts:
        pts.project(pv)
        step = 9973
        cnt = (N - 1) // step
        u, v = pts.fetch_strided(0, step, cnt)
        sample = xyz_l[0:cnt * step:step].astype(np.float64)
        ref = orc.project_points(sample, truth)
        ok = well_conditioned(sample, truth) if prec == "f32" else np.ones(cnt, bool)
        got = np.stack([u, v], 1)
        if prec == "f64":
            np.testing.assert_allclose(got[ok], ref[ok], rtol=1e-9, atol=1e-9)
        else:
            assert_f32_close(got[ok], ref[ok], truth["w"])
        # observed = projection of the truth pose (fetched from the device) + 1 px noise
        uu, vv = pts.fetch()
        obs = np.stack([uu, vv], 1) + np.random.default_rng(1).normal(0, 1.0, (N, 2))
        obs[~np.isfinite(obs)] = 0.0
        pts.set_observed(obs)
        rng = np.random.default_rng(2)
        bounds = orc.bounds_to_array(base, syn.TARGETS_D9)
        # BASELINE config 3: 10 M vertices x population 256
        cand = _cand_matrix(L, base, syn.TARGETS_D9, bounds, rng.uniform(0.4, 0.6, (256, 9)))
        whole, amin_w = pts.eval_population(cand, L.LOSS_HUBER, 10.0)
        assert whole.shape == (256,) and amin_w == int(np.argmin(whole))
        # the only 10 M check against the oracle runs on the production grid: stripes of several rows (the V-wide and 2-wide
        # groups of pop_walk_stripe) and, in float32, every candidate tile in a column of its own
        _, stripes, ytiles = pts.eval_population_info()
        rows = -(-N // 256)
        assert -(-rows // stripes) >= 2, (stripes, ytiles)
        if prec == "f32":
            assert ytiles == 2, (stripes, ytiles)
        mean_d, amin_m = pts.eval_population(cand, L.LOSS_MEAN_DIST, 0.0)
        assert pts.eval_population_info()[1:] == (stripes, ytiles) and amin_m == int(np.argmin(mean_d))
        # four of the 256 candidates against the float64 oracle on all 10 M vertices, both losses
        xyz64 = xyz_l.astype(np.float64)
        for c in (0, 131, 255, amin_w):
            proj = orc.project_points(xyz64, orc.vector_to_params(cand[c]))
            ref_l = orc.huber(obs, proj, 10.0)
            assert whole[c] == pytest.approx(ref_l, rel=1e-9 if prec == "f64" else 1e-5), c
            ref_m = orc.mean_distance(obs, proj)
            assert mean_d[c] == pytest.approx(ref_m, rel=1e-9 if prec == "f64" else 1e-5), c
            del proj
        del xyz64
    cut = 3_777_777
    parts = []
    for a, b in ((0, cut), (cut, N)):
        with L.Points(xyz_l[a:b], origin, prec) as pp:
            pp.set_observed(obs[a:b])
            l, _ = pp.eval_population(cand[:8], L.LOSS_HUBER, 10.0)
            parts.append(l * (b - a))
    np.testing.assert_allclose((parts[0] + parts[1]) / N, whole[:8], rtol=1e-12 if prec == "f64" else 2e-6)


# ------------------------------------------------------------------ optimisers end to end
def test_cma_optimizer_recovers_pose(L):
    from alproj_amd import optimize as opt
    from alproj_amd import synthetic as syn
    truth = syn.truth_params(316)
    init = dict(truth, pan=truth["pan"] + 4, tilt=truth["tilt"] - 3, fov=truth["fov"] + 5,
                roll=truth["roll"] + 2)
    xyz = syn.gcp_points(1500, truth, seed=11)
    uv = orc.project_points(xyz, truth) + np.random.default_rng(11).normal(0, 1.0, (1500, 2))
    o = opt.CMAOptimizer(pd.DataFrame(xyz, columns=["x", "y", "z"]), pd.DataFrame(uv, columns=["u", "v"]), init)
    o.set_target(["fov", "pan", "tilt", "roll"])
    params, err = o.optimize(generation=80, sigma=0.3, population_size=32, f_scale=10.0, seed=5,
                             progress=False)
    assert set(params) == set(init)
    assert err < 1.6                                       # noise floor: E|N2(0,1)| = 1.2533 px
    assert abs(params["pan"] - truth["pan"]) < 0.05 and abs(params["fov"] - truth["fov"]) < 0.1
    # the reported error is the reference's "rmse" of the returned parameters
    ref = orc.mean_distance(uv, orc.project_points(xyz, params))
    assert err == pytest.approx(ref, rel=1e-5)


def test_cma_optimizer_default_is_float64_at_gcp_scale(L):
    """optimize(precision=None) on a g5-sized point set: the loss closure the optimiser itself builds holds a float64
    point set and reproduces the reference's float64 losses (g5) to 1e-10 (1e-8 for candidates next to a pole of the lens model); a set above F64_MAX_POINTS is float32."""
    from alproj_amd import optimize as opt
    g = load("g5_population.npz")
    init = orc.vector_to_params(g["params_init"])
    o = opt.CMAOptimizer(pd.DataFrame(g["xyz"], columns=["x", "y", "z"]), pd.DataFrame(g["uv_obs"], columns=["u", "v"]), init)
    for tag in ("d9", "d12", "d21"):
        o.set_target([str(t) for t in g[f"{tag}_targets"]])
        for key, fs in (("hub", 10.0), ("md", None)):
            f = o._loss_function(g[f"{tag}_bounds"], f_scale=fs)             # precision left to the default
            try:
                assert f.points.precision == L.ALP_F64
                losses, amin = f(g[f"{tag}_X"])
                # 1e-10 (observed: 1e-11) -- except for the candidates that have a pole of the rational lens model next to the
                # points (min |den| < 0.25, d21 only), where the reference's own value is rounding noise amplified by 1 / den^2:
                # 1e-8 there, as in test_population_golden
                ref = g[f"{tag}_{key}"]
                den = np.array([orc.conditioning(g["xyz"], orc.candidate_params(init, o.target_params, g[f"{tag}_bounds"], x))[1]
                                for x in g[f"{tag}_X"]])
                assert np.all(np.abs(losses - ref) <= np.where(den >= 0.25, 1e-10, 1e-8) * np.abs(ref)), np.abs(losses / ref - 1).max()
                assert amin == int(np.argmin(ref))
            finally:
                f.points.close()
    # the optimiser run itself, default precision: the reported error is the float64 mean distance of the returned pose
    o.set_target(["pan", "tilt"])
    params, err = o.optimize(generation=5, population_size=8, seed=2, progress=False)
    ref = orc.mean_distance(g["uv_obs"], orc.project_points(g["xyz"], params))
    assert err == pytest.approx(ref, rel=1e-9)
    # DSM-sized: float32 (the threshold lowered instead of allocating 4 M points)
    saved = opt.F64_MAX_POINTS
    opt.F64_MAX_POINTS = 100
    try:
        f = o._loss_function(g["d9_bounds"][:2], f_scale=10.0)
        assert f.points.precision == L.ALP_F32
        f.points.close()
    finally:
        opt.F64_MAX_POINTS = saved


def test_lsq_optimizer(L):
    from alproj_amd import optimize as opt
    from alproj_amd import synthetic as syn
    truth = syn.truth_params(316)
    init = dict(truth, pan=truth["pan"] + 1, tilt=truth["tilt"] - 1, k1=0.0, k2=0.0)
    xyz = syn.gcp_points(800, truth, seed=12)
    uv = orc.project_points(xyz, truth) + np.random.default_rng(12).normal(0, 0.5, (800, 2))
    o = opt.LsqOptimizer(pd.DataFrame(xyz, columns=["x", "y", "z"]), pd.DataFrame(uv, columns=["u", "v"]), init)
    o.set_target(["pan", "tilt", "k1", "k2"])
    params, err = o.optimize(method="trf")
    assert err < 0.8 and abs(params["pan"] - truth["pan"]) < 0.02
    with pytest.raises(ValueError):
        o.optimize(method="lm", bound_widths={"pan": 1})
    with pytest.raises(ValueError):
        o.optimize(method="lm", loss="huber")
