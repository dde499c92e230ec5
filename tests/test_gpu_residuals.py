"""The batched residual vectors (alp_residuals_batch, residual_batch_kernel: DESIGN section 4, K3) at every launch shape.

residuals_impl stages at most 256 MB of output per launch: a chunk of points for all B poses, copied back contiguously when
one chunk holds every point and with a pitched copy into out + 2 off otherwise.  Within a launch each lane holds RES_V = 3
points (768 per workgroup and pass) and the grid is capped at cu_count * 8 workgroups, beyond which it strides.  Every checked
call here follows a call with other poses and other observations that leaves at least as much staging behind, so a point or
a pose the kernel skips shows up as a mismatch.  References (tests/residual_cases.py):
  * row b of a batch is bit-equal to residuals(cand[b]), the B = 1 call -- which runs as one chunk with the contiguous copy up
    to 16 777 216 points, so this checks the pitched path against the contiguous one on every value;
  * float64 sets: every row is bit-equal to observed - project(pose) (alp_project + fetch), and within
    1e-9 of max(|ref|, w) of the oracle;
  * float32 sets: within 2e-5 of max(|ref|, w) of the float64 oracle evaluated on what the set stores, after the float32
    filters (residual_cases.compare_with_oracle)."""
import numpy as np
import pytest

from oracle import ref_numpy as orc
from tests import residual_cases as rc
from tests.popeval_cases import local_inputs_f32, oracle_r2, pole_a2_steps
from tests.test_gpu_points import well_conditioned

pytestmark = pytest.mark.gpu

PAN, FOV = orc.PARAM_KEYS.index("pan"), orc.PARAM_KEYS.index("fov")
SMALL_N = (1, 255, 256, 257, 767, 768, 769, 1023, 1025, 4099)
SMALL_B = (1, 2, 3, 22)
# worst |d| / max(|ref|, w) of the float32 sets measured on an MI355X, per test (the bound is rc.F32_TOL = 2e-5): shapes 1.6e-7,
# grid-stride passes 1.7e-7, chunks 1.7e-7, 10 M 1.1e-7, poles 1.2e-6, layouts 1.1e-7; float64 poles 1.3e-11 (rc.F64_TOL = 1e-9)


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


@pytest.fixture(scope="module")
def dsm10(L):
    return rc.dsm10_case(L)


def checked_batch(L, pts, cand, uv):
    """residuals_batch(cand) on a set whose observations are uv, after a call of the same size (B and n) with other poses and
    other observations; -> (rows, number of kernel launches of the checked call)"""
    other = cand.copy()
    other[:, PAN] += 7.0
    other[:, FOV] -= 3.0
    pts.set_observed(uv[::-1] + 400.0)
    pts.residuals_batch(other)                  # its rows go back to the result pool the checked call draws from
    pts.set_observed(uv)
    L.kernel_timing(True)
    try:
        L.kernel_time_ms()
        got = pts.residuals_batch(cand)
        _, sections = L.kernel_time_ms()
    finally:
        L.kernel_timing(False)
    assert got.shape == (len(cand), 2 * pts.n)
    return got, sections


def check_identities(L, pts, cand, uv, got, prec):
    """row b == residuals(cand[b]) bit for bit; float64: row b == observed - project(cand[b]) bit for bit"""
    for b, c in enumerate(cand):
        assert np.array_equal(got[b], pts.residuals(c), equal_nan=True), f"row {b} differs from the B = 1 call"
    if prec == "f64":
        for b, c in enumerate(cand):
            pts.project(c)
            u, v = pts.fetch()
            want = (uv - np.stack([u, v], 1)).ravel()
            assert np.array_equal(got[b], want, equal_nan=True), f"row {b} differs from observed - project()"


def run_case(L, pts, cand, uv, xyz, prec, o, rows=None, label=""):
    """one checked call, its launch count, its identities and its oracle comparison -> worst float32 ratio"""
    got, sections = checked_batch(L, pts, cand, uv)
    assert sections == rc.launches(pts.n, len(cand)), (label, sections)
    check_identities(L, pts, cand, uv, got, prec)
    return rc.compare_with_oracle(got, xyz, uv, cand, prec, o, rows, well_conditioned, label)[0]


# ------------------------------------------------------------------ 1. shapes and grid-stride passes
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("n", SMALL_N)
def test_shapes(L, n, prec):
    """n around the 256-lane and 768-point steps of a workgroup, B up to 22 (D = 21 finite differences around a lens pose,
    x, y, z among the targets, UTM coordinates with the origin at the camera): one launch each"""
    p = rc.lens_pose()
    cand = rc.fd_poses(p)
    xyz, uv = rc.gcp_case(n, p, seed=n)
    o = rc.camera(p)
    with L.Points(xyz, o, prec) as pts:
        pts.set_observed(uv)
        for B in SMALL_B:
            assert rc.launches(n, B) == 1
            run_case(L, pts, cand[:B], uv, xyz, prec, o, label=f"n {n}, B {B}")


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("dn", [-1, 0, 257], ids=["S-1", "S", "S+257"])
def test_grid_stride_passes(L, dn, prec):
    """n = S - 1, S, S + 257 with S = cu_count * 8 * 256 * RES_V, one full pass of the capped grid: the last lane of the
    pass, the pass exactly full, a second pass of 257 points.  B = 1 and 3 (from B = 11 a chunk holds fewer than S points)"""
    S = rc.stride_pass(L.device_info()["cu_count"])
    n = S + dn
    p = rc.lens_pose()
    cand = rc.fd_poses(p)
    xyz, uv = rc.gcp_case(n, p, seed=5)
    o = rc.camera(p)
    with L.Points(xyz, o, prec) as pts:
        pts.set_observed(uv)
        for B in (1, 3):
            assert rc.chunk_points(n, B) == n
            run_case(L, pts, cand[:B], uv, xyz, prec, o, label=f"S {dn:+d}, B {B}")


# ------------------------------------------------------------------ 2. several chunks
CHUNK22 = rc.chunk_points(1 << 40, 22)


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("B,n,chunks", [(22, 2 * CHUNK22, 2), (22, 3 * CHUNK22 + 517, 4), (rc.B_MAX, 3 * 4096 + 5, 4)],
                         ids=["B22-two-chunks-exact", "B22-ragged-last-chunk", "B4096"])
def test_several_chunks(L, B, n, chunks, prec):
    """chunk = max(1024, (256 MiB // (16 B)) // 1024 * 1024), capped at n: the launch count is the number of chunks, every row
    is bit-equal to the B = 1 call's (one contiguous chunk), and the oracle agrees on a strided sample and at every point
    within 3 of a chunk boundary and of n"""
    chunk = rc.chunk_points(n, B)
    assert rc.launches(n, B) == chunks and (B != rc.B_MAX or chunk == 4096)
    p = rc.lens_pose()
    cand = rc.spread_poses(p, B, seed=B)
    xyz, uv = rc.gcp_case(n, p, seed=n)
    o = rc.camera(p)
    with L.Points(xyz, o, prec) as pts:
        pts.set_observed(uv)
        run_case(L, pts, cand, uv, xyz, prec, o, rows=rc.sample_points(n, chunk, step=97), label=f"B {B}, n {n}")


@pytest.mark.parametrize("prec,B", [("f64", 2), ("f32", 2), ("f64", 22)], ids=["f64-B2", "f32-B2", "f64-B22-bench-f1"])
def test_ten_million_dsm_points(L, dsm10, prec, B):
    """bench.py's f1 shape: the 10 M DSM (a raster set) at B = 2 (2 chunks) and bench.py's own call, B = 22 (14 chunks)"""
    x10, uv, cand, b10 = dsm10
    n = len(x10)
    cand = cand if B == 22 else cand[[0, -1]]
    assert rc.launches(n, B) == {2: 2, 22: 14}[B]
    o = rc.camera(b10)
    with L.Points(x10, o, prec) as pts:
        assert pts.row_length() > 0
        pts.set_observed(uv)
        run_case(L, pts, cand, uv, x10, prec, o, rows=rc.sample_points(n, rc.chunk_points(n, B), step=9973),
                 label=f"10 M DSM, B {B}")


# ------------------------------------------------------------------ 4. poles
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_pole_of_one_lens_denominator(L, prec):
    """tests/test_gpu_points.py::test_pole_of_one_lens_denominator_is_an_infinite_loss's construction (k4 = -0.5: den_y =
    (1 + a2) - r2 / 2 is zero iff 1 + a2 == r2 / 2), its a2 steps as ONE batch.  On the pose that lands on the device's pole,
    at that point: the y residual is +-inf like the reference's division (optimize.py:112-116), never NaN, and the x residual
    finite.  float64: every row bit-equal to observed - project() at every point.  Against the oracle only where the oracle's
    own |den_x| and |den_y| are both >= 0.25 (every step pose puts other points near its pole too)."""
    from alproj_amd import synthetic as syn
    truth = dict(syn.truth_params(316), k4=-0.5, k5=0.0, k6=0.0)
    xyz = syn.gcp_points(400, truth, seed=31, margin=-0.25)
    r2 = oracle_r2(xyz, truth)
    i0 = int(np.argmin(np.abs(r2 - 1.4)))
    assert 1.2 < r2[i0] < 1.6
    keep = (np.abs(1 - r2 / 2) > 0.25) & (np.abs(1 + truth["a2"] - r2 / 2) > 0.25)
    keep[i0] = True
    i = int(np.count_nonzero(keep[:i0]))
    xyz = xyz[keep]
    assert len(xyz) > 100
    uv = orc.project_points(xyz, truth) + np.random.default_rng(31).normal(0, 1.0, (len(xyz), 2))
    assert np.isfinite(uv).all()
    o = rc.camera(truth)
    if prec == "f32":
        a2 = pole_a2_steps(oracle_r2(xyz, truth)[i], -0.5, prec)
    else:
        # r2 formed in the set's local frame, as the device forms it, is within a few ulps of the device's: a window of
        # +-2000 ulps instead of the 2^17 the absolute frame needs keeps the batch within B_MAX
        a2 = pole_a2_steps(oracle_r2(xyz - o, dict(truth, x=0.0, y=0.0, z=0.0))[i], -0.5, prec, W=2000)
    assert len(a2) <= rc.B_MAX
    cand = np.tile(orc.params_to_vector(truth), (len(a2), 1))
    cand[:, orc.PARAM_KEYS.index("a2")] = a2
    n = len(xyz)
    with L.Points(xyz, o, prec) as pts:
        pts.set_observed(uv)
        got, sections = checked_batch(L, pts, cand, uv)
        assert sections == 1
        res = got.reshape(len(cand), n, 2)
        hit = np.flatnonzero(~np.isfinite(res[:, i, 1]))
        assert len(hit) >= 1, "no pose landed on the device's pole: widen W"
        assert np.all(np.isinf(res[hit, i, 1])), res[hit, i]
        assert np.all(np.isfinite(res[hit, i, 0])), res[hit, i]
        check_identities(L, pts, cand, uv, got, prec)
    # the oracle where its own denominators are both >= 0.25
    w = truth["w"]
    xl, ul = (xyz, uv) if prec == "f64" else local_inputs_f32(xyz, uv, o)
    worst, least_kept = 0.0, n
    with np.errstate(all="ignore"):
        for b, c in enumerate(cand):
            q = orc.vector_to_params(c)
            r2b = oracle_r2(xyz, q)
            den = q["k4"] * r2b
            ok = (np.abs(1 + den) >= 0.25) & (np.abs(1 + q["a2"] + den) >= 0.25)
            if prec == "f32":
                ok &= well_conditioned(xyz, q, rc.F32_DEPTH_FRAC)
            least_kept = min(least_kept, int(ok.sum()))
            ref = orc.residual_vector(xl[ok], ul[ok], q if prec == "f64" else rc.local_pose(c, o)).reshape(-1, 2)
            r = rc.worst_ratio(res[b, ok], ref, w)
            assert r <= (rc.F64_TOL if prec == "f64" else rc.F32_TOL), (b, r)
            worst = max(worst, r)
    print(f"[residuals {prec}] poles: {len(hit)} of {len(cand)} poses on the device's pole; worst |d| / max(|ref|, w) = "
          f"{worst:.3e}; at least {least_kept} of {n} points compared on every pose")
    assert 2 * least_kept >= n


# ------------------------------------------------------------------ 5. layouts
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_raster_and_plane_layouts_give_the_same_bits(L, monkeypatch, prec):
    """40 rows of bench.py's 10 M DSM (as a rank of a sharded run generates them), the last row 123 points short, seen from the
    f1 leg's camera (a small DSM under standoff_params would lie wholly outside the frame): the set recognised as a raster
    (row_length() > 0) and the same set built with ALP_NO_POINTS_GRID (row_length() == 0) give the same residual rows and the
    same exact Jacobian, bit for bit; both against the oracle"""
    from alproj_amd import synthetic as syn
    side = syn.grid_side(10_000_000)
    s = syn.surface(side, rows=(1500, 1540))
    xyz = syn.vert_to_xyz_local(s["vert"])[: 40 * side - 123].astype(np.float64)
    base = syn.local_params(syn.standoff_params(side), s["offsets"])
    truth = syn.local_params(syn.perturbed(syn.standoff_params(side)), s["offsets"])
    cand = rc.fd_poses(truth)
    n = len(xyz)
    uv = orc.project_points(xyz, truth) + np.random.default_rng(300).normal(0, 1.0, (n, 2))
    o = rc.camera(base)
    out = {}
    for layout in ("raster", "planes"):
        if layout == "planes":
            monkeypatch.setenv("ALP_NO_POINTS_GRID", "1")
        else:
            monkeypatch.delenv("ALP_NO_POINTS_GRID", raising=False)
        with L.Points(xyz, o, prec) as pts:
            monkeypatch.delenv("ALP_NO_POINTS_GRID", raising=False)
            w = pts.row_length()
            assert (w == side) if layout == "raster" else (w == 0), (layout, w)
            pts.set_observed(uv)
            got, sections = checked_batch(L, pts, cand, uv)
            assert sections == 1
            check_identities(L, pts, cand, uv, got, prec)
            jac = pts.jacobian(cand[0], list(range(21)) + [23, 24])
        rc.compare_with_oracle(got, xyz, uv, cand, prec, o, None, well_conditioned, f"{layout} layout")
        out[layout] = (got, jac)
    assert np.array_equal(out["raster"][0], out["planes"][0], equal_nan=True)
    assert np.array_equal(out["raster"][1], out["planes"][1], equal_nan=True)


# ------------------------------------------------------------------ 6. refusals and empty sets
def test_refusals_and_empty_sets(L):
    p = rc.lens_pose()
    cand = rc.fd_poses(p)
    xyz, uv = rc.gcp_case(64, p, seed=64)
    o = rc.camera(p)
    with L.Points(xyz, o, "f64") as pts:
        with pytest.raises(L.AlprojHipError) as e:
            pts.residuals_batch(cand)                                   # no observations yet, as the B = 1 call
        with pytest.raises(L.AlprojHipError) as e1:
            pts.residuals(cand[0])
        assert e.value.code == e1.value.code
        pts.set_observed(uv)
        for B in (0, rc.B_MAX + 1):
            with pytest.raises(L.AlprojHipError):
                pts.residuals_batch(np.tile(cand[0], (B, 1)))
        assert pts.residuals_batch(np.tile(cand[0], (rc.B_MAX, 1))).shape == (rc.B_MAX, 128)
    for prec in ("f64", "f32"):
        with L.Points(np.zeros((0, 3)), o, prec) as empty:
            for observed in (False, True):
                if observed:
                    empty.set_observed(np.zeros((0, 2)))
                try:
                    single = ("ok", empty.residuals(cand[0]).shape)
                except L.AlprojHipError as err:
                    single = ("raised", err.code)
                try:
                    batch = ("ok", empty.residuals_batch(cand[:3]).shape)
                except L.AlprojHipError as err:
                    batch = ("raised", err.code)
                assert batch[0] == single[0], (prec, observed, single, batch)
                if single[0] == "ok":
                    assert single[1] == (0,) and batch[1] == (3, 0)
                else:
                    assert batch[1] == single[1]
