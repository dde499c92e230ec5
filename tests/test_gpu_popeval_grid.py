"""The population kernel on every launch grid: popeval_kernel walks a stripe of rows_per = ceil(rows / stripes) rows in unmasked
groups of V rows, the rows those leave over two at a time, and masked single rows (pop_walk_stripe), and takes candidate tiles
c0, c0 + gridDim.y * TC, ... (alproj_amd/csrc/alp_point_kernels.h).  The shipped grid gives every small point set one row per
stripe, so only the masked single rows run there; here the grid is forced through ALP_POP_GRID="stripes,tile_columns" over a
sweep that puts every group width, every leftover and empty trailing stripes in front of the float64 oracle, and checks what
IS invariant: the same bits for the same call, for a permuted population and whatever the other candidates are, and every
point counted exactly once."""
import numpy as np
import pytest

from oracle import ref_numpy as orc
from tests import popeval_cases as pc
from tests.test_gpu_points import f32_loss_tolerance

pytestmark = pytest.mark.gpu

GRIDS = pc.STRIPES + pc.EMPTY_STRIPES
# (P, tile columns): one candidate, one tile, one tile full, one candidate over, and two full tiles plus a lone candidate in 1, 2
# and 3 columns (with 2, column 0 takes tiles 0 and 2)
P_COLS = ((1, 1), (127, 1), (128, 1), (129, 1), (129, 2), (257, 1), (257, 2), (257, 3))
# Bounds set from what the MI355X measured on these sets (the test prints it), with margin:
# float64 against the oracle: 8.8e-12 (general, lens-free), 4.2e-11 (shared-pose) -> 1e-10
F64_RTOL = 1e-10
# float32 against the oracle evaluated on the float32-rounded local inputs (what the handle stores): 3.9e-7 general, 6.9e-7
# lens-free, 6.6e-6 shared-pose (its losses are the smallest, near the 1 px noise, and its float32 pose records' rounding is
# the same in absolute terms) -- never looser than 1e-5
F32_STORED_INPUT_RTOL = {"general": 2e-6, "lens_free": 3e-6, "shared_pose": 1e-5}
# across the 54 forced grids of one population: float64 5.3e-16 (the order of the float64 additions), float32 3.3e-8 (which
# rows go through which group width)
CROSS_GRID_RTOL = {"f64": 1e-14, "f32": 2e-7}
# float32 shared-pose candidates of the 4097-candidate population on 5 rows come closer to the truth than those of the 257 on
# 67 rows: 1.13e-5 measured for one whose Huber loss is 29 (the noise floor is ~26), the same on every grid -- the float32
# floor of the pose records, not the walk; the other variants keep f32_loss_tolerance's 1e-5
F32_SHARED_POSE_FEW_ROWS_RTOL = 2e-5


@pytest.fixture(scope="module")
def L():
    from alproj_amd import _lib
    _lib.init(0)
    return _lib


@pytest.fixture(scope="module")
def cases(L):
    """the 67-row point set, one population of 257 candidates per variant and their oracle losses, computed once"""
    xyz, uv = pc.point_set()
    o = pc.origin()
    xyz32, uv32 = pc.local_inputs_f32(xyz, uv, o)
    pops = {v: pc.population(v, 257) for v in pc.VARIANTS}
    return dict(xyz=xyz, uv=uv, o=o, pops=pops,
                ref={v: pc.oracle_losses(xyz, uv, pops[v]) for v in pc.VARIANTS},
                ref32={v: pc.oracle_losses(xyz32, uv32, pops[v], o) for v in pc.VARIANTS},
                tol32={v: f32_loss_tolerance(xyz, pops[v]) for v in pc.VARIANTS})


def forced(pts, monkeypatch, stripes, cols, cand, kind, fs, want_argmin=True):
    """one call on the grid stripes x cols; the launch must report that grid (stripes clamped to the rows), so that a change
    which drops the hook fails here instead of testing the default grid"""
    monkeypatch.setenv("ALP_POP_GRID", f"{stripes},{cols}")
    losses, amin = pts.eval_population(cand, kind, fs, want_argmin=want_argmin)
    variant, s, c = pts.eval_population_info()
    rows = -(-pts.n // 256)
    assert (s, c) == (min(stripes, rows), cols), (stripes, cols, s, c)
    return losses, amin, variant


def expected_variant(variant, P):
    return "general" if variant == "shared_pose" and P == 1 else variant


def bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def rel(a, b):
    return np.abs(a - b) / np.abs(b)


# ------------------------------------------------------------------ 1 + 4: oracle parity and cross-grid agreement
@pytest.mark.parametrize("loss", list(pc.LOSSES))
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_oracle_parity_on_every_grid(L, cases, variant, prec, loss, monkeypatch):
    kind, fs = pc.LOSSES[loss]
    cand = cases["pops"][variant]
    ref = cases["ref"][variant][loss]
    ref32 = cases["ref32"][variant][loss]
    tol = np.full(len(cand), F64_RTOL) if prec == "f64" else cases["tol32"][variant]
    worst, worst32 = 0.0, 0.0
    across = {}
    with L.Points(cases["xyz"], cases["o"], prec) as pts:
        pts.set_observed(cases["uv"])
        for s in GRIDS:
            for P, cols in P_COLS:
                got, amin, var = forced(pts, monkeypatch, s, cols, cand[:P], kind, fs)
                assert var == expected_variant(variant, P)
                bad = np.abs(got - ref[:P]) > tol[:P] * np.abs(ref[:P])
                assert not bad.any(), (s, cols, P, np.flatnonzero(bad)[:8], rel(got, ref[:P]).max())
                assert amin == orc.first_argmin(ref[:P]), (s, cols, P)
                worst = max(worst, rel(got, ref[:P]).max())
                if prec == "f32":
                    d32 = rel(got, ref32[:P]).max()
                    assert d32 <= F32_STORED_INPUT_RTOL[variant], (s, cols, P, d32)
                    worst32 = max(worst32, d32)
                if P == 257:      # losses only (no float32 argmin confirmation replacing any): the cross-grid comparison
                    across[(s, cols)], _, _ = forced(pts, monkeypatch, s, cols, cand, kind, fs, want_argmin=False)
    first = across[(GRIDS[0], 1)]
    spread = max(rel(v, first).max() for v in across.values())
    print(f"[popeval grid] {variant} {prec} {loss}: max rel. deviation from the float64 oracle {worst:.3e}"
          + (f", from the oracle on the stored float32 inputs {worst32:.3e}" if prec == "f32" else "")
          + f"; across {len(across)} grids {spread:.3e}")
    assert spread <= CROSS_GRID_RTOL[prec], spread


# ------------------------------------------------------------------ 2: every point counted once
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_every_point_counted_once_in_every_tile(L, cases, variant, prec, monkeypatch):
    """Every candidate is the pose that produced the observations; a marked point's observation is off by d_k pixels (float64:
    d_k = 4^k, ten marks per call, so that loss * n spells out in base 4 how often each marked point was counted; float32, whose
    residual noise sums to some px: one mark of 2^14 px per call).  Mean distance, no argmin confirmation."""
    t = pc.truth(variant)
    xyz = cases["xyz"]
    exact = orc.project_points(xyz, t)
    P = 257
    cand = np.tile(L.params_vector(t), (P, 1))
    if variant == "general":          # identical candidates with a lens are the shared-pose variant: one other pan
        cand = np.vstack([cand, cand[:1]])
        cand[-1, L.PARAM_KEYS.index("pan")] += 0.5
    V = pc.GROUP_ROWS[(variant, prec)]
    kind, fs = pc.LOSSES["mean_dist"]
    n = len(xyz)
    per_call = 10 if prec == "f64" else 1
    calls = 0
    with L.Points(xyz, cases["o"], prec) as pts:
        for gi, s in enumerate(GRIDS):
            cols = 1 + gi % 3
            marks = pc.mark_positions(s, V)
            for k0 in range(0, len(marks), per_call):
                chunk = marks[k0:k0 + per_call]
                d = 4.0 ** np.arange(len(chunk)) if prec == "f64" else np.array([2.0 ** 14])
                uv = exact.copy()
                uv[chunk, 0] += d
                pts.set_observed(uv)
                got, _, var = forced(pts, monkeypatch, s, cols, cand, kind, fs, want_argmin=False)
                assert var == variant
                truth_l = got[:P]
                assert np.array_equal(bits(truth_l), bits(np.full(P, truth_l[0]))), (s, cols)   # identical candidates
                total = truth_l[0] * n
                if prec == "f64":
                    counts = pc.mark_counts(total, len(chunk))
                    assert counts == [1] * len(chunk), (s, cols, chunk, counts, total)
                else:
                    assert pc.mark_counts(total, 1, d[0]) == [1], (s, cols, chunk, total / d[0])
                calls += 1
    assert calls > len(GRIDS)


# ------------------------------------------------------------------ 3: bitwise invariants at a fixed grid
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_bitwise_invariants_at_a_fixed_grid(L, cases, variant, prec, monkeypatch):
    """the same call twice: the same bits; a permuted population (across tile boundaries): the permuted bits; other candidates
    changed (same P, same variant): the bits of the unchanged ones"""
    cand = cases["pops"][variant]
    P = len(cand)
    rng = np.random.default_rng(7)
    other = pc.population(variant, 60, seed=99)
    with L.Points(cases["xyz"], cases["o"], prec) as pts:
        pts.set_observed(cases["uv"])
        for s, cols in ((5, 2), (12, 3), (60, 1), (2, 1)):
            for loss, (kind, fs) in pc.LOSSES.items():
                a, _, var = forced(pts, monkeypatch, s, cols, cand, kind, fs, want_argmin=False)
                assert var == variant
                b, _, _ = forced(pts, monkeypatch, s, cols, cand, kind, fs, want_argmin=False)
                assert np.array_equal(bits(a), bits(b)), (s, cols, loss)
                perm = rng.permutation(P)
                c, _, var = forced(pts, monkeypatch, s, cols, cand[perm], kind, fs, want_argmin=False)
                assert var == variant and np.array_equal(bits(c), bits(a[perm])), (s, cols, loss)
                changed = rng.choice(P, len(other), replace=False)
                mixed = cand.copy()
                mixed[changed] = other
                m, _, var = forced(pts, monkeypatch, s, cols, mixed, kind, fs, want_argmin=False)
                keep = np.setdiff1d(np.arange(P), changed)
                assert var == variant and np.array_equal(bits(m[keep]), bits(a[keep])), (s, cols, loss)


# ------------------------------------------------------------------ 5: the second walk over multi-row stripes
SECOND_WALK_STRIPES = 3                # rows_per 23: V-wide groups, 2-wide leftovers and a single row in every variant
POISON_SLOTS = (0, 63, 64, 127, 128, 256)
POLE_K4 = -0.125                        # den_y = (1 + a2) - r2 / 8: zero only at a vertex far outside the frame (r2 > 4)


def poison_positions(V, n=pc.N):
    """(NaN vertices, pole vertices): a V-wide group's last row (lane j = V - 1), a 2-wide group, the ragged last row"""
    rp = pc.rows_per(SECOND_WALK_STRIPES)
    narrow = V * (rp // V)                # first row of the first 2-wide group of a stripe
    nan_at = [(rp + V - 1) * 256 + 63, (narrow + 1) * 256 + 128, n - 1]
    pole_at = [(2 * rp + 2 * V - 1) * 256 + 255, (rp + narrow) * 256, n - 2]
    return nan_at, pole_at


def second_walk_set(V):
    """the 67-row set with vertices that poison chosen candidates: NaN -- a vertex at integer metres east of the origin is the
    camera of a candidate looking along a coordinate axis (R = I: the camera-frame coordinates cancel to exactly 0 in the
    device's float32 and float64 arithmetic and in the oracle's); pole -- out-of-frame vertices at r2 ~ 4.5 of the truth pose"""
    xyz, _ = pc.point_set()
    o = pc.origin()
    t = pc.truth("general")
    nan_at, pole_at = poison_positions(V)
    nan_cam = [o + np.array([kx, 0.0, 0.0]) for kx in (8.0, 16.0, 32.0)]
    far = syn_far_points(t)
    r2 = pc.oracle_r2(far, t)
    pick = np.flatnonzero((r2 > 4.2) & (r2 < 5.0))[:3]
    assert len(pick) == 3
    for i, c in zip(nan_at, nan_cam):
        xyz[i] = c
    for i, j in zip(pole_at, pick):
        xyz[i] = far[j]
    uv = orc.project_points(xyz, t) + np.random.default_rng(3).normal(0, 1.0, (len(xyz), 2))
    assert np.isfinite(uv).all()
    nan_cands = []
    for c in nan_cam:
        p = dict(pc.truth("general"), x=c[0], y=c[1], z=c[2], pan=0.0, tilt=-90.0, roll=0.0)
        nan_cands.append(p)
    return xyz, uv, o, nan_at, pole_at, nan_cands


def syn_far_points(t):
    from alproj_amd import synthetic as syn
    return syn.gcp_points(400, t, seed=77, margin=-0.8)


def pole_candidates(L, pts, monkeypatch, xyz, o, pole_at, prec, variant, kind, fs):
    """for each pole vertex: one candidate the device puts exactly on it (found by a sweep of 1 + a2 ulp by ulp through r2 / 8
    on the same set, grid and variant) and the oracle's own pole candidate (a2 = r2_oracle / 8 - 1)"""
    t = dict(pc.truth("general"), k4=POLE_K4, k5=0.0, k6=0.0)
    xyz_l = np.asarray(xyz, np.float64) - o
    if prec == "f32":
        xyz_l = xyz_l.astype(np.float32).astype(np.float64)
    t_l = dict(t, x=t["x"] - o[0], y=t["y"] - o[1], z=t["z"] - o[2])
    dev, ora = [], []
    ia2 = L.PARAM_KEYS.index("a2")
    r2_local, r2_oracle = pc.oracle_r2(xyz_l, t_l), pc.oracle_r2(xyz, t)      # (whole sets: numpy's rounding depends on the shape)
    for i in pole_at:
        r2_dev_guess = r2_local[i]
        a2 = pc.pole_a2_steps(r2_dev_guess, POLE_K4, prec, W=1 << 14 if prec == "f64" else 400)
        sweep = np.tile(L.params_vector(t), (len(a2), 1))
        sweep[:, ia2] = a2
        if variant == "general":
            sweep = np.vstack([sweep, L.params_vector(dict(t, pan=t["pan"] + 0.5))])
        got, _, var = forced(pts, monkeypatch, SECOND_WALK_STRIPES, 1, sweep, kind, fs, want_argmin=False)
        assert var == variant
        hit = np.flatnonzero(~np.isfinite(got[:len(a2)]))
        assert len(hit) >= 1, "no candidate landed on the device's pole"
        dev.append(sweep[hit[0]].copy())
        o_pole = sweep[hit[0]].copy()
        o_pole[ia2] = r2_oracle[i] * -POLE_K4 - 1.0
        ora.append(o_pole)
    return dev, ora


@pytest.mark.parametrize("variant,prec", [("general", "f64"), ("shared_pose", "f64"), ("lens_free", "f64"), ("lens_free", "f32"),
                                          ("general", "f32")])
def test_second_walk_on_multi_row_stripes(L, cases, variant, prec, monkeypatch):
    """Candidates poisoned at tile slots 0, 63, 64, 127 (the second walk's redo_hi half), 128 and 256 (the lone candidate of the
    last tile) by vertices in a V-wide group (lane j = V - 1), a 2-wide group and the ragged row: the non-finite pattern is the
    oracle's (+inf stays +inf; float32 general: non-finite, NaN allowed for +inf -- include/alproj_hip.h), every clean candidate
    has the bits of the same call with clean candidates in place of the poisoned ones, and NaN never wins the argmin."""
    V = pc.GROUP_ROWS[(variant, prec)]
    xyz, uv, o, nan_at, pole_at, nan_cands = second_walk_set(V)
    kind, fs = pc.LOSSES["mean_dist"] if variant != "shared_pose" else pc.LOSSES["huber"]
    clean = cases["pops"][variant].copy()
    P = len(clean)
    with L.Points(xyz, o, prec) as pts:
        pts.set_observed(uv)
        poison, oracle_poison = [], []
        if variant == "lens_free":
            nan_lf = [L.params_vector(dict(p, **{k: 0.0 for k in pc.LENS_KEYS})) for p in nan_cands]
            inf_lf = []
            for dx in (1.0, 2.0, 3.0):
                p = dict(pc.truth("lens_free"), a2=-1.0)
                p["x"] += dx
                inf_lf.append(L.params_vector(p))
            poison = [nan_lf[0], inf_lf[0], nan_lf[1], inf_lf[1], inf_lf[2], nan_lf[2]]
            oracle_poison = poison
        else:
            dev, ora = pole_candidates(L, pts, monkeypatch, xyz, o, pole_at, prec, variant, kind, fs)
            if variant == "shared_pose":
                poison, oracle_poison = dev + dev, ora + ora
            else:
                nan_g = [L.params_vector(p) for p in nan_cands]
                poison = [nan_g[0], dev[0], nan_g[1], dev[1], dev[2], nan_g[2]]
                oracle_poison = [nan_g[0], ora[0], nan_g[1], ora[1], ora[2], nan_g[2]]
        cand = clean.copy()
        cand[list(POISON_SLOTS)] = poison
        got, amin, var = forced(pts, monkeypatch, SECOND_WALK_STRIPES, 2, cand, kind, fs)
        assert var == variant
        ref_clean, _, var = forced(pts, monkeypatch, SECOND_WALK_STRIPES, 2, clean, kind, fs, want_argmin=False)
        assert var == variant
    with np.errstate(all="ignore"):
        exp = np.array([orc.loss_of(xyz, uv, orc.vector_to_params(c), kind, fs) for c in oracle_poison])
    assert np.all(~np.isfinite(exp)) and np.isnan(exp).any() == (variant != "shared_pose")
    slots = np.array(POISON_SLOTS)
    g = got[slots]
    if prec == "f64" or variant == "lens_free":
        assert np.array_equal(np.isnan(g), np.isnan(exp)) and np.array_equal(np.isposinf(g), np.isposinf(exp)), (g, exp)
    else:
        assert np.all(~np.isfinite(g)) and np.all(np.isnan(g[np.isnan(exp)])), (g, exp)
    keep = np.setdiff1d(np.arange(P), slots)
    assert np.isfinite(got[keep]).all()
    assert np.array_equal(bits(got[keep]), bits(ref_clean[keep]))
    assert amin not in POISON_SLOTS and got[amin] <= got[keep].min() * (1 + 1e-4)


# ------------------------------------------------------------------ a large population on few rows
FEW_ROWS_N = 5 * 256 - 37


@pytest.fixture(scope="module")
def few_rows(L):
    xyz, uv = pc.point_set(FEW_ROWS_N, seed=5)
    pops = {v: pc.population(v, 4097, seed=11) for v in pc.VARIANTS}
    tol32 = {v: f32_loss_tolerance(xyz, pops[v]) for v in pc.VARIANTS}
    tol32["shared_pose"] = np.maximum(tol32["shared_pose"], F32_SHARED_POSE_FEW_ROWS_RTOL)
    return dict(xyz=xyz, uv=uv, o=pc.origin(), pops=pops, ref={v: pc.oracle_losses(xyz, uv, pops[v]) for v in pc.VARIANTS},
                tol32=tol32)


def check_against(got, ref, tol, label):
    bad = np.abs(got - ref) > tol * np.abs(ref)
    assert not bad.any(), (label, np.flatnonzero(bad)[:8], rel(got, ref).max())


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_large_population_on_few_rows(L, few_rows, variant, prec, monkeypatch):
    """P = 4097 (33 tiles, the last of one candidate) on 5 rows, in 1 to 33 tile columns -- fewer columns than tiles walk the
    c0 += gridDim.y * TC loop many times"""
    cand = few_rows["pops"][variant]
    with L.Points(few_rows["xyz"], few_rows["o"], prec) as pts:
        pts.set_observed(few_rows["uv"])
        for s, cols in ((1, 1), (2, 2), (3, 5), (5, 33), (1000, 32), (4, 3)):
            for loss, (kind, fs) in pc.LOSSES.items():
                ref = few_rows["ref"][variant][loss]
                tol = np.full(len(ref), F64_RTOL) if prec == "f64" else few_rows["tol32"][variant]
                got, amin, var = forced(pts, monkeypatch, s, cols, cand, kind, fs)
                assert var == variant
                check_against(got, ref, tol, (s, cols, loss))
                assert amin == orc.first_argmin(ref), (s, cols, loss)


# ------------------------------------------------------------------ 6: one handle, many calls
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_one_handle_many_calls(L, few_rows, prec, monkeypatch):
    """one Points handle: P = 1, 300, 129, 4097, 7 with the variant switching and stripes x P growing and shrinking -- the
    candidate records (the lens-free ones live at offset cand_cap) and the partial sums are regrown in ensure_pop_scratch"""
    seq = (("lens_free", 1, 5, 1), ("general", 300, 5, 3), ("shared_pose", 129, 2, 2), ("lens_free", 4097, 5, 7),
           ("general", 7, 1, 1), ("lens_free", 300, 3, 2), ("shared_pose", 4097, 4, 1))
    with L.Points(few_rows["xyz"], few_rows["o"], prec) as pts:
        pts.set_observed(few_rows["uv"])
        for variant, P, s, cols in seq:
            cand = few_rows["pops"][variant][:P]
            for loss, (kind, fs) in pc.LOSSES.items():
                ref = few_rows["ref"][variant][loss][:P]
                tol = np.full(P, F64_RTOL) if prec == "f64" else few_rows["tol32"][variant][:P]
                got, amin, var = forced(pts, monkeypatch, s, cols, cand, kind, fs)
                assert var == expected_variant(variant, P)
                check_against(got, ref, tol, (variant, P, s, cols, loss))
                assert amin == orc.first_argmin(ref)


# ------------------------------------------------------------------ the shipped rule
def test_shipped_rule_uses_multi_row_stripes_and_every_tile_column(L, monkeypatch):
    """unforced: float32, general variant, P = 2048 on ~600 k points -- the rule itself picks stripes of several rows and one
    column per candidate tile; 64 candidates (first, last, tile edges, the argmin and random ones) against the oracle"""
    monkeypatch.delenv("ALP_POP_GRID", raising=False)
    xyz, uv = pc.point_set(600_000 - 99, seed=13)
    cand = pc.population("general", 2048, seed=17)
    with L.Points(xyz, pc.origin(), "f32") as pts:
        pts.set_observed(uv)
        for loss, (kind, fs) in pc.LOSSES.items():
            got, amin = pts.eval_population(cand, kind, fs)
            variant, stripes, ytiles = pts.eval_population_info()
            rows = -(-len(xyz) // 256)
            assert variant == "general" and ytiles == 2048 // pc.TC and -(-rows // stripes) >= 2, (stripes, ytiles)
            rng = np.random.default_rng(3)
            edges = [0, 1, 127, 128, 255, 256, 1023, 1024, 1919, 1920, 2047, amin]
            sel = np.unique(np.concatenate([edges, rng.choice(2048, 64 - len(edges), replace=False)]))
            ref = pc.oracle_losses(xyz, uv, cand[sel])[loss]
            check_against(got[sel], ref, f32_loss_tolerance(xyz, cand[sel]), loss)
