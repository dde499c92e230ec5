"""CPU: the numpy restatement of the CMA-ES candidate draw (tests/cma_cases.py) that tests/test_gpu_cma_limits.py holds the
device to -- pinned to Random123's philox4x32-10 known-answer vectors, its draw procedure checked on cases whose answer is known
without it, and the restated grid rule of the batched population launch at the shapes the GPU tests rely on."""
import numpy as np
import pytest

from tests import cma_cases as cc

# Random123 kat_vectors, philox4x32 with 10 rounds: counter, key -> output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = cc.philox4x32_10(*[np.uint64(c) for c in ctr], np.uint64(key[0]), np.uint64(key[1]))
    assert [int(g) for g in got] == list(want)


def test_philox_is_elementwise_over_arrays():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2 ** 32, (4, 40), dtype=np.uint64)
    k0, k1 = np.uint64(0x9E3779B9), np.uint64(0x12345678)
    whole = cc.philox4x32_10(*c, k0, k1)
    for i in range(0, 40, 7):
        one = cc.philox4x32_10(*c[:, i], k0, k1)
        assert [int(w[i]) for w in whole] == [int(o) for o in one]


def test_uniforms_stay_in_the_unit_interval():
    lo, hi = np.uint64(0), np.uint64(0xFFFFFFFF)
    assert cc.uniform53(lo, lo) == 0.5 / 2 ** 53                   # never 0: log(u1) is finite
    assert cc.uniform53(hi, hi) == 1.0                              # 2^53 - 0.5 rounds to even: rad = 0, harmless
    assert cc.uniform53(np.uint64(1 << 31), lo) == 0.5 + 0.5 / 2 ** 53


def test_counter_layout():
    """the key is (seed low, seed high); the generation enters modulo 2^32; the deviates of D are a prefix of those of D + 1;
    an odd D drops the sine of its last pair"""
    D = 13
    t, c = np.arange(5)[None, :], np.arange(7)[:, None]
    base = cc.normals(D, t, c, 5, seed=(3 << 32) + 11)
    np.testing.assert_array_equal(base, cc.normals(D, t, c, (1 << 32) + 5, seed=(3 << 32) + 11))
    np.testing.assert_array_equal(base, cc.normals(D, t, c, 5, seed=(1 << 64) + (3 << 32) + 11))
    assert not np.array_equal(base, cc.normals(D, t, c, 5, seed=(4 << 32) + 11))
    assert not np.array_equal(base, cc.normals(D, t, c, 6, seed=(3 << 32) + 11))
    wide = cc.normals(32, t, c, 5, seed=(3 << 32) + 11)
    np.testing.assert_array_equal(base, wide[..., :D])
    # pair j >> 1 = 6: z[12] = rad cos(ang), z[13] = rad sin(ang) -- radius 1 apart from rounding
    w = cc.philox4x32_10(np.uint64(6), np.uint64(2), np.uint64(3), np.uint64(5), *cc.key_of((3 << 32) + 11))
    u1, u2 = cc.uniform53(w[0], w[1]), cc.uniform53(w[2], w[3])
    rad = np.sqrt(-2.0 * np.log(u1))
    assert base[3, 2, 12] == rad * np.cos(cc.TWO_PI * u2)
    assert wide[3, 2, 13] == rad * np.sin(cc.TWO_PI * u2)


def test_normals_are_standard():
    z = cc.normals(8, np.arange(50)[None, :], np.arange(2000)[:, None], 9, seed=77).reshape(-1, 8)
    n = len(z)
    assert np.abs(z.mean(0)).max() < 5 / np.sqrt(n)
    assert np.abs(z.var(0) - 1).max() < 5 * np.sqrt(2 / n)
    c = np.corrcoef(z.T) - np.eye(8)
    assert np.abs(c).max() < 5 / np.sqrt(n)                        # the cos / sin pair included


def test_sample_procedure():
    """unbounded: try 0; n_max = 0: try 0 clipped; otherwise the first feasible try, every earlier one infeasible; none
    feasible: try n_max clipped"""
    rng = np.random.default_rng(4)
    D, P = 5, 200
    BD = np.linalg.qr(rng.normal(size=(D, D)))[0] * rng.uniform(0.5, 1.5, D)
    mean, sigma, seed, gen = rng.uniform(-1, 1, D), 0.8, (7 << 32) + 1, 12
    x, t, sc, near = cc.sample(mean, sigma, BD, None, P, 100, seed, gen)
    z0 = cc.normals(D, 0, np.arange(P), gen, seed)
    assert (t == 0).all() and not near.any()
    close = dict(rtol=0, atol=1e-14)                                # (matrix products of other shapes round otherwise)
    np.testing.assert_allclose(x, mean + sigma * (z0 @ BD.T), **close)
    half = 1.2 * sigma * np.sqrt((BD ** 2).sum(1))
    box = np.column_stack([mean - half, mean + half])
    x, t, _, _ = cc.sample(mean, sigma, BD, box, P, 0, seed, gen)
    assert (t == 0).all()
    np.testing.assert_allclose(x, np.clip(mean + sigma * (z0 @ BD.T), box[:, 0], box[:, 1]), **close)
    for n_max in (1, 17, 40):
        x, t, _, _ = cc.sample(mean, sigma, BD, box, P, n_max, seed, gen)
        assert (t <= n_max).all() and (t > 0).any()
        for i in range(0, P, 9):
            zs = cc.normals(D, np.arange(t[i] + 1), i, gen, seed)
            xs = mean + sigma * (zs @ BD.T)
            inside = np.all((xs >= box[:, 0]) & (xs <= box[:, 1]), axis=1)
            assert not inside[:min(t[i], n_max)].any()
            if t[i] < n_max:
                assert inside[t[i]]
                np.testing.assert_allclose(x[i], xs[t[i]], **close)
            else:
                np.testing.assert_allclose(x[i], np.clip(xs[n_max], box[:, 0], box[:, 1]), **close)


def test_batched_grid_rule_at_the_tested_shapes():
    """the readings the GPU tests rely on (256 CUs): the float32 general variant on 10 M points with K P = 65536 gets 2171
    stripes from the unbatched rule, capped to 256; the 1127-point GCP set with K P = 250 gets 5 x 2; a GCP-sized set gets tile
    columns from the fill rule; the partial sums never pass 128 MB"""
    assert cc.batched_grid(10_000_000, 65536, "f32", False, 256) == (256, 512)
    assert cc.batched_grid(1127, 250, "f64", True, 256) == (5, 2)
    assert cc.batched_grid(1_000_000, 65536, "f32", False, 256) == (256, 512)
    assert cc.batched_grid(1_000_000, 32768, "f64", True, 256) == (512, 2)
    assert cc.batched_grid(67 * 256 - 37, 4096, "f64", False, 256) == (67, 16)
    for n in (1, 300, 1127, 67 * 256 - 37, 10 ** 5, 10 ** 6, 10 ** 7, 10 ** 8):
        for R in (2, 250, 2048, 4096, 32768, 65536):
            for prec in ("f32", "f64"):
                for lf in (False, True):
                    s, c = cc.batched_grid(n, R, prec, lf, 256)
                    assert 1 <= s <= -(-n // 256) and 1 <= c <= -(-R // 128)
                    assert s * R * 8 <= cc.BATCHED_PARTIALS_BYTES
