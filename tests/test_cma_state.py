"""cma.CMA.get_state / set_state (the state the device loop of the generation takes and gives back): the round trip is
exact, clears the cached eigendecomposition, and a tell after it continues exactly as without it."""
import numpy as np

from alproj_amd.cma import CMA


def _advanced(seed, D=9, P=50, gens=5):
    opt = CMA(mean=np.full(D, 0.5), sigma=0.3, bounds=np.column_stack([np.zeros(D), np.ones(D)]), population_size=P,
              n_max_resampling=100, seed=seed)
    rng = np.random.default_rng(seed)
    for _ in range(gens):
        X = opt.ask_population()
        opt.tell_population(X, rng.random(P) + np.sum((X - 0.3) ** 2, axis=1))
    return opt


def test_round_trip_is_exact():
    a = _advanced(1)
    st = a.get_state()
    assert set(st) == {"mean", "sigma", "C", "p_sigma", "pc", "g"}
    b = _advanced(2)
    b.set_state(st)
    back = b.get_state()
    for k in ("mean", "C", "p_sigma", "pc"):
        np.testing.assert_array_equal(back[k], st[k])
    assert back["sigma"] == st["sigma"] and back["g"] == st["g"] == 5
    st["mean"][0] = 123.0                          # copies, not views
    assert a.get_state()["mean"][0] != 123.0


def test_set_state_clears_the_eigendecomposition():
    a = _advanced(3)
    a._eigen()
    assert a._B is not None
    a.set_state(a.get_state())
    assert a._B is None and a._D is None


def test_tell_continues_identically_after_the_round_trip():
    a, b = _advanced(4), _advanced(5)
    b._eigen()                                     # b's own cached eigendecomposition: set_state must drop it
    b.set_state(a.get_state())
    P, D = a.population_size, a.dim
    X = np.random.default_rng(9).random((P, D))
    losses = np.random.default_rng(10).random(P)
    losses[[3, 7]] = np.nan
    losses[11] = losses[12]
    oa = a.tell_population(X, losses)
    ob = b.tell_population(X, losses)
    np.testing.assert_array_equal(oa, ob)
    sa, sb = a.get_state(), b.get_state()
    for k in ("mean", "C", "p_sigma", "pc"):
        np.testing.assert_array_equal(sa[k], sb[k])
    assert sa["sigma"] == sb["sigma"] and sa["g"] == sb["g"]
