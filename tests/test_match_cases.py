"""CPU: the numpy restatement of the matcher core (tests/match_cases.py) against three loops in Python integers, and the
input checks of the Python layer that need no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_cases as mc  # noqa: E402


def test_restatement_equals_triple_loop():
    rng = np.random.default_rng(11)
    des1 = rng.integers(0, 256, size=(7, 5), dtype=np.uint8)
    des2 = rng.integers(0, 256, size=(9, 5), dtype=np.uint8)
    for ratio in (0.7, 0.5, 1.0):
        mc.assert_same(mc.restate(des1, des2, ratio), mc.restate_loops(des1, des2, ratio), f"ratio {ratio}")
    # the extremes of a byte, and float32 input holding the same integers
    des1[0], des2[3] = 0, 255
    mc.assert_same(mc.restate(des1, des2), mc.restate_loops(des1, des2), "extremes")
    mc.assert_same(mc.restate(des1.astype(np.float32), des2.astype(np.float32)), mc.restate_loops(des1, des2), "float32")


def test_restatement_puts_the_lower_index_first_on_a_tie():
    rng = np.random.default_rng(12)
    des2 = rng.integers(0, 256, size=(9, 5), dtype=np.uint8)
    des2[6] = des2[2]
    des2[8] = des2[2]
    des1 = np.stack([des2[2], des2[8], des2[4]])
    for fn in (mc.restate, mc.restate_two_pass):
        r = fn(des1, des2)
        assert r["idx"][:2].tolist() == [[2, 6], [2, 6]] and r["dist2"][:2].tolist() == [[0, 0], [0, 0]]
        assert r["idx"][2, 0] == 4 and not r["good"][0]          # 0 < 0.7 * 0 is false
        mc.assert_same(r, mc.restate_loops(des1, des2), fn.__name__)
    same = np.tile(des2[:1], (9, 1))
    for fn in (mc.restate, mc.restate_two_pass):
        assert fn(des1, same)["idx"].tolist() == [[0, 1]] * 3


def test_two_pass_form_equals_the_sort():
    des2 = mc.random_bytes(300, 3, 5) // 64          # four values per byte: many ties
    des1 = mc.random_bytes(200, 3, 6) // 64
    mc.assert_same(mc.restate_two_pass(des1, des2), mc.restate(des1, des2), "two-pass")


def test_builders():
    q = mc.unit_queries(64)
    assert q.shape == (64, 64) and q[5, 5] == 255 and q[5, 6] == 128 and q.dtype == np.uint8
    t = mc.asymmetric_train(32, 64)
    assert t[3, 2] == (21 + 26) % 251 and t[2, 3] != t[3, 2]
    n = mc.noisy_copies(mc.random_bytes(50, 61, 1), 40, 2)
    assert n.shape == (40, 61) and n.dtype == np.uint8


def test_python_layer_refuses_before_any_device_call(monkeypatch):
    """every refusal of knn_match / match_descriptors / match_keypoints is a ValueError raised with the library untouched"""
    from alproj_amd import _lib, gcp

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    monkeypatch.setattr(_lib, "init", no_device)
    u8 = mc.random_bytes(4, 8, 1)
    f32 = u8.astype(np.float32)
    bad = [
        (u8.tolist(), u8, "numpy arrays"), (u8, None, "numpy arrays"),
        (u8[0], u8, "two-dimensional"), (u8, u8[None], "two-dimensional"),
        (u8, f32, "both be uint8 or both float32"), (u8.astype(np.int8), u8.astype(np.int8), "both be uint8 or both float32"),
        (u8.astype(np.float64), u8.astype(np.float64), "both be uint8 or both float32"),
        (u8[:, ::2], u8[:, ::2], "C-contiguous"), (u8, np.asfortranarray(u8), "C-contiguous"),
        (u8, u8[:, :7].copy(), "lengths differ"),
        (np.zeros((4, 513), np.uint8), np.zeros((4, 513), np.uint8), "1..512"), (np.zeros((4, 0), np.uint8), np.zeros((4, 0), np.uint8), "1..512"),
        (u8, u8[:1], "at least 2 rows"), (u8, u8[:0], "at least 2 rows"),
    ]
    for a, b, text in bad:
        for call in (lambda: gcp.knn_match(a, b), lambda: gcp.match_descriptors(a, b), lambda: _lib.match_knn2(a, b)):
            with pytest.raises(ValueError, match=text):
                call()
    for ratio in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            gcp.match_descriptors(u8, u8, ratio)
        with pytest.raises(ValueError, match="finite"):
            gcp.match_keypoints(np.zeros((4, 2)), u8, np.zeros((4, 2)), u8, ratio)
    # match_keypoints: the reference's empty answers come first (gcp.py:52-53), then the shapes
    for args in ((np.zeros((4, 2)), None, np.zeros((4, 2)), u8), (np.zeros((4, 2)), u8, np.zeros((4, 2)), None),
                 (np.zeros((1, 2)), u8[:1], np.zeros((4, 2)), u8), (np.zeros((4, 2)), u8, np.zeros((1, 2)), u8[:1]),
                 (np.zeros((0, 2)), u8[:0], np.zeros((4, 2)), u8)):
        p1, p2 = gcp.match_keypoints(*args)
        assert p1.shape == p2.shape == (0, 2) and p1.dtype == p2.dtype == np.int32
    for args in ((np.zeros((4, 3)), u8, np.zeros((4, 2)), u8), (np.zeros((3, 2)), u8, np.zeros((4, 2)), u8),
                 (np.zeros((4, 2)), u8, np.zeros(4), u8), (np.zeros((4, 2)), u8.tolist(), np.zeros((4, 2)), u8)):
        with pytest.raises(ValueError, match="one row per descriptor"):
            gcp.match_keypoints(*args)
    with pytest.raises(ValueError, match="lengths differ"):
        gcp.match_keypoints(np.zeros((4, 2)), u8, np.zeros((4, 2)), u8[:, :7].copy())
    assert set(("knn_match", "match_descriptors", "match_keypoints")) <= set(gcp.__all__)
