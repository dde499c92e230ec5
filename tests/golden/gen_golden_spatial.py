#!/usr/bin/env python3
"""Golden vectors for filter_spatial FROM THE REFERENCE ITSELF.

Run only in the build container (reference checkout at /root/reference):

    python tests/golden/gen_golden_spatial.py

Loads the reference's ``src/alproj/gcp.py`` by file path (``cv2``, which its module header imports and
``_filter_spatial`` does not touch, is registered as an empty placeholder), runs ``_filter_spatial``
(gcp.py:282-357) on the seeded point sets below and stores inputs + masks in ``g21_filter_spatial.npz``.
Only data is written.  Case k is stored as pts<k>, args<k> = (grid_size, width, height, random_state or -1),
sel<k> (the selection) and mask<k>.
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference/src/alproj/gcp.py"
OUT = os.path.dirname(os.path.abspath(__file__))


def load_reference():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("alproj_ref_gcp", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def point_sets():
    rng = np.random.default_rng(20261020)
    w, h = 1504, 1000
    sets = {}
    # integer pixels as match_keypoints returns them, crowded so that cells hold several points; duplicates
    p = np.stack([rng.integers(0, w, 700), rng.integers(0, h, 700)], axis=1).astype("int32")
    p[:30] = p[30:60]
    sets["int"] = p
    # sub-pixel points, some exactly on cell borders of every grid below, one outside the image on each side
    f = np.stack([rng.uniform(0, w, 600), rng.uniform(0, h, 600)], axis=1)
    f[:40] = np.round(f[:40] / 50.0) * 50.0
    f[40] = (-3.5, 20.0)
    f[41] = (w + 7.25, 30.0)
    f[42] = (100.0, -0.5)
    f[43] = (200.0, h + 64.0)
    sets["float"] = f
    # equal distances to a cell centre: the four corners of squares about the centres of 100-pixel cells (the last square
    # has side 0: four copies of the centre), and five points at distance 5 from the centre (650, 50)
    c = []
    for cx, cy, r in ((150.0, 250.0, 7.0), (350.0, 50.0, 21.5), (450.0, 450.0, 0.0)):
        c += [(cx - r, cy - r), (cx + r, cy - r), (cx - r, cy + r), (cx + r, cy + r)]
    c += [(653.0, 54.0), (654.0, 53.0), (650.0, 55.0), (655.0, 50.0), (646.0, 47.0)]
    sets["ties"] = np.array(c)
    sets["one"] = np.array([[17.0, 23.0]])
    return (w, h), sets


def near_root_pairs():
    """Pairs of points of the cell (0, 0) of a 2-pixel grid (centre (1, 1)) whose squared distances to the centre differ while
    their correctly rounded roots agree; the farther point comes first, so 'center' must keep it.  Searched, not assumed."""
    rng = np.random.default_rng(7)
    out = []
    while len(out) < 2:
        x, y = rng.uniform(1.1, 1.9, 2)
        d2 = (x - 1.0) ** 2 + (y - 1.0) ** 2
        x2 = x
        for _ in range(40):
            x2 = np.nextafter(x2, 2.0)
            e2 = (x2 - 1.0) ** 2 + (y - 1.0) ** 2
            if e2 > d2 and np.sqrt(e2) == np.sqrt(d2):
                out.append(((x2, y), (x, y)))           # the farther one first
                break
    return out


def main():
    gcp = load_reference()
    (w, h), sets = point_sets()
    cases = []
    for name in ("int", "float"):
        for grid in (50, 64, 100, 333, 2000):           # 64 and 333 do not divide 1504 x 1000; 2000: one cell
            for sel, seed in (("first", None), ("center", None), ("random", 11)):
                cases.append((sets[name], grid, (w, h), sel, seed))
    cases.append((sets["float"], 37.5, (w, h), "center", None))          # a float grid size
    cases.append((sets["ties"], 100, (w, h), "center", None))
    cases.append((sets["ties"], 100, (w, h), "first", None))
    cases.append((sets["ties"][::-1].copy(), 100, (w, h), "center", None))
    cases.append((sets["one"], 100, (w, h), "first", None))
    cases.append((sets["one"], 100, (w, h), "center", None))
    cases.append((sets["one"], 100, (w, h), "random", 3))
    pairs = near_root_pairs()
    pts = np.array([q for pr in pairs for q in pr])
    d = np.sqrt((pts[:, 0] - 1.0) ** 2 + (pts[:, 1] - 1.0) ** 2)
    d2 = (pts[:, 0] - 1.0) ** 2 + (pts[:, 1] - 1.0) ** 2
    assert d[0] == d[1] and d2[0] != d2[1], "the pair no longer shares a rounded root"
    cases.append((pts, 2, (8, 8), "center", None))
    res = {}
    for k, (p, grid, size, sel, seed) in enumerate(cases):
        mask = gcp._filter_spatial(p, grid, size, selection=sel, random_state=seed)
        res[f"pts{k}"] = p
        res[f"args{k}"] = np.array([grid, size[0], size[1], -1 if seed is None else seed], dtype=np.float64)
        res[f"sel{k}"] = np.array(sel)
        res[f"mask{k}"] = mask
    np.savez_compressed(os.path.join(OUT, "g21_filter_spatial.npz"), n_cases=len(cases), **res)
    print("g21_filter_spatial.npz:", len(cases), "cases;", sum(int(res[f"mask{k}"].sum()) for k in range(len(cases))), "points kept")


if __name__ == "__main__":
    main()
