#!/usr/bin/env python3
"""g20_weighted.npz: frequency weights, evaluated by the reference itself on ROW-DUPLICATED tables (build container only).

    python tests/golden/gen_golden_weighted.py

The reference has no weights.  For integer weights "weight w_i" means "row i appears w_i times", and that it can evaluate:
the losses stored here are what `CMAOptimizer._loss_function` (optimize.py:329-357) returned, with both losses, for tables in
which row i of the points and of the observations is repeated w_i times (np.repeat: rows of weight 0 are absent).  Stored:
1 103 GCP-like points, their noisy observations, integer weights 0..3 (about a fifth of them 0), and three populations of
P = 140 (two candidate tiles, the second ragged; row 0 = the initial camera, rows 3 and 7 identical):
  lf   the first phase's nine targets around a camera WITHOUT lens coefficients (the lens-free kernel variant),
  gen  all 21 targets around a camera with a lens (the general variant),
  sp   the twelve lens coefficients alone (every candidate shares the pose: the shared-pose variant),
each with its initial parameters, targets, bounds, normalised candidates X and the losses md / hub.  The UN-duplicated points
are what is stored.  Data only."""
import os
import sys

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import BASE, FULL, gcp_like, load_reference, pvec  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
POSE9 = ["x", "y", "z", "fov", "pan", "tilt", "roll", "a1", "a2"]
LENS12 = ["k1", "k2", "k3", "k4", "k5", "k6", "p1", "p2", "s1", "s2", "s3", "s4"]


def main():
    opt, _ = load_reference()
    rng = np.random.default_rng(20261018)
    truth = dict(FULL, x=FULL["x"] + 4, y=FULL["y"] - 6, z=FULL["z"] + 2, fov=73.0, pan=97.0)
    n = 1103
    pts = gcp_like(opt, rng, n, truth)
    uv_obs = opt.project(pd.DataFrame(pts, columns=["x", "y", "z"]), truth).to_numpy() + rng.normal(0, 1.0, (n, 2))
    w = rng.choice(4, size=n, p=[0.2, 0.3, 0.3, 0.2]).astype(np.float64)
    rep = w.astype(np.int64)
    dfx = pd.DataFrame(np.repeat(pts, rep, axis=0), columns=["x", "y", "z"])
    dfu = pd.DataFrame(np.repeat(uv_obs, rep, axis=0), columns=["u", "v"])
    assert len(dfx) == int(w.sum())
    g = dict(xyz=pts, uv_obs=uv_obs, weights=w)
    P = 140
    for name, init, tgt, spread in (("lf", dict(BASE, tilt=3.0, roll=1.0, a1=1.02, a2=0.98), POSE9, 0.1),
                                    ("gen", dict(FULL), POSE9 + LENS12, 0.05),
                                    ("sp", dict(FULL), LENS12, 0.05)):
        o = opt.CMAOptimizer(dfx, dfu, dict(init))
        o.set_target(tgt)
        bounds = opt.bounds_to_array(o.params_init, tgt, None)
        X = rng.uniform(0.5 - spread, 0.5 + spread, (P, len(tgt)))
        X[0] = 0.5
        X[7] = X[3]
        g.update({f"{name}_params_init": pvec(init), f"{name}_targets": np.array(tgt), f"{name}_bounds": bounds, f"{name}_X": X})
        for tag, fs in (("md", None), ("hub", 10.0)):
            f = o._loss_function(bounds, fs)
            g[f"{name}_{tag}"] = np.array([f(x) for x in X])
        print("g20_weighted:", name, "argmin md", int(np.argmin(g[f"{name}_md"])), "hub", int(np.argmin(g[f"{name}_hub"])),
              "losses", g[f"{name}_md"][:3])
    np.savez(f"{OUT}/g20_weighted.npz", **g)
    print("g20_weighted: n", n, "zeros", int((w == 0).sum()), "W", int(w.sum()))


if __name__ == "__main__":
    main()
