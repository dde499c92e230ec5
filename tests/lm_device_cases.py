"""Helpers of the device loop of LsqOptimizer.optimize(method="normal", device_loop=True), shared by
tests/test_lm_device_host.py (CPU: the state machine of host/alp_lm.h through the selfcheck driver's --lm mode) and
tests/test_gpu_lm_device.py (GPU: the same machine inside alp_lm_step_host, and the whole loop); and the start counts and
stop patterns of tests/test_gpu_lm_device_starts.py (GPU: the loop with up to 1024 starts).

The reference of the state machine is alproj_amd/optimize.py: _normal_lm_steps.  ``lockstep`` runs it and records, per round, the
trial point and the sums it received there; the machine under test then receives the same sums round by round and must
produce the same trial points (within TRIAL_TOL of the box width per coordinate), status, evaluations and iterations.

TRIAL_TOL = 1e-10: a copy of _normal_lm_steps whose Cholesky and triangular solves run in 80-bit np.longdouble stayed within
2.0e-12 of the float64 one on the 48 g14 runs used here (1.2e-13 on the 20 bounded linear runs) and stopped with the same status
after the same number of evaluations in all of them; 1e-10 is 50 x that -- the distance another rounding of the same solve can
move a trial point."""
import subprocess

import numpy as np

from alproj_amd import optimize as aopt

TRIAL_TOL = 1e-10
TOLS = dict(ftol=1e-10, xtol=1e-10, gtol=1e-10)
LINEAR_D = (1, 2, 16, 17, 23)
RUNNING = -2                    # alp_lm_get's status of a start that has not stopped


# ---------------------------------------------------------------------------------------------------- start counts and stop patterns
# (tests/test_gpu_lm_device_starts.py; held by tests/test_lm_device_host.py)
# lm_select_kernel lists the running starts by a ballot per wave of 64, a prefix over the 4 waves of its workgroup, and passes
# of 256 starts that carry `base`.  The start counts put a handle's last start on either side of a wave seam (63 | 64 | 65), a
# pass seam (255 | 256 | 257), in the third pass (513) and at the limit; the seam slots are the first and last slot of a wave
# and of a pass.
WAVE, PASS = 64, 256
SEAM_K = (1, 63, 64, 65, 255, 256, 257, 513, 1024)
SEAM_SLOTS = (0, 63, 64, 65, 255, 256, 257)
HALF_SEED = 5
SPARSE_SEED = 17                # survivors at K = 1024: 8, 5, 0 and 3 in the four passes, none in 8 of the 16 waves
SUBSET_SEED = 11
TABLE_SEED = 13                 # resample.bootstrap_table(n, 257, TABLE_SEED): 257 distinct integer rows at n = 64 and 400


def seam_slots(K):
    """the seam slots that exist among K starts, and the last start"""
    return sorted({j for j in SEAM_SLOTS + (K - 1,) if 0 <= j < K})


def random_half(K):
    """K // 2 of the K slots, seeded"""
    return np.sort(np.random.default_rng(HALF_SEED).permutation(K)[:K // 2])


def sparse_survivors(K):
    """the slots that keep running in the sparse pattern: each with probability 1 / 64, from ONE seeded draw of 1024 numbers,
    so that the survivors among K starts are those among 1024 that lie below K"""
    return np.flatnonzero(np.random.default_rng(SPARSE_SEED).uniform(size=1024)[:K] < 1.0 / WAVE)


def stop_sets(K):
    """{name: the sorted slots to stop} among K starts, each set once: a pattern that does not fit in K, or that is the set
    another name already gave (K = 1: "all but 0" is "none"), is left out"""
    everyone = np.arange(K)
    sets = {"none": everyone[:0], "all": everyone}
    for j in seam_slots(K):
        sets["all but %d" % j] = np.delete(everyone, j)
        sets["only %d" % j] = everyone[j:j + 1]
    sets["even"], sets["odd"] = everyone[0::2], everyone[1::2]
    if K > WAVE:
        sets["first wave"] = everyone[:WAVE]
    if K > PASS:
        sets["first pass"] = everyone[:PASS]
    sets["all but the last wave"] = everyone[:(K - 1) // WAVE * WAVE]
    sets["random half"] = random_half(K)
    sets["all but sparse survivors"] = np.setdiff1d(everyone, sparse_survivors(K))
    out, seen = {}, set()
    for name, s in sets.items():
        s = np.asarray(s, dtype=np.int64)
        if s.tobytes() not in seen:
            seen.add(s.tobytes())
            out[name] = s
    return out


def subset_slots(K=1024):
    """48 of K >= 1024 slots: eight on either side of the seams 64, 256 and 512 (four before, four after), the first and the
    last eight, and eight seeded others"""
    fixed = np.concatenate([np.arange(0, 8), np.arange(60, 68), np.arange(252, 260), np.arange(508, 516), np.arange(K - 8, K)])
    others = np.setdiff1d(np.arange(K), fixed)
    return np.sort(np.concatenate([fixed, np.random.default_rng(SUBSET_SEED).permutation(others)[:8]]))


def pack(G, g, cost):
    """(G (D, D), g (D,), cost) -> the row the machines read: G's row-major upper triangle, g, cost"""
    G = np.asarray(G, dtype=np.float64)
    return np.concatenate([G[np.triu_indices(len(G))], np.asarray(g, dtype=np.float64), [float(cost)]])


def lockstep(fun, x0, lower, upper, max_nfev=None, **tols):
    """_normal_lm_steps on ``fun`` -> (trials [x, ...], rows [packed sums at each trial], result dict)"""
    steps = aopt._normal_lm_steps(x0, lower, upper, max_nfev=max_nfev, **dict(TOLS, **tols))
    trials, rows = [], []
    try:
        x = next(steps)
        while True:
            trials.append(np.array(x, dtype=np.float64))
            out = fun(x)
            rows.append(pack(*out))
            x = steps.send(out)
    except StopIteration as stop:
        return trials, rows, stop.value


def driver(exe, x0, lower, upper, rows, max_nfev=None, **tols):
    """the selfcheck driver's --lm mode on the given rows -> (trials, dict of the final record)"""
    t = dict(TOLS, **tols)
    d = len(x0)
    max_nfev = 100 * d if max_nfev is None else int(max_nfev)
    text = ["%d %d %s %s %s" % (d, max_nfev, float(t["ftol"]).hex(), float(t["xtol"]).hex(), float(t["gtol"]).hex())]
    for v in (x0, lower, upper):
        text.append(" ".join(repr(float(a)) for a in v))
    for r in rows:
        text.append(" ".join(repr(float(a)) for a in r))
    out = subprocess.run([exe, "--lm"], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    trials = [np.array([float.fromhex(w) for w in line.split()[1:]]) for line in out if line.startswith("trial")]
    last = [line for line in out if line.startswith(("final", "starved"))][0].split()
    rec = dict(stopped=last[0] == "final", status=int(last[1]), evaluations=int(last[2]), iterations=int(last[3]),
               cost=float.fromhex(last[4]), grad_norm=float.fromhex(last[5]), mu=float.fromhex(last[6]), nu=float.fromhex(last[7]),
               x=np.array([float.fromhex(w) for w in last[8:]]))
    return trials, rec


def assert_same_run(trials, rec, ref_trials, ref, width, what=""):
    """the machine under test against _normal_lm_steps on the same sums"""
    worst = max((float(np.max(np.abs(a - b) / width)) for a, b in zip(trials, ref_trials)), default=0.0)
    print("%s: %d trial points, worst deviation %.3g of the width (tol %.3g); status %d / %d, evaluations %d / %d" %
          (what, len(ref_trials), worst, TRIAL_TOL, rec["status"], ref["status"], rec["evaluations"], ref["evaluations"]))
    assert len(trials) == len(ref_trials), (len(trials), len(ref_trials))
    assert worst <= TRIAL_TOL
    assert rec["status"] == ref["status"] and rec["evaluations"] == ref["evaluations"] and rec["iterations"] == ref["iterations"]
    assert (np.abs(rec["x"] - ref["x"]) <= TRIAL_TOL * width).all()
    if np.isfinite(ref["cost"]):
        assert rec["cost"] == ref["cost"]
    else:
        assert not np.isfinite(rec["cost"])
    if np.isnan(ref["grad_norm"]):
        assert np.isnan(rec["grad_norm"])
    else:
        assert rec["grad_norm"] == ref["grad_norm"]


def linear_problem(D):
    """A bounded linear least-squares problem with exact G and g: dict(fun, lower, upper, starts (4, D), width).
    A = standard normal (4 D + 8, D) with column scales 1 .. 1e3, b = A x* + 0.01 noise, x* uniform in [-1, 1]; the box is
    [-1, 1] except every third variable, whose upper bound is x* - 0.1 and whose lower bound lies 2 below that: about a third of
    the variables end on a bound."""
    rng = np.random.default_rng(100 + D)
    A = rng.standard_normal((4 * D + 8, D)) * np.logspace(0, 3, D)
    xs = rng.uniform(-1, 1, D)
    b = A @ xs + 0.01 * rng.standard_normal(4 * D + 8)
    lower, upper = -np.ones(D), np.ones(D)
    upper[::3] = xs[::3] - 0.1
    lower[::3] = upper[::3] - 2.0
    G = A.T @ A

    def fun(x):
        r = A @ np.asarray(x, dtype=np.float64) - b
        return G, A.T @ r, 0.5 * float(r @ r)

    starts = rng.uniform(lower, upper, (4, D))
    return dict(fun=fun, lower=lower, upper=upper, starts=starts, width=upper - lower, G=G)
