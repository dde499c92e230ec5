"""CPU: the oracle of the exact Jacobian (alp_jacobian) and the host half of it.

- A complex-safe restatement of the reference's projection (src/alproj/optimize.py:8-155), pinned to
  oracle.ref_numpy.project_points in real arithmetic, whose complex-step derivative (exact to rounding: no subtraction)
  is the oracle of tests/test_gpu_jacobian.py; checked here against fourth-order central differences.
- The derivative of the pose fold (host/alp_host.cpp: fold_pose_jacobian, a dual-number run of fold_pose_any) compiled
  without HIP into a small driver, against central differences of fold_pose for all 23 targets.
- The Python entry points refuse w / h and repeated targets before any GPU call."""
import os
import subprocess

import numpy as np
import pandas as pd
import pytest

from oracle import ref_numpy as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
KEYS = orc.PARAM_KEYS
TARGETS = [k for k in KEYS if k not in ("w", "h")]          # the 23 keys an exact Jacobian may differentiate


def cs_project(xyz, p):
    """optimize.py:8-155 for an (N, 3) float64 array and a 25-vector p (complex entries allowed, w and h real) ->
    (u, v).  The operations of intrinsic_mat, extrinsic_mat, project and _distort, with numpy's complex-capable
    functions in place of math's."""
    X, Y, Z, fov, pan, tilt, roll, a1, a2, k1, k2, k3, k4, k5, k6, p1, p2, s1, s2, s3, s4 = p[:21]
    w, h, cx, cy = float(np.real(p[21])), float(np.real(p[22])), p[23], p[24]
    pi = np.pi
    fov_x = fov * pi / 180
    fov_y = fov_x * h / w
    fx = w / (2 * np.tan(fov_x / 2))
    fy = h / (2 * np.tan(fov_y / 2))
    a, b, c = pan * pi / 180, -(tilt + 90) * pi / 180, -roll * pi / 180
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    ry = np.array([[np.cos(c), 0, np.sin(c)], [0, 1, 0], [-np.sin(c), 0, np.cos(c)]])
    rot = np.dot(np.dot(rx, ry), rz)
    emat = np.zeros((4, 4), dtype=np.result_type(rot, X, Y, Z))
    emat[:3, :3] = rot
    emat[:3, 3:] = np.dot(rot, np.array([[-X], [-Y], [-Z]]))
    emat[3, 3] = 1
    xyz = np.asarray(xyz, dtype=np.float64)
    cam = np.dot(emat, np.vstack((xyz.T, np.ones((1, xyz.shape[0])))))
    img = np.dot(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]]), cam[:3, :])
    u = w - img[0] / img[2]
    v = img[1] / img[2]
    c0, c1 = (float(q) for q in np.array([(w - 1) / 2, (h - 1) / 2], dtype="float32"))
    x = (u - c0) / c0
    y = (v - c1) / c1
    r = (x ** 2 + y ** 2) ** 0.5
    r2, r4, r6 = r ** 2, r ** 4, r ** 6
    xd = (x * (1 + k1 * r2 + k2 * r4 + k3 * r6) / (1 + k4 * r2 + k5 * r4 + k6 * r6)
          + 2 * p1 * x * y + p2 * (r2 * 2 * x ** 2) + s1 * r2 + s2 * r4)
    yd = (y * (1 + a1 + k1 * r2 + k2 * r4 + k3 * r6) / (1 + a2 + k4 * r2 + k5 * r4 + k6 * r6)
          + 2 * p1 * x * y + p2 * (r2 * 2 * y ** 2) + s3 * r2 + s4 * r4)
    return xd * c0 + c0, yd * c1 + c1


def cs_jacobian(xyz, pvec, targets, of_residuals=True):
    """(2N, D) complex-step Jacobian of the projection (rows u_0, v_0, u_1, ...), negated for the residual vector"""
    pvec = np.asarray(pvec, dtype=np.float64)
    step = 1e-30
    n = len(xyz)
    J = np.empty((2 * n, len(targets)))
    for j, t in enumerate(targets):
        p = pvec.astype(np.complex128)
        p[KEYS.index(t)] += 1j * step
        u, v = cs_project(xyz, p)
        J[0::2, j] = np.imag(u) / step
        J[1::2, j] = np.imag(v) / step
    return -J if of_residuals else J


def g5_case():
    g = np.load(os.path.join(G, "g5_population.npz"))
    return g["xyz"], g["uv_obs"], np.array(g["params_init"], dtype=np.float64)


def g14_case():
    g = np.load(os.path.join(G, "g14_lsq.npz"))
    return g["xyz"], np.array(g["trf_linear_d7_params"], dtype=np.float64)


def cases():
    xyz5, _, p5 = g5_case()
    xyz14, p14 = g14_case()
    return [("g5", xyz5, p5), ("g14", xyz14, p14)]


@pytest.mark.parametrize("name,xyz,p", cases(), ids=["g5", "g14"])
def test_restatement_is_the_reference_projection(name, xyz, p):
    want = orc.project_points(xyz, orc.vector_to_params(p))
    u, v = cs_project(xyz, p.astype(np.complex128))
    assert np.abs(np.imag(u)).max() == 0 and np.abs(np.imag(v)).max() == 0
    got = np.column_stack([np.real(u), np.real(v)])
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


@pytest.mark.parametrize("name,xyz,p", cases(), ids=["g5", "g14"])
def test_complex_step_agrees_with_central_differences(name, xyz, p):
    J = cs_jacobian(xyz, p, TARGETS, of_residuals=False)
    # the differences are taken in coordinates relative to a point near the camera (the model does not change under a common
    # shift of points and camera, and the reference's absolute UTM coordinates would add their own cancellation to them)
    o = np.round(p[:3])
    xyz_l, p_l = xyz - o, p.copy()
    p_l[:3] -= o
    h = 1e-3
    for j, t in enumerate(TARGETS):
        k = KEYS.index(t)

        def f(dt):
            q = p_l.copy()
            q[k] += dt
            u, v = cs_project(xyz_l, q)
            return np.column_stack([u, v]).reshape(-1)

        fd = (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)
        scale = np.abs(J[:, j]).max()
        assert scale > 0, t
        assert np.abs(J[:, j] - fd).max() <= 1e-8 * scale, (name, t, np.abs(J[:, j] - fd).max() / scale)


# ---------------------------------------------------------------------------------------------------- the host fold
DRIVER = r"""
#include "host/alp_host.h"
#include <cstdio>
// stdin: lines of 25 parameters + 3 origin words.  stdout per line: the 32 record words of fold_pose, then the 26 x D
// table of fold_pose_jacobian for the targets given on the command line (or the return code when it refuses)
int main(int argc, char **argv) {
    int32_t t[64];
    int D = argc - 1;
    for (int j = 0; j < D && j < 64; ++j) t[j] = (int32_t)atoi(argv[j + 1]);
    double p[ALP_NPARAM], o[3];
    for (;;) {
        for (int i = 0; i < ALP_NPARAM; ++i) if (scanf("%lf", &p[i]) != 1) return 0;
        for (int i = 0; i < 3; ++i) if (scanf("%lf", &o[i]) != 1) return 0;
        double rec[alp::POSE_WORDS], jac[alp::JAC_WORDS * alp::JAC_MAX];
        alp::fold_pose(p, o, rec);
        for (int i = 0; i < alp::POSE_WORDS; ++i) printf("%.17g ", rec[i]);
        const int rc = alp::fold_pose_jacobian(p, o, t, D, jac);
        if (rc) { printf("rc %d\n", rc); continue; }
        for (int i = 0; i < alp::JAC_WORDS * D; ++i) printf("%.17g ", jac[i]);
        printf("\n");
    }
}
"""


@pytest.fixture(scope="module")
def fold_driver(tmp_path_factory):
    from alproj_amd import _build
    cxx = _build.host_compiler("clang") or _build.host_compiler("gcc")
    if not cxx:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("fold_jac")
    src = d / "fold_jac.cpp"
    src.write_text(DRIVER)
    exe = str(d / "fold_jac")
    cmd = [cxx, "-O2", "-std=c++17", f"-I{_build.INCLUDE}", f"-I{_build.CSRC}", str(src),
           os.path.join(_build.HOST_DIR, "alp_host.cpp"), "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_driver(exe, rows, targets):
    inp = "\n".join(" ".join(repr(float(v)) for v in row) for row in rows) + "\n"
    r = subprocess.run([exe] + [str(KEYS.index(t)) for t in targets], input=inp, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@pytest.mark.parametrize("name,xyz,p", cases(), ids=["g5", "g14"])
def test_record_table_against_central_differences(fold_driver, name, xyz, p):
    # origin: not the camera, so rows 3 / 7 / 11 move with x, y, z.  Camera and origin are shifted together by a point near
    # them (the fold sees their difference alone): a step of 1e-3 on a UTM coordinate would not be representable exactly
    p = p.copy()
    p[:3] -= np.round(p[:3])
    origin = p[:3] + np.array([3.5, -2.25, 1.125])
    h = 1e-3
    rows = [np.concatenate([p, origin])]
    for t in TARGETS:
        for dt in (2 * h, h, -h, -2 * h):
            q = p.copy()
            q[KEYS.index(t)] += dt
            rows.append(np.concatenate([q, origin]))
    out = run_driver(fold_driver, rows, TARGETS)
    D = len(TARGETS)
    first = np.array(out[0].split(), dtype=np.float64)
    jac = first[32:].reshape(26, D)
    recs = np.array([np.array(line.split()[:32], dtype=np.float64) for line in out[1:]]).reshape(D, 4, 32)
    for j, t in enumerate(TARGETS):
        f2, f1, m1, m2 = recs[j]
        fd = ((-f2 + 8 * f1 - 8 * m1 + m2) / (12 * h))[:26]
        scale = max(np.abs(fd).max(), np.abs(jac[:, j]).max())
        assert scale > 0, t
        assert np.abs(jac[:, j] - fd).max() <= 1e-9 * scale, (name, t, np.abs(jac[:, j] - fd).max() / scale)
        # the sparsity jacobian_kernel relies on: a lens target moves one lens word by 1 or 2, a pose target rows 0..11 alone
        if t in orc.DIST_KEYS:
            nz = np.flatnonzero(jac[:, j])
            assert len(nz) == 1 and nz[0] >= 12 and jac[nz[0], j] in (1.0, 2.0), (t, nz)
        else:
            assert not jac[12:, j].any(), t
    # c0, c1 and the constants depend on no target: the table stops at word 25
    assert all(np.array_equal(r[26:], first[26:32]) for r in recs.reshape(-1, 32))


def test_record_table_refusals(fold_driver):
    _, _, p = g5_case()
    row = [np.concatenate([p, p[:3]])]
    for bad in (["w"], ["fov", "h"], ["pan", "pan"], []):
        assert run_driver(fold_driver, row, bad)[0].split()[-2:] == ["rc", "-1"], bad
    assert "rc" not in run_driver(fold_driver, row, ["cy", "s4", "x"])[0]


# ---------------------------------------------------------------------------------------------------- refusals
def _frames():
    xyz, uv, p = g5_case()
    return (pd.DataFrame(xyz[:50], columns=["x", "y", "z"]), pd.DataFrame(uv[:50], columns=["u", "v"]),
            orc.vector_to_params(p))


@pytest.mark.parametrize("targets", [["fov", "w"], ["h"], ["pan", "tilt", "pan"], ["nope"]])
def test_parameter_covariance_refuses_before_the_gpu(monkeypatch, targets):
    from alproj_amd import _lib
    from alproj_amd import optimize as aopt

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched")

    monkeypatch.setattr(_lib, "Points", no_gpu)
    monkeypatch.setattr(_lib, "init", no_gpu)
    dfx, dfu, params = _frames()
    with pytest.raises(ValueError):
        aopt.parameter_covariance(dfx, dfu, params, targets)


@pytest.mark.parametrize("method", ["trf", "dogbox", "lm"])
@pytest.mark.parametrize("targets", [["fov", "w"], ["pan", "pan"]])
def test_analytic_lsq_refuses_before_the_gpu(monkeypatch, method, targets):
    from alproj_amd import _lib
    from alproj_amd import optimize as aopt

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched")

    monkeypatch.setattr(_lib, "Points", no_gpu)
    monkeypatch.setattr(_lib, "init", no_gpu)
    dfx, dfu, params = _frames()
    o = aopt.LsqOptimizer(dfx, dfu, params)
    o.set_target(targets)
    with pytest.raises(ValueError):
        o.optimize(method=method, jac="analytic")
