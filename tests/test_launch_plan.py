"""CPU: the launch planning of the point-set kernels (alproj_amd/csrc/host/alp_plan.h: pop_grid, stage_chunk_points,
stream_grid) against the Python restatements the GPU tests lean on (tests/cma_cases.py: batched_grid; tests/residual_cases.py:
chunk_points, launches, stride_pass).  The C++ is reached through the self-checking driver of the HIP-free host code
(csrc/host/alp_host_selfcheck.cpp --plan), built without HIP by the library's own clang++: what it prints is what
popeval_launch_t, residuals_impl and jacobian_impl launch with.  A mismatch is a bug in one of the two statements."""
import subprocess

import pytest

from alproj_amd import _build
from tests import cma_cases as cc
from tests import residual_cases as rc

# the five readings and the sweep of tests/test_cma_sampler_reference.py: test_batched_grid_rule_at_the_tested_shapes
NAMED = [(10_000_000, 65536, "f32", False), (1127, 250, "f64", True), (1_000_000, 65536, "f32", False),
         (1_000_000, 32768, "f64", True), (67 * 256 - 37, 4096, "f64", False)]
SWEEP = [(n, R, prec, lf) for n in (1, 300, 1127, 67 * 256 - 37, 10 ** 5, 10 ** 6, 10 ** 7, 10 ** 8)
         for R in (2, 250, 2048, 4096, 32768, 65536) for prec in ("f32", "f64") for lf in (False, True)]
CUS = (256, 64, 304)
CHUNK22 = rc.chunk_points(1 << 40, 22)


def plan(queries):
    """[(stripes, tile columns, chunk points, stream grid, confirm grid)] of [(n, P, prec, V, cu, batched, pairs[, a, b])]"""
    if _build.host_compiler("clang") is None:
        pytest.skip("no clang compiler")
    exe = _build.build_host("plain", "clang")
    text = "".join(",".join(str(v) for v in (q[0], q[1], q[2], q[3], cc.POP_TC) + tuple(q[4:])) + "\n" for q in queries)
    r = subprocess.run([exe, "--plan"], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(out) == len(queries)
    return out


@pytest.mark.parametrize("batched", [True, False])
def test_pop_grid_is_the_restated_rule(batched):
    """every shape of test_batched_grid_rule_at_the_tested_shapes at 256, 64 and 304 CUs, batched and not (the unbatched rule is
    the one behind config 5's and config 3's headline numbers)"""
    cases = [(n, R, prec, lf, cu) for cu in CUS for (n, R, prec, lf) in NAMED + SWEEP]
    got = plan([(n, R, prec, cc.GROUP_V[(prec, lf)], cu, int(batched), 1) for (n, R, prec, lf, cu) in cases])
    for case, g in zip(cases, got):
        assert g[:2] == cc.batched_grid(*case, batched=batched), (case, batched, g)


def test_pop_grid_readings_of_the_gpu_tests():
    """the numbers written into test_batched_grid_rule_at_the_tested_shapes, read off the C++ itself"""
    got = plan([(n, R, prec, cc.GROUP_V[(prec, lf)], 256, 1, 1) for (n, R, prec, lf) in NAMED])
    assert [g[:2] for g in got] == [(256, 512), (5, 2), (256, 512), (512, 2), (67, 16)]
    # the 2171 stripes the unbatched rule gives the first of them, before the cap
    assert plan([(10_000_000, 65536, "f32", 6, 256, 0, 1)])[0][:2] == (2171, 512)


def test_pop_grid_override_order():
    """ALP_POP_GRID comes before the clamp to the rows and before the batched steps; a pair that is not valid is ignored"""
    n, rows = 1127, 5
    plain = plan([(n, 250, "f64", 6, 256, 0, 1)])[0][:2]
    assert plan([(n, 250, "f64", 6, 256, 0, 1, 3, 2)])[0][:2] == (3, 2)
    assert plan([(n, 250, "f64", 6, 256, 0, 1, 900, 1)])[0][:2] == (rows, 1)
    assert plan([(n, 250, "f64", 6, 256, 1, 1, 900, 1)])[0][:2] == (rows, 2)          # batched: the fill rule still adds columns
    assert plan([(n, 250, "f64", 6, 256, 0, 1, 3, 3)])[0][:2] == plain                 # 250 candidates are two tiles
    assert plan([(n, 250, "f64", 6, 256, 0, 1, 0, 1)])[0][:2] == plain


def test_stage_chunks_are_the_restated_rule():
    """B (residuals) and D (Jacobian) of tests/test_gpu_residuals.py and tests/test_gpu_jacobian.py; n around one chunk, CHUNK22
    and the 10 M DSM"""
    n10 = 3163 * 3163                       # synthetic.grid_side(10_000_000) squared: the bench-shaped DSM
    cases = []
    for B in (1, 2, 3, 11, 21, 22, rc.B_MAX):
        c = rc.chunk_points(1 << 40, B)
        for n in (1, 1023, 1024, 1025, c - 1, c, c + 1, 2 * c, 3 * c + 517, CHUNK22, 2 * CHUNK22, 3 * CHUNK22 + 517, 3 * 4096 + 5,
                  10_000_000, n10):
            cases.append((n, B))
    got = plan([(n, 1, "f32", 6, 256, 0, B) for (n, B) in cases])
    for (n, B), g in zip(cases, got):
        assert g[2] == rc.chunk_points(n, B), (n, B, g)
        assert -(-n // g[2]) == rc.launches(n, B), (n, B, g)
    assert rc.launches(2 * CHUNK22, 22) == 2 and rc.launches(3 * CHUNK22 + 517, 22) == 4 and rc.launches(3 * 4096 + 5, rc.B_MAX) == 4


@pytest.mark.parametrize("cu", [1, 64, 256, 304])
def test_stream_grid_cap_is_one_stride_pass(cu):
    """stride_pass = the cap of stream_grid x 256 lanes x RES_V points; below the cap one workgroup per 256 items"""
    S = rc.stride_pass(cu)
    items = [1, 255, 256, 257, 256 * (8 * cu - 1), 256 * 8 * cu, 256 * 8 * cu + 1, S, 10 ** 8, 1 << 40]
    got = plan([(n, 1, "f32", 6, cu, 0, 1) for n in items])
    for n, g in zip(items, got):
        assert g[3] == min(-(-n // 256), 8 * cu), (n, g)
    assert got[-1][3] * 256 * rc.RES_V == S
