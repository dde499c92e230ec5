"""CPU: the launch planning of the point-set kernels (alproj_amd/csrc/host/alp_plan.h: pop_grid, stage_chunk_points,
stream_grid) and of a render frame (frame_plan, initial_park_caps, frame_verdict: read off the C++ at hand-worked cases) against the Python restatements the GPU tests lean on (tests/cma_cases.py: batched_grid; tests/residual_cases.py:
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


def ask(queries):
    """the driver's answer to each query line, split into words"""
    if _build.host_compiler("clang") is None:
        pytest.skip("no clang compiler")
    exe = _build.build_host("plain", "clang")
    r = subprocess.run([exe, "--plan"], input="".join(q + "\n" for q in queries), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = [line.split() for line in r.stdout.splitlines()]
    assert len(out) == len(queries)
    return out


def plan(queries):
    """[(stripes, tile columns, chunk points, stream grid, confirm grid)] of [(n, P, prec, V, cu, batched, pairs[, a, b])]"""
    return [tuple(int(v) for v in words)
            for words in ask([",".join(str(v) for v in (q[0], q[1], q[2], q[3], cc.POP_TC) + tuple(q[4:])) for q in queries])]


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


# ---------------------------------------------------------------- the render frame (alp_raster.hip)
GT = (64, 16)          # cells of a raster_grid_kernel tile (raster_plan.h: GT_W x GT_H)
FRAME_FIELDS = ("tiles_x", "tiles", "plan_grid", "grid_wgs", "parked_wgs0", "parked_wgs1", "general_wgs", "large_wgs", "index_grid",
                "resolve_grid", "tile_bounds_bytes", "tile_lists_bytes")


def frame_plan(implicit, gh, gw, n_tri, w, h, cu):
    q = ",".join(str(v) for v in ("frame", int(implicit), gh, gw, n_tri, w, h, cu) + GT)
    return dict(zip(FRAME_FIELDS, (int(v) for v in ask([q])[0])))


def test_frame_plan_of_the_full_size_frame():
    """the 100 M-vertex DSM on the 5616 x 3744 frame at 256 CUs: 157 x 625 tiles of 64 x 16 cells"""
    p = frame_plan(True, 10000, 10000, 2 * 9999 * 9999, 5616, 3744, 256)
    assert (p["tiles_x"], p["tiles"], p["plan_grid"], p["grid_wgs"], p["resolve_grid"]) == (157, 98125, 384, 98128, 16384)
    assert (p["parked_wgs0"], p["parked_wgs1"], p["general_wgs"], p["large_wgs"]) == (2048, 512, 512, 2048)
    assert (p["tile_bounds_bytes"], p["tile_lists_bytes"], p["index_grid"]) == (98125 * 24, 98125 * 12, 0)


def test_frame_plan_of_the_smallest_meshes():
    """one cell: one tile, one whole turn of the 8 XCDs; one triangle and one pixel: one workgroup each"""
    p = frame_plan(True, 2, 2, 2, 640, 427, 256)
    assert (p["tiles_x"], p["tiles"], p["plan_grid"], p["grid_wgs"]) == (1, 1, 1, 8)
    p = frame_plan(False, 0, 0, 1, 1, 1, 256)
    assert (p["index_grid"], p["resolve_grid"], p["tiles"], p["grid_wgs"]) == (1, 1, 0, 0)
    assert (p["general_wgs"], p["large_wgs"]) == (512, 2048)
    # the caps: 64 workgroups per CU
    p = frame_plan(False, 0, 0, 3 * 64 * 256, 5616, 3744, 1)
    assert (p["index_grid"], p["resolve_grid"]) == (64, 64)


def test_queue_start_capacities():
    """ALP_QUEUE_CAP: the default start gives the cells twice the entries, an override gives every queue the override; the second
    round starts at an eighth + 64"""
    got = [[int(v) for v in line] for line in ask(["queues,-", "queues,8", "queues,0", "queues,1048576", "queues,5000"])]
    M = 1 << 20
    assert got[0] == [M, M, M, 2 * M, M // 8 + 64, M // 8 + 64, 2 * M // 8 + 64]
    assert got[1] == [8, 8, 8, 8, 65, 65, 65]
    assert got[2] == got[0] and got[3] == got[0]            # out of range: ignored; the default spelled out: the default
    assert got[4] == [5000, 5000, 5000, 5000, 689, 689, 689]


def grown(n):
    return n + n // 4 + 1024


@pytest.mark.parametrize("name,has_park,have,round0,round1,want", [
    # have: items, general, small, large, cells, small_b, large_b, cells_b; counters per round: items, general, small, large, cells
    ("no overflow", 1, (8, 8, 8, 8, 8, 65, 65, 65), (8, 8, 8, 8, 8), (8, 8, 65, 65, 65),
     ("-", "-", "-", 8, 8, 8, 8, 8, 65, 65, 65)),
    ("first-round cells alone", 1, (8, 8, 8, 8, 8, 65, 65, 65), (0, 3, 8, 0, 70000), (0, 3, 1, 0, 65),
     ("-", "-", "park", 8, 8, 8, 8, grown(70000), 65, 65, grown(70000) // 8 + 64)),
    ("second-round small triangles alone", 1, (8, 8, 8, 8, 8, 65, 65, 65), (1, 1, 8, 8, 8), (1, 1, 66, 65, 0),
     ("-", "-", "park", 8, 8, 8, 8, 8, grown(66), 65, 65)),
    ("work items of round 1 above those of round 0", 1, (100, 8, 8, 8, 8, 65, 65, 65), (90, 8, 0, 0, 0), (101, 2, 0, 0, 0),
     ("items", "-", "-", grown(101), 8, 8, 8, 8, 65, 65, 65)),
    # no parked queues yet (an index array): their counters are not looked at
    ("parked counters without parked queues", 0, (8, 8, 0, 0, 0, 0, 0, 0), (8, 9, 500, 500, 500), (0, 0, 500, 500, 500),
     ("-", "general", "-", 8, grown(9), 0, 0, 0, 0, 0, 0)),
])
def test_overflow_verdicts(name, has_park, have, round0, round1, want):
    q = ",".join(str(v) for v in ("verdict", has_park) + have + round0 + round1)
    got = ask([q])[0]
    assert got[:3] == list(want[:3]) and [int(v) for v in got[3:]] == list(want[3:]), (name, got)
    # asked again with the capacities it gave, the verdict is none
    again = ask([",".join(str(v) for v in ["verdict", has_park] + got[3:] + list(round0 + round1))])[0]
    assert again == ["-", "-", "-"] + got[3:], (name, again)
