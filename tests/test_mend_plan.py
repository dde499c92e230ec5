"""CPU: host::mend_grid (alproj_amd/csrc/host/alp_plan.h), the launch shape of the mend pass of a float32 point set, through the
self-checking driver of the HIP-free host code (--plan, query "mend,n,P,V,TC,cu") against the Python restatement the GPU tests
use (tests/mend_cases.py: mend_grid).  The grid is planned for the worst case, every one of the P candidates flagged: at least
one stripe, tile columns that cover P, partial sums (stripes x P doubles) within 128 MB."""
import subprocess

import pytest

from alproj_amd import _build
from tests import mend_cases as mc

V, TC = 5, 128                          # PopCfg<double>: rows per group, candidates per tile
NS = [0, 1, 200, 256, 257, 1129, 1282, 3383, 67 * 256 - 37, 10 ** 5, 10 ** 6, 10 ** 7, 10 ** 8, 2 ** 31 - 1, 2 ** 31]
PS = [1, 2, 127, 128, 129, 300, 2048, 4096, 32768, 65535, 65536]
CUS = [1, 64, 256, 304]


def ask(queries):
    if _build.host_compiler("clang") is None:
        pytest.skip("no clang compiler")
    exe = _build.build_host("plain", "clang")
    r = subprocess.run([exe, "--plan"], input="".join(q + "\n" for q in queries), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(out) == len(queries)
    return out


def test_mend_grid_is_the_restated_rule_and_keeps_its_bounds():
    cases = [(n, P, cu) for cu in CUS for n in NS for P in PS]
    got = ask([f"mend,{n},{P},{V},{TC},{cu}" for (n, P, cu) in cases])
    for (n, P, cu), (stripes, cols) in zip(cases, got):
        assert (stripes, cols) == mc.mend_grid(n, P, V, TC, cu), (n, P, cu)
        assert stripes >= 1 and stripes <= max(1, -(-n // 256)), (n, P, cu, stripes)
        assert cols * TC >= P and (cols - 1) * TC < P, (n, P, cu, cols)
        assert stripes * P * 8 <= 128 << 20, (n, P, cu, stripes)


def test_mend_grid_readings():
    """the shapes of the measurements and of the GPU tests at 256 CUs, read off the C++ itself"""
    got = ask([f"mend,{n},{P},{V},{TC},256" for (n, P) in [(10_000_000, 2048), (10_000_000, 256), (1127, 50), (1129, 300), (3383, 140),
                                                           (2 ** 31, 65536)]])
    assert got == [(1954, 16), (1954, 2), (5, 1), (5, 3), (14, 2), (256, 512)]
