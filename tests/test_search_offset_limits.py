"""The size limit behind the search kernel's 32-bit pair offsets (no GPU needed).

k_stein_search_bf16 writes kbest / kidx ([B][Ppad]) and reads cand ([B][K]) through 32-bit BYTE offsets from the row of a
wave step's first point: offset = 4 · (row · width + column), row < 4 points per step, column < width.  The launchers
refuse any plan that search_offsets_fit (svn-icp_amd/csrc/search_limits.hpp) rejects.  This test compiles that header on
the host and checks, at the boundary, that every accepted width keeps the kernel's unsigned 32-bit arithmetic exact and
that the first rejected width is one where it would wrap.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svn-icp_amd", "csrc")

PROBE = r"""
#include <cstdio>
#include <cstdint>
#include <initializer_list>
#include "search_limits.hpp"
using namespace svnicp;
// the kernel's arithmetic: unsigned 32-bit, worst row and column of a step
static bool u32_exact(int Ppad, int K) {
  for (int w : {Ppad, K}) {
    const unsigned int row = (unsigned int)(kSearchPointsPerStep - 1), col = (unsigned int)w - 1u;
    const unsigned int off4 = 4u * (row * (unsigned int)w + col);
    const uint64_t exact = 4ull * ((uint64_t)row * (uint64_t)w + col);
    if ((uint64_t)off4 != exact) return false;
  }
  return true;
}
int main() {
  const int cases[][2] = {{128, 100}, {65536, 100}, {1 << 28, 100}, {(1 << 28) + 1, 100}, {100, 1 << 28},
                          {100, (1 << 28) + 1}, {1 << 30, 100}, {2147483647, 128}};
  for (auto& c : cases) std::printf("%d %d %d %d\n", c[0], c[1], (int)search_offsets_fit(c[0], c[1]), (int)u32_exact(c[0], c[1]));
  return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("limits")
    (d / "probe.cpp").write_text(PROBE)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)
    out = subprocess.run([str(d / "probe")], check=True, capture_output=True, text=True).stdout
    return {(int(p), int(k)): (f == "1", e == "1") for p, k, f, e in (l.split() for l in out.splitlines())}


def test_accepted_sizes_keep_the_32bit_offsets_exact(probe):
    for (p, k), (fits, exact) in probe.items():
        if fits:
            assert exact, (p, k)


def test_limit_is_at_the_first_width_that_would_wrap(probe):
    b = 1 << 28
    assert probe[(b, 100)] == (True, True) and probe[(100, b)] == (True, True)
    assert probe[(b + 1, 100)] == (False, False) and probe[(100, b + 1)] == (False, False)
    assert probe[(65536, 100)][0]   # 65 536 particles: any number of source points per workgroup
    assert not probe[(1 << 30, 100)][0] and not probe[(2147483647, 128)][0]
