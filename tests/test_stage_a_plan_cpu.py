"""Which stage-A kernel a registration gets, and the sizes its scratch follows (no GPU needed).

svn-icp_amd/csrc/stage_a_plan.hpp states the choice among the four exact top-K kernels (streaming, seeded scan, Morton
tiles, brute force) as one pure function of the query rows, M, K and the option `knn`.  This test compiles that header on
the host and checks the choice case by case.  The expectations were worked out from the rules by
hand and by a script, not taken from the header's output: among them the two rules that are easy to miss — option `tiles`
is "automatic without brute force", and option `brute` with K > 128 is the same.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svn-icp_amd", "csrc")

KERNELS = ("Stream", "SeededScan", "Tiles", "Brute")
OPTIONS = {"auto": "KnnOption{}", "v1": "KnnOption{false, KnnKernel::Stream}", "v2": "KnnOption{false, KnnKernel::SeededScan}",
           "tiles": "KnnOption{false, KnnKernel::Tiles}", "brute": "KnnOption{false, KnnKernel::Brute}"}

# (query rows, M, K, option) -> kernel
CASES = [
    (700, 20000, 7, "auto", "Brute"),
    (131072, 262144, 100, "auto", "Tiles"),
    (16384, 16384, 100, "auto", "Brute"),            # exactly 2^28 pairs
    (16384, 16385, 100, "auto", "Tiles"),
    (900, 12000, 150, "auto", "SeededScan"),
    (900, 12000, 150, "brute", "SeededScan"),        # brute with K > 128: automatic without brute force
    (900, 12000, 150, "tiles", "SeededScan"),
    (700, 20000, 7, "tiles", "Tiles"),
    (100, 5000000, 8, "auto", "SeededScan"),         # 9766 tiles > 8192
    (100, 5000000, 8, "tiles", "SeededScan"),
    (300, 7680, 1, "v2", "Stream"),                  # 15 tiles: below the seeded scan's 16
    (300, 7681, 1, "v2", "SeededScan"),              # pads to 8192
    (1000000, 3000, 201, "auto", "Stream"),
    (300000, 2000, 16, "auto", "Stream"),
    (700, 20000, 7, "v1", "Stream"),
    (131072, 262144, 100, "brute", "Brute"),         # the option has no pair limit
    (1, 1, 1, "auto", "Brute"),
    (300, 9000, 201, "v2", "Stream"),
]

PROBE = r"""
#include <cstdio>
#include <initializer_list>
#include "stage_a_plan.hpp"
using namespace svnicp;
int main() {
%s
  for (int K : {1, 64, 128, 129, 200}) std::printf("size %%d %%d %%d\n", K, knn_pool_size(K), knn_slice_count(K));
  return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("stage_a_plan")
    lines = "\n".join('  std::printf("plan %d %%d\\n", (int)plan_stage_a(%dll, %dll, %d, %s, -1).kernel);' % (i, rows, M, K, OPTIONS[opt])
                      for i, (rows, M, K, opt, _) in enumerate(CASES))
    (d / "probe.cpp").write_text(PROBE % lines)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)
    out = subprocess.run([str(d / "probe")], check=True, capture_output=True, text=True).stdout
    rows = [l.split() for l in out.splitlines()]
    return ({int(r[1]): KERNELS[int(r[2])] for r in rows if r[0] == "plan"},
            {int(r[1]): (int(r[2]), int(r[3])) for r in rows if r[0] == "size"})


@pytest.mark.parametrize("i", range(len(CASES)), ids=["%d-%d-%d-%s" % c[:4] for c in CASES])
def test_kernel_choice(probe, i):
    assert probe[0][i] == CASES[i][4], CASES[i]


def test_pool_and_slice_sizes_at_their_boundaries(probe):
    sizes = probe[1]
    assert [sizes[K][0] for K in (1, 64, 128, 129)] == [256, 256, 256, 512]
    assert [sizes[K][1] for K in (1, 64, 128, 200)] == [64, 64, 64, 32]
