"""The largest cloud a context accepts (registration_plan.hpp: kMaxCloudRows, cloud_rows_refusal): row indices are int32
behind stage A, and a kernel that clamps a winner's index into [0, M - 1] in 32 bits forms its byte offset as
(uint64)(uint32)index * 24.  The largest accepted M keeps that offset exact; the first refused M is refused, and svnicp_set_source / svnicp_set_target / svnicp_set_clouds ask the plan and nothing else.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svn-icp_amd", "csrc")

PROBE = r'''
#include <cstdint>
#include <cstdio>
#include "registration_plan.hpp"
using namespace svnicp;
int main() {
  const int64_t M = kMaxCloudRows;
  const int m_last = (int)(M - 1);                            // what a 32-bit clamp ends at
  const uint64_t off = (uint64_t)(uint32_t)m_last * 24u;      // … and the last row's byte offset
  printf("max %lld\n", (long long)M);
  printf("m_last %d\n", m_last);
  printf("offset %llu\n", (unsigned long long)off);
  printf("accepts_max %d\n", cloud_rows_refusal(M) == nullptr);
  printf("accepts_one %d\n", cloud_rows_refusal(1) == nullptr);
  printf("refuses_next %d\n", cloud_rows_refusal(M + 1) != nullptr);
  printf("refuses_2_32 %d\n", cloud_rows_refusal(1ll << 32) != nullptr);
  return 0;
}
'''


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host compiler")
def test_largest_cloud_keeps_the_row_offset_exact(tmp_path):
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    M = int(got["max"])
    assert M == 2 ** 31 - 1                       # every row index fits an int32
    assert int(got["m_last"]) == M - 1            # … and so does the clamp's upper end
    assert int(got["offset"]) == 24 * (M - 1)     # exact in 64 bits (below 2^36)
    assert got["accepts_max"] == "1" and got["accepts_one"] == "1"
    assert got["refuses_next"] == "1" and got["refuses_2_32"] == "1"


def test_the_setters_ask_the_plan():
    api = open(os.path.join(CSRC, "api.hip")).read()
    assert len(re.findall(r"cloud_rows_refusal\(", api)) == 3
    assert "0x7fffffff" not in api.lower()
