"""Where stage A's select kernel writes the search table (registration_plan.hpp: select_writes_table) and where target and
queries share one Morton sort (joint_morton_sort), without a GPU: the rules compiled on the host over the registrations
they must and must not apply to, the options' two values each and their rows in INTEGRATION.md."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svn-icp_amd", "csrc")

PROBE = r"""
#include <cstdio>
#include "registration_plan.hpp"
using namespace svnicp;
static int rule(int P, int K, long long B, long long M, const char* knn, int accum, int table, int batch, bool shard) {
  Tuning t; t.accum = accum; t.table_select = table;
  if (knn[0] == 't') t.knn = {false, KnnKernel::Tiles};
  if (knn[0] == '1') t.knn = {false, KnnKernel::Stream};
  if (knn[0] == '2') t.knn = {false, KnnKernel::SeededScan};
  RegistrationFacts f; f.P = P; f.K = K; f.I = 3; f.B = B; f.M = M; f.p_lo = 0; f.p_hi = P; f.batch = batch; f.shard_set = shard;
  const RegistrationRows r = registration_rows(batch, f.I, B);
  const StageAPlan a = plan_stage_a(r.Bq, M, K, t.knn, t.fallback_sliced_max);
  return select_writes_table(f, t, a, plan_stage_b(f, t, r.Bi)) ? 1 : 0;
}
static int joint(long long B, long long M, const char* knn, int sort, int batch, bool shard) {
  Tuning t; t.sort_joint = sort;
  if (knn[0] == 't') t.knn = {false, KnnKernel::Tiles};
  RegistrationFacts f; f.P = 12; f.K = 100; f.I = 3; f.B = B; f.M = M; f.p_lo = 0; f.p_hi = 12; f.batch = batch; f.shard_set = shard;
  const RegistrationRows r = registration_rows(batch, f.I, B);
  return joint_morton_sort(f, t, plan_stage_a(r.Bq, M, f.K, t.knn, t.fallback_sliced_max)) ? 1 : 0;
}
int main() {
  Tuning d;
  std::printf("sort_default %d\n", d.sort_joint);
  std::printf("sort_tiles %d\n", joint(130, 8229, "tiles", 1, 0, false));
  std::printf("sort_auto_large %d\n", joint(131072, 262144, "auto", 1, 0, false));
  std::printf("sort_separate_option %d\n", joint(130, 8229, "tiles", 0, 0, false));
  std::printf("sort_brute %d\n", joint(130, 8229, "auto", 1, 0, false));
  std::printf("sort_minibatch %d\n", joint(130, 8229, "tiles", 1, 16, false));
  std::printf("sort_particle_shard %d\n", joint(130, 8229, "tiles", 1, 0, true));
  std::printf("default %d\n", d.table_select);
  std::printf("tiles_split %d\n", rule(12, 100, 130, 8229, "tiles", 3, 1, 0, false));
  std::printf("auto_large %d\n", rule(128, 100, 131072, 262144, "auto", 3, 1, 0, false));
  std::printf("gather_option %d\n", rule(12, 100, 130, 8229, "tiles", 3, 0, 0, false));
  std::printf("auto_small_is_brute %d\n", rule(12, 100, 130, 8229, "auto", 3, 1, 0, false));
  std::printf("eight_particles_fused %d\n", rule(8, 100, 130, 8229, "tiles", 3, 1, 0, false));
  std::printf("accum_valu %d\n", rule(12, 100, 130, 8229, "tiles", 1, 1, 0, false));
  std::printf("k_above_128 %d\n", rule(12, 150, 130, 8229, "tiles", 3, 1, 0, false));
  std::printf("target_too_small %d\n", rule(12, 100, 130, 7000, "tiles", 3, 1, 0, false));
  std::printf("streaming %d\n", rule(12, 100, 130, 8229, "1", 3, 1, 0, false));
  std::printf("seeded_scan %d\n", rule(12, 100, 130, 8229, "2", 3, 1, 0, false));
  std::printf("minibatch %d\n", rule(12, 100, 130, 8229, "tiles", 3, 1, 16, false));
  std::printf("particle_shard %d\n", rule(12, 100, 130, 8229, "tiles", 3, 1, 0, true));
  return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host compiler")
def test_rule(tmp_path):
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    on = {"default", "tiles_split", "auto_large", "sort_default", "sort_tiles", "sort_auto_large"}
    assert {k for k, v in got.items() if v == "1"} == on, got
    assert len(got) == 20


def test_parser_takes_select_and_gather_only():
    api = open(os.path.join(CSRC, "api.hip")).read()
    m = re.search(r'k == "table"\)\s*\{([^}]*)\}', api)
    assert m, "svnicp_set_option does not parse table"
    body = m.group(1)
    assert re.search(r'v == "select"\)\s*t\.table_select = 1', body) and re.search(r'v == "gather"\)\s*t\.table_select = 0', body)
    assert "else ok = false" in body and sorted(re.findall(r'v == "(\w+)"', body)) == ["gather", "select"]


def test_parser_takes_joint_and_separate_only():
    api = open(os.path.join(CSRC, "api.hip")).read()
    m = re.search(r'k == "sort"\)\s*\{([^}]*)\}', api)
    assert m, "svnicp_set_option does not parse sort"
    body = m.group(1)
    assert re.search(r'v == "joint"\)\s*t\.sort_joint = 1', body) and re.search(r'v == "separate"\)\s*t\.sort_joint = 0', body)
    assert "else ok = false" in body and sorted(re.findall(r'v == "(\w+)"', body)) == ["joint", "separate"]


def test_rules_are_applied_once_where_the_registration_is_planned():
    api = open(os.path.join(CSRC, "api.hip")).read()
    begin = api[api.index("int svnicp_align_begin("):api.index("static int ensure_dbg_upd(")]
    for rule in ("select_writes_table(", "joint_morton_sort("):
        assert api.count(rule) == 1 and rule in begin, rule


def test_option_is_documented():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [l for l in doc.splitlines() if l.startswith("| `table`")]
    assert len(row) == 1 and "`select`" in row[0] and "`gather`" in row[0]
    row = [l for l in doc.splitlines() if l.startswith("| `sort`")]
    assert len(row) == 1 and "`joint`" in row[0] and "`separate`" in row[0]
