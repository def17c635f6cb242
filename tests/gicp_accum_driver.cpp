// gicp_accum_driver.cpp — runs gicp_accumulate_pair (svn-icp_amd/csrc/gicp_pair_device.hpp: the per-pair arithmetic of
// k_gicp_accumulate) on the host, so that tests/test_gicp_cpu.py can compile it under the address and undefined-behaviour
// sanitizers and compare its sums with the numpy restatement.
//
//   gicp_accum_driver cases.txt
// cases.txt: one pair per line, 15 hexadecimal floats: ok s(3) u(3) m(3) n(3) eps delta.  A line "=" closes a group: the 29
// sums of the group's pairs, added in file order, are printed as hexadecimal floats on one line, and the sums start again.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gicp_pair_device.hpp"

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: gicp_accum_driver cases.txt\n"); return 64; }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::perror("open"); return 65; }
  double acc[svnicp::kGicpSums] = {};
  char line[1024];
  while (std::fgets(line, sizeof line, f)) {
    if (line[0] == '=') {
      for (int i = 0; i < svnicp::kGicpSums; ++i) std::printf("%a%c", acc[i], i + 1 < svnicp::kGicpSums ? ' ' : '\n');
      std::memset(acc, 0, sizeof acc);
      continue;
    }
    double v[15];
    char* p = line;
    for (int i = 0; i < 15; ++i) {
      char* end = nullptr;
      v[i] = std::strtod(p, &end);
      if (end == p) { std::fprintf(stderr, "bad line: %s", line); std::fclose(f); return 66; }
      p = end;
    }
    svnicp::gicp_accumulate_pair(acc, v[0] != 0.0, v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12], v[13], v[14]);
  }
  std::fclose(f);
  return 0;
}
