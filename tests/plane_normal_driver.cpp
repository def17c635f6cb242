// plane_normal_driver.cpp — normal_from_scatter (svn-icp_amd/csrc/plane_normal_device.hpp) as a stand-alone host program for
// tests/test_plane_alone_cpu.py, which builds it with -fsanitize=address,undefined and runs it as a child process.
//   plane_normal_driver cases.txt
// cases.txt : per matrix 7 numbers — finite d0 d1 d2 a01 a02 a12 (text; hexadecimal floats are read exactly)
// stdout    : per matrix one line "valid n0 n1 n2", the normal as hexadecimal floats
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plane_normal_device.hpp"

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 64; }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::perror("open"); return 65; }
  std::vector<double> v;
  char tok[64];
  while (std::fscanf(f, "%63s", tok) == 1) v.push_back(std::strtod(tok, nullptr));
  std::fclose(f);
  if (v.size() % 7 != 0) { std::fprintf(stderr, "%zu numbers: not a multiple of 7\n", v.size()); return 66; }
  for (size_t c = 0; c < v.size() / 7; ++c) {
    const double* p = v.data() + 7 * c;
    double n0 = -1.0, n1 = -1.0, n2 = -1.0;
    const bool valid = svnicp::normal_from_scatter(p[1], p[2], p[3], p[4], p[5], p[6], p[0] != 0.0, n0, n1, n2);
    std::printf("%d %a %a %a\n", valid ? 1 : 0, n0, n1, n2);
  }
  return 0;
}
