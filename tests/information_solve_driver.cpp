// information_solve_driver.cpp — svnicp_information_solve (svn-icp_amd/csrc/information_solve.hpp) as a stand-alone host program
// for tests/test_information_cpu.py, which builds it with -fsanitize=address,undefined and runs it as a child process.
//   information_solve_driver cases.txt
// cases.txt : per case 46 numbers — form pairs sum_wr2 eig_floor_ratio H[36] b[6] (text; "nan" and "inf" are read as such)
// stdout    : per case one line "rc <code>" and, when rc is 0, one line of 110 numbers with %.17g:
//             rank sigma2 eigval[6] eigvec[36] eig_t[3] vec_t[9] eig_r[3] vec_r[9] step[6] cov[36]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "information_solve.hpp"

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 64; }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::perror("open"); return 65; }
  std::vector<double> v;
  char tok[64];
  while (std::fscanf(f, "%63s", tok) == 1) v.push_back(std::strtod(tok, nullptr));
  std::fclose(f);
  if (v.size() % 46 != 0) { std::fprintf(stderr, "%zu numbers: not a multiple of 46\n", v.size()); return 66; }
  for (size_t c = 0; c < v.size() / 46; ++c) {
    const double* p = v.data() + 46 * c;
    svnicp_information io{};
    io.struct_size = (int32_t)sizeof io;
    io.form = (int32_t)p[0]; io.pairs = (int64_t)p[1]; io.sum_wr2 = p[2]; io.eig_floor_ratio = p[3];
    for (int i = 0; i < 36; ++i) io.H[i] = p[4 + i];
    for (int i = 0; i < 6; ++i) io.b[i] = p[40 + i];
    const char* why = nullptr;
    const int rc = svnicp_info::solve(&io, &why);
    std::printf("rc %d%s%s\n", rc, why ? " " : "", why ? why : "");
    if (rc != 0) continue;
    std::printf("%d %.17g", (int)io.rank, io.sigma2);
    auto put = [](const double* a, int n) { for (int i = 0; i < n; ++i) std::printf(" %.17g", a[i]); };
    put(io.eigval, 6); put(io.eigvec, 36); put(io.eig_t, 3); put(io.vec_t, 9); put(io.eig_r, 3); put(io.vec_r, 9);
    put(io.step, 6); put(io.cov, 36);
    std::printf("\n");
  }
  return 0;
}
