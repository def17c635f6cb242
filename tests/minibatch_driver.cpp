// minibatch_driver.cpp — sets SteinICPParam::use_minibatch through svn-icp_amd/host/svnicp_hip_shim.hpp and registers once;
// tests/test_minibatch_gpu.py compares the table's checksum and the mean pose with the Python run of the same seed.
//   minibatch_driver in.bin
// in.bin: int64 P, B, M, K, I, batch; uint64 seed; f64 init[6][P]; f64 src[B][3]; f64 tgt[M][3]
// stdout: RESULT <sum of idx[j] * (j + 1) mod 2^64> <mean pose, six hex floats>
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "svnicp_hip_shim.hpp"

template <typename T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s in.bin\n", argv[0]); return 64; }
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) { perror("open"); return 65; }
  int64_t h[6];
  uint64_t seed = 0;
  if (!rd(fi, h, 6) || !rd(fi, &seed, 1)) return 66;
  const int64_t P = h[0], B = h[1], M = h[2], K = h[3], I = h[4], batch = h[5];
  std::vector<double> init((size_t)6 * P), src((size_t)3 * B), tgt((size_t)3 * M);
  if (!rd(fi, init.data(), init.size()) || !rd(fi, src.data(), src.size()) || !rd(fi, tgt.data(), tgt.size())) return 66;
  fclose(fi);
  try {
    svnicp::SteinICPParam prm;
    prm.iterations = (int)I; prm.lr = 1.0; prm.max_dist = 1.0; prm.KNN_count = (int)K; prm.SVN_full_grad = false;
    prm.use_minibatch = true; prm.batch_size = (int)batch; prm.minibatch_seed = seed;
    svnicp::SVNICP icp(prm, init);
    icp.add_cloud(src.data(), B, tgt.data(), M, init.data(), (int)P);
    if (icp.stein_align() != svnicp::ALIGN_SUCCESS) return 2;
    const std::vector<int32_t> idx = icp.get_minibatch_indices();
    uint64_t sum = 0;
    for (size_t j = 0; j < idx.size(); ++j) sum += (uint64_t)idx[j] * (uint64_t)(j + 1);
    const auto mean = icp.get_transformation();
    printf("RESULT %" PRIu64, sum);
    for (double v : mean) printf(" %a", v);
    printf("\n");
  } catch (const std::exception& e) {
    fprintf(stderr, "minibatch_driver: %s\n", e.what());
    return 3;
  }
  return 0;
}
