// morton_order_driver.hip — the Morton sort of stage A alone (svn-icp_amd/csrc/spatial_prep.hip, compiled into this
// program): launch_morton_order_joint through the project's three-pass radix chain and through rocPRIM's radix_sort_pairs,
// both `order` arrays compared element by element with each other and with std::stable_sort by key on the host (a stable
// sort by key is the one order by (key, input position), so there is nothing to tolerate).  The keys come from the device:
// rocPRIM's call leaves keys_a as k_morton_keys wrote it.  tests/test_morton_order_gpu.py runs it once and reads the lines.
//   morton_order_driver            one line per case:
//   case <name> M <M> n <n> radix_vs_host <mismatches> merge_vs_host <mismatches> radix_vs_merge <mismatches> fill <bad words>
//        distinct_keys <count> radix_us <stream time> merge_us <stream time>
// exit status 0: every case ran (mismatches are the test's business), 1: a HIP call failed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "kernels.hpp"

using namespace svnicp;

#define CHK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); exit(1); } } while (0)

template <class T> struct Dev {
  T* p = nullptr;
  explicit Dev(size_t n) { CHK(hipMalloc(&p, (n ? n : 1) * sizeof(T))); }
  ~Dev() { (void)hipFree(p); }
};

struct Result { std::vector<int32_t> order; std::vector<unsigned int> keys; float us; long bad_fill; };

static Result run(const std::vector<double>& tgt, const std::vector<double>& src, bool rocprim_sort, hipStream_t st) {
  const int64_t M = (int64_t)tgt.size() / 3, n = (int64_t)src.size() / 3;
  const size_t N = (size_t)(M + n), fill_words = 1000 + (size_t)n;
  Dev<double> dt(tgt.size()), ds(src.size());
  Dev<unsigned long long> bbox(6);
  Dev<unsigned int> ka(N), kb(N);
  Dev<int32_t> va(N), order(N), fill(fill_words + 1);
  const size_t tmp_bytes = sort_temp_bytes(N, 31);
  Dev<unsigned char> tmp(tmp_bytes);
  CHK(hipMemcpy(dt.p, tgt.data(), tgt.size() * 8, hipMemcpyHostToDevice));
  CHK(hipMemcpy(ds.p, src.data(), src.size() * 8, hipMemcpyHostToDevice));
  Pose0 pose{};
  pose.R0[0] = pose.R0[4] = pose.R0[8] = 1.0;
  hipEvent_t e0, e1;
  CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
  Result r;
  for (int rep = 0; rep < 2; ++rep) {   // the first call warms up (code load), the second is timed
    CHK(hipMemsetAsync(order.p, 0xff, N * 4, st));
    CHK(hipMemsetAsync(fill.p, 0, (fill_words + 1) * 4, st));
    CHK(launch_bbox(dt.p, M, bbox.p, false, st));
    CHK(hipEventRecord(e0, st));
    CHK(launch_morton_order_joint(dt.p, M, ds.p, n, pose, bbox.p, ka.p, kb.p, va.p, order.p, tmp.p, tmp_bytes, rocprim_sort, fill.p, fill_words, st));
    CHK(hipEventRecord(e1, st));
    CHK(hipStreamSynchronize(st));
  }
  float ms = 0.0f;
  CHK(hipEventElapsedTime(&ms, e0, e1));
  r.us = 1000.0f * ms;
  r.order.resize(N); r.keys.resize(N);
  CHK(hipMemcpy(r.order.data(), order.p, N * 4, hipMemcpyDeviceToHost));
  CHK(hipMemcpy(r.keys.data(), ka.p, N * 4, hipMemcpyDeviceToHost));   // the unsorted keys behind rocPRIM's call only
  std::vector<int32_t> f(fill_words + 1);
  CHK(hipMemcpy(f.data(), fill.p, (fill_words + 1) * 4, hipMemcpyDeviceToHost));
  r.bad_fill = f[fill_words] != 0;   // the word behind the table stays
  for (size_t i = 0; i < fill_words; ++i) r.bad_fill += f[i] != -1;
  CHK(hipEventDestroy(e0)); CHK(hipEventDestroy(e1));
  return r;
}

static long mismatches(const std::vector<int32_t>& a, const std::vector<int32_t>& b) {
  long bad = a.size() != b.size();
  for (size_t i = 0; i < a.size() && i < b.size(); ++i) bad += a[i] != b[i];
  return bad;
}

static void one_case(const std::string& name, const std::vector<double>& tgt, const std::vector<double>& src, hipStream_t st) {
  const int64_t M = (int64_t)tgt.size() / 3, n = (int64_t)src.size() / 3;
  const Result merge = run(tgt, src, true, st);
  const Result radix = run(tgt, src, false, st);
  // host: values as k_morton_keys writes them (row indices of their own cloud), stable sort by the device's keys
  std::vector<int32_t> pos((size_t)(M + n)), want((size_t)(M + n));
  std::iota(pos.begin(), pos.end(), 0);
  std::stable_sort(pos.begin(), pos.end(), [&](int32_t x, int32_t y) { return merge.keys[(size_t)x] < merge.keys[(size_t)y]; });
  for (size_t i = 0; i < pos.size(); ++i) want[i] = pos[i] < M ? pos[i] : pos[i] - (int32_t)M;
  std::vector<unsigned int> k = merge.keys;
  std::sort(k.begin(), k.end());
  const long distinct = (long)(std::unique(k.begin(), k.end()) - k.begin());
  printf("case %s M %lld n %lld radix_vs_host %ld merge_vs_host %ld radix_vs_merge %ld fill %ld distinct_keys %ld radix_us %.1f merge_us %.1f\n",
         name.c_str(), (long long)M, (long long)n, mismatches(radix.order, want), mismatches(merge.order, want),
         mismatches(radix.order, merge.order), radix.bad_fill + merge.bad_fill, distinct, radix.us, merge.us);
  fflush(stdout);
}

static std::vector<double> cloud(int64_t n, unsigned seed, double lo = -20.0, double hi = 20.0) {
  std::mt19937_64 g(seed);
  std::uniform_real_distribution<double> u(lo, hi);
  std::vector<double> p((size_t)n * 3);
  for (double& v : p) v = u(g);
  return p;
}

int main() {
  hipStream_t st;
  CHK(hipStreamCreate(&st));
  const double nan = std::numeric_limits<double>::quiet_NaN();
  // sizes: the smallest shape that reaches the tile family, one more, a larger one
  one_case("size_7780_1000", cloud(7780, 1), cloud(1000, 2), st);
  one_case("size_7781_1001", cloud(7781, 3), cloud(1001, 4), st);
  one_case("random_16384_4096", cloud(16384, 5), cloud(4096, 6), st);
  one_case("flagship_262144_131072", cloud(262144, 20), cloud(131072, 21), st);   // the benchmark's clouds: 64 + 32 workgroups
  // block edges: both clouds one below, at and one above a multiple of the radix chain's workgroup (1024 threads x 4 pairs =
  // 4096 pairs of ONE cloud; a multiple of the 4 pairs per thread and of a wave's 256 as well)
  one_case("edge_below", cloud(16383, 7), cloud(8191, 8), st);
  one_case("edge_at", cloud(16384, 9), cloud(8192, 10), st);
  one_case("edge_above", cloud(16385, 11), cloud(8193, 12), st);
  {  // one cell: every point the same, one key per cloud
    std::vector<double> t((size_t)16384 * 3, 1.25), s((size_t)4096 * 3, 1.25);
    one_case("one_cell_16384_4096", t, s, st);
  }
  {  // two cells: the box's two corners
    std::vector<double> t = cloud(9000, 13), s = cloud(3000, 14);
    for (size_t i = 0; i < t.size(); ++i) t[i] = ((i / 3) % 3 == 0) ? -5.0 : 5.0;
    for (size_t i = 0; i < s.size(); ++i) s[i] = ((i / 3) % 5 < 2) ? -5.0 : 5.0;
    one_case("two_cells", t, s, st);
  }
  {  // heavy duplicates: snapped to a 0.5 m grid in a small room, stability decides
    std::vector<double> t = cloud(16384, 15, -3.0, 3.0), s = cloud(4096, 16, -3.0, 3.0);
    for (double& v : t) v = 0.5 * std::round(v / 0.5);
    for (double& v : s) v = 0.5 * std::round(v / 0.5);
    one_case("grid_duplicates", t, s, st);
  }
  {  // NaN coordinates: key digit 0 along that axis; whole NaN rows: key 0
    std::vector<double> t = cloud(9001, 17), s = cloud(2999, 18);
    for (size_t i = 0; i < t.size() / 3; ++i) {
      if (i % 3 == 0) t[3 * i] = t[3 * i + 1] = t[3 * i + 2] = nan;
      else if (i % 7 == 0) t[3 * i + 1] = nan;
    }
    for (size_t i = 0; i < s.size() / 3; ++i)
      if (i % 2 == 0) s[3 * i] = s[3 * i + 1] = s[3 * i + 2] = nan;
    one_case("nan_rows", t, s, st);
    std::vector<double> tn((size_t)8192 * 3, nan), sn((size_t)1024 * 3, nan);
    one_case("all_nan", tn, sn, st);
  }
  {  // sentinel: every query beyond the box's far corner, so every query key is the largest key
    std::vector<double> t = cloud(8200, 19), s((size_t)2000 * 3, 1e6);
    one_case("sentinel_queries", t, s, st);
  }
  CHK(hipStreamDestroy(st));
  return 0;
}
