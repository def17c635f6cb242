// segment_driver.cpp — runs the header-only C++ range-image segmentation (svn-icp_amd/host/registration_pipeline.hpp:
// segment_images, segment_scan) on a file of points; tests/test_segment_cpu.py compares it with pipeline.py.
//   segment_driver in.bin out.bin [reps]   (reps > 0: also time segment_scan, median of reps calls, printed in ms)
// in.bin : svnicp_seg_params, int32 n, n x 3 float32
// out.bin: int64 m, m x 3 float32 segmented cloud, m x int64 input index, then the images [n_scan * horizon_scan]:
//          int32 owner, float32 range, int8 ground, int32 label
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "registration_pipeline.hpp"

template <typename T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) { fprintf(stderr, "usage: %s in.bin out.bin [reps]\n", argv[0]); return 64; }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) { perror("open"); return 65; }
  svnicp_seg_params prm;
  int32_t n = 0;
  if (!rd(fi, &prm, 1) || !rd(fi, &n, 1)) return 66;
  svnicp::Cloud pts((size_t)n);
  if (n && !rd(fi, &pts[0][0], (size_t)3 * n)) return 66;
  std::vector<int64_t> idx;
  const svnicp::Cloud out = svnicp::segment_scan(pts, prm, &idx);
  const svnicp::SegImages im = svnicp::segment_images(pts, prm);
  const int64_t m = (int64_t)out.size();
  fwrite(&m, sizeof m, 1, fo);
  if (m) { fwrite(&out[0][0], sizeof(float), (size_t)3 * m, fo); fwrite(idx.data(), sizeof(int64_t), (size_t)m, fo); }
  fwrite(im.owner.data(), sizeof(int32_t), im.owner.size(), fo);
  fwrite(im.range.data(), sizeof(float), im.range.size(), fo);
  fwrite(im.ground.data(), sizeof(int8_t), im.ground.size(), fo);
  fwrite(im.label.data(), sizeof(int32_t), im.label.size(), fo);
  fclose(fo); fclose(fi);
  const int reps = argc == 4 ? atoi(argv[3]) : 0;
  if (reps > 0) {
    std::vector<double> ms;
    for (int k = 0; k < reps; ++k) {
      const auto t0 = std::chrono::steady_clock::now();
      const svnicp::Cloud o = svnicp::segment_scan(pts, prm);
      ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() + 0.0 * (double)o.size());
    }
    std::sort(ms.begin(), ms.end());
    printf("host segment_scan: median %.3f ms over %d calls\n", ms[ms.size() / 2], reps);
  }
  printf("segmented %d points into %lld\n", n, (long long)m);
  return 0;
}
