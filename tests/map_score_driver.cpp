// map_score_driver.cpp — runs the header-only C++ pose scoring (svn-icp_amd/host/registration_pipeline.hpp:
// VoxelHashMap::ScorePoses) on a file of map clouds, scan rows and poses; tests/test_map_score_cpu.py compares it with pipeline.py.
//   map_score_driver in.bin out.bin
// in.bin : f64 voxel_size, f64 map_range, int32 max_points, f64 gate, int32 steps, per step { f64 R[9] (row-major), f64 t[3], int32 m, m x 3 float32 },
//          int32 n, n x 3 float32 scan rows (sensor frame), int32 C, C x 12 f64 poses (R row-major, then t)
// out.bin: C x 4 f64 {located, inliers, sum_d2, cost}
#include <cstdio>
#include <vector>

#include "registration_pipeline.hpp"

template <typename T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 64; }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) { perror("open"); return 65; }
  double voxel = 0, range = 0, gate = 0;
  int32_t max_points = 0, steps = 0, n = 0, C = 0;
  if (!rd(fi, &voxel, 1) || !rd(fi, &range, 1) || !rd(fi, &max_points, 1) || !rd(fi, &gate, 1) || !rd(fi, &steps, 1)) return 66;
  svnicp::VoxelHashMap map(voxel, range, max_points);
  for (int s = 0; s < steps; ++s) {
    svnicp::Pose3 pose;
    int32_t m = 0;
    if (!rd(fi, pose.R.data(), 9) || !rd(fi, pose.t.data(), 3) || !rd(fi, &m, 1)) return 66;
    svnicp::Cloud cloud((size_t)m);
    if (m && !rd(fi, &cloud[0][0], (size_t)3 * m)) return 66;
    map.AddPointCloud(cloud, pose);
  }
  if (!rd(fi, &n, 1)) return 66;
  svnicp::Cloud rows((size_t)n);
  if (n && !rd(fi, &rows[0][0], (size_t)3 * n)) return 66;
  if (!rd(fi, &C, 1)) return 66;
  std::vector<double> poses((size_t)12 * C);
  if (C && !rd(fi, poses.data(), poses.size())) return 66;
  const std::vector<double> out = map.ScorePoses(rows, poses, gate);
  fwrite(out.data(), sizeof(double), out.size(), fo);
  fclose(fo); fclose(fi);
  return 0;
}
