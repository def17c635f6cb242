// map_visibility_driver.cpp — runs the header-only C++ visibility clearing (svn-icp_amd/host/registration_pipeline.hpp:
// VoxelHashMap::ClearSeenThrough) on a file of map points and a scan; tests/test_map_visibility_cpu.py compares it with pipeline.py.
//   map_visibility_driver in.bin out.bin
// in.bin : svnicp_seg_params, svnicp_visibility_opt, f64 voxel_size, f64 map_range, int32 max_points, f64 R[9] (row-major), f64 t[3],
//          int32 m, m x 3 float32 map points (inserted with the identity pose), int32 n, n x 3 float32 scan (sensor frame)
// out.bin: int64 pixels_filled, points_tested, points_removed, voxels_emptied, int64 voxels, int64 k, k x 3 float32: the map after
//          the call, voxels in ascending index, points of a voxel in their order
#include <cstdio>
#include <vector>

#include "registration_pipeline.hpp"

template <typename T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 64; }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) { perror("open"); return 65; }
  svnicp_seg_params sensor;
  svnicp_visibility_opt opt;
  double voxel = 0, range = 0;
  int32_t max_points = 0, m = 0, n = 0;
  svnicp::Pose3 pose;
  if (!rd(fi, &sensor, 1) || !rd(fi, &opt, 1) || !rd(fi, &voxel, 1) || !rd(fi, &range, 1) || !rd(fi, &max_points, 1) ||
      !rd(fi, pose.R.data(), 9) || !rd(fi, pose.t.data(), 3) || !rd(fi, &m, 1))
    return 66;
  svnicp::Cloud stored((size_t)m);
  if (m && !rd(fi, &stored[0][0], (size_t)3 * m)) return 66;
  if (!rd(fi, &n, 1)) return 66;
  svnicp::Cloud scan((size_t)n);
  if (n && !rd(fi, &scan[0][0], (size_t)3 * n)) return 66;
  svnicp::VoxelHashMap map(voxel, range, max_points);
  map.AddPointCloud(stored, svnicp::Pose3{});
  const svnicp_visibility_stats st = map.ClearSeenThrough(scan, pose, sensor, opt);
  const svnicp::Cloud left = map.GetMap();
  const int64_t head[6] = {st.pixels_filled, st.points_tested, st.points_removed, st.voxels_emptied, (int64_t)map.Size(), (int64_t)left.size()};
  fwrite(head, sizeof(int64_t), 6, fo);
  if (!left.empty()) fwrite(&left[0][0], sizeof(float), 3 * left.size(), fo);
  fclose(fo); fclose(fi);
  return 0;
}
