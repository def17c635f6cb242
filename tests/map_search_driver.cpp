// map_search_driver.cpp — runs the header-only C++ coarse-to-fine search (svn-icp_amd/host/registration_pipeline.hpp:
// VoxelHashMap::SearchPoses) on a file of map clouds, scan rows and a search; tests/test_map_search_cpu.py compares it with
// pipeline.py.
//   map_search_driver in.bin out.bin
// in.bin : f64 voxel_size, f64 map_range, int32 max_points, f64 gate, int32 steps, per step { f64 R[9] (row-major), f64 t[3], int32 m, m x 3 float32 },
//          int32 n, n x 3 float32 scan rows (sensor frame), f64 guess R[9], t[3], f64 extent[6], step[6], int32 levels, keep
// out.bin: int32 levels, active_axes; per level { int64 count, int32 kept, count x 6 int32 lattice, count x 4 f64 records, kept x int32 indices };
//          int32 best_lattice[6], f64 best_correction[6], best_record[4], zero_record[4], fine_step[6]
#include <cstdio>
#include <vector>

#include "registration_pipeline.hpp"

template <typename T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <typename T> static void wr(FILE* f, const T* p, size_t n) { fwrite(p, sizeof(T), n, f); }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 64; }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) { perror("open"); return 65; }
  double voxel = 0, range = 0, gate = 0;
  int32_t max_points = 0, steps = 0, n = 0, levels = 0, keep = 0;
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
  svnicp::Pose3 guess;
  std::array<double, 6> extent{}, step{};
  if (!rd(fi, guess.R.data(), 9) || !rd(fi, guess.t.data(), 3) || !rd(fi, extent.data(), 6) || !rd(fi, step.data(), 6) || !rd(fi, &levels, 1) ||
      !rd(fi, &keep, 1))
    return 66;
  try {
    const svnicp::MapSearchResult r = map.SearchPoses(rows, guess, extent, step, levels, keep, gate);
    const int32_t head[2] = {r.levels, r.active_axes};
    wr(fo, head, 2);
    for (const auto& lv : r.level) {
      const int64_t count = (int64_t)lv.lattice.size();
      const int32_t kept = (int32_t)lv.kept.size();
      wr(fo, &count, 1); wr(fo, &kept, 1);
      wr(fo, &lv.lattice[0][0], (size_t)6 * count); wr(fo, lv.records.data(), lv.records.size()); wr(fo, lv.kept.data(), lv.kept.size());
    }
    wr(fo, r.best_lattice.data(), 6); wr(fo, r.best_correction.data(), 6); wr(fo, r.best_record.data(), 4); wr(fo, r.zero_record.data(), 4);
    wr(fo, r.fine_step.data(), 6);
  } catch (const std::invalid_argument& e) {
    fprintf(stderr, "refused: %s\n", e.what());
    return 2;
  }
  fclose(fo); fclose(fi);
  return 0;
}
