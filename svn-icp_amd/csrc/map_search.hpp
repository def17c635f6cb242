// map_search.hpp — host-side interface of map_search.hip (svnicp_map_search_poses; the contract is in include/svnicp_hip.h,
// the design in DESIGN.md §4.17).  voxel_map.hip owns the map (map_state.hpp: MapSearchBufs) and calls these.  The lattice of a search --
// m, the active axes, the fine step, every level's count -- is planned here, once, on the host, before the first launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace svnicp {

constexpr int kSearchMaxLevels = 8;
constexpr int kSearchMaxKeep = 1024;                  // survivors of a level: they are ordered in LDS
constexpr int64_t kSearchMaxNodes = (int64_t)1 << 20; // per level, the limit of svnicp_map_score_poses
constexpr int kLatOff = 1 << 20;                      // lattice entries lie in (-2^20, 2^20): 21 bits each once offset
constexpr int kRankThreads = 1024;                    // k_map_search_rank: one workgroup

struct MapSearchGrid {   // passed to the kernels by value: nothing is uploaded between levels
  double G[12];          // the guess: R row-major, then t
  double fine[6];        // the finest lattice's step per axis (0 on an axis without a usable step)
  int m[6];              // level 0: j = -m..m per axis
  int active_mask;       // bit a: m[a] >= 1
  int children;          // 3^A
};

struct MapSearchPlan {
  MapSearchGrid grid;
  int levels, keep, active_axes;
  int64_t count[kSearchMaxLevels];   // nodes per level
  int64_t first[kSearchMaxLevels];   // the level's first node in the buffers that hold all levels
  int kept[kSearchMaxLevels];        // min(keep, count)
  int64_t total, max_count;
  int64_t zero_index;                // level 0's node of the zero correction
};

inline int64_t pow3(int e) { int64_t p = 1; while (e-- > 0) p *= 3; return p; }

// The limits of the contract -> nullptr, or the reason for the refusal.  The guess and the gate are the caller's to check.
inline const char* plan_map_search(const double extent[6], const double step[6], int levels, int keep, MapSearchPlan& P) {
  if (levels < 1 || levels > kSearchMaxLevels) return "need 1 <= levels <= 8";
  if (keep < 1 || keep > kSearchMaxKeep) return "need 1 <= keep <= 1024";
  const int64_t top = pow3(levels - 1);
  P.levels = levels; P.keep = keep; P.active_axes = 0;
  P.grid.active_mask = 0;
  int64_t c0 = 1, zero = 0;
  for (int a = 0; a < 6; ++a) {
    const double e = extent[a], s = step[a];
    if (!(std::isfinite(e) && e >= 0.0)) return "extents must be finite and >= 0";
    int64_t m = 0;
    if (e != 0.0) {
      if (!(std::isfinite(s) && s > 0.0)) return "an axis with a non-zero extent needs a finite step > 0";
      const double q = std::floor(e / s + 1e-9);
      if (!(q < (double)kLatOff)) return "lattice overflow: m * 3^(levels-1) + (3^(levels-1) - 1) / 2 must stay below 2^20";
      m = (int64_t)q;
    }
    if (m * top + (top - 1) / 2 >= (int64_t)kLatOff)
      return "lattice overflow: m * 3^(levels-1) + (3^(levels-1) - 1) / 2 must stay below 2^20";
    P.grid.m[a] = (int)m;
    P.grid.fine[a] = (std::isfinite(s) && s > 0.0) ? s / (double)top : 0.0;
    if (m >= 1) { P.grid.active_mask |= 1 << a; ++P.active_axes; }
    c0 *= 2 * m + 1;
    if (c0 > kSearchMaxNodes) return "a level holds more than 2^20 nodes";
    zero = zero * (2 * m + 1) + m;
  }
  P.grid.children = (int)pow3(P.active_axes);
  P.zero_index = zero;
  P.total = 0; P.max_count = 0;
  for (int l = 0; l < levels; ++l) {
    P.count[l] = l == 0 ? c0 : (int64_t)P.kept[l - 1] * P.grid.children;
    if (P.count[l] > kSearchMaxNodes) return "a level holds more than 2^20 nodes";
    P.kept[l] = (int)(P.count[l] < keep ? P.count[l] : keep);
    P.first[l] = P.total;
    P.total += P.count[l];
    if (P.count[l] > P.max_count) P.max_count = P.count[l];
  }
  return nullptr;
}

// doubles per kept node of the last level in the staging block: correction 6 | pose 12 | record 4; then 6 int32 of lattice
constexpr int kSearchTopDoubles = 22;
inline size_t map_search_stage_bytes(int n_top) { return (size_t)(4 + kSearchTopDoubles * n_top) * 8 + (size_t)n_top * 24; }

// Level `level` of the lattice: lat[count][6] and poses[count][12].  Level 0 comes from grid.m; a later level from the kept
// list (indices into parent_lat, in rank order) of the level before.
hipError_t launch_map_search_nodes(const MapSearchGrid& grid, int level, int levels, int64_t count, const int32_t* parent_lat,
                                   const int32_t* parent_kept, int32_t* lat, double* poses, hipStream_t stream);
// The `kept` smallest of rec[count][4] by (cost, lattice lexicographic) as indices in rank order; 1 <= kept <= min(count, 1024).
hipError_t launch_map_search_rank(const double* rec, const int32_t* lat, int64_t count, int kept, int32_t* kept_out, hipStream_t stream);
// The staging block the host reads with one copy: zero_rec | per kept node of the last level {correction, pose, record} | lattices.
hipError_t launch_map_search_gather(const MapSearchGrid& grid, const int32_t* lat, const double* poses, const double* rec,
                                    const int32_t* kept, int n_top, const double* zero_rec, double* stage, hipStream_t stream);

}  // namespace svnicp
