// map_score.hpp — host-side interface of map_score.hip (svnicp_map_score_poses; the contract is in include/svnicp_hip.h, the
// design in DESIGN.md §4.16).  voxel_map.hip owns the map (map_state.hpp: MapScoreBufs) and calls these.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "map_table.hpp"   // MapTableView

namespace svnicp {

constexpr int kScoreRows = 256;          // source rows per workgroup: one per thread, whatever n and C are
constexpr int kScorePoseBatch = 32768;   // poses per launch (the grid's y extent is limited to 65535)

inline int64_t map_score_chunks(int64_t n) { return (n + kScoreRows - 1) / kScoreRows; }

// Queues the scoring of poses [0, C) on `stream`: rows src[n][3] (device), poses[C][12] (device), out[C][4] (device).
// part_cnt holds 2 * min(C, kScorePoseBatch) * chunks entries and part_sum half as many; both are unused with one chunk.
hipError_t launch_map_score(const MapTableView& T, const float* src, int64_t n, const double* poses, int64_t C, double thr2,
                            unsigned int* part_cnt, double* part_sum, double* out, hipStream_t stream);

}  // namespace svnicp
