// map_state.hpp — host-only: the svnicp_map object and the pieces every entry point of voxel_map.hip states the same way
// (what prep_state.hpp is for svnicp_prep).  One stream per object; every buffer grows on demand and is reused across
// scans.  The members are grouped by the job that owns them; a job's launch chain sees its own group, never this object.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "device_buffer.hpp"
#include "map_normals.hpp"
#include "map_score.hpp"
#include "map_search.hpp"
#include "map_table.hpp"
#include "map_visibility.hpp"

// svnicp_map_score_poses: its poses, chunk records and results (the query's buffers are not touched)
struct MapScoreBufs {
  GrowBuf<double> poses, psum, out;
  GrowBuf<unsigned int> pcnt;
  int64_t C = 0;   // poses of the last scoring (0 before one)
};

// svnicp_map_search_poses: the lattice vectors, poses and records of EVERY level (the tap reads them), the kept lists
// (kSearchMaxKeep indices per level), its own chunk records, and the staging block the host reads with one copy
struct MapSearchBufs {
  GrowBuf<int32_t> lat, kept;
  GrowBuf<double> poses, rec, psum, stage;
  GrowBuf<unsigned int> pcnt;
  std::vector<double> host;       // the staging block of the last search, as map_search.hpp lays it out
  svnicp::MapSearchPlan plan{};   // the last search's lattice (done says whether there is one)
  bool done = false;              // does not depend on the table: a search's results outlive later changes of the map
};

struct svnicp_map {
  int device = 0;
  svnicp_host::Stream stream;   // before the buffers: destroyed after them
  double voxel = 1.0, max_range = 80.0;
  int max_points = 20;
  svnicp::MapTable table;
  svnicp::MapInsertScratch ins;
  svnicp::MapSelection sel;     // set by svnicp_map_query
  svnicp::MapNormals nrm;       // of sel's rows
  svnicp::MapVisibility vis;
  MapScoreBufs sc;
  MapSearchBufs se;
  GrowBuf<float> in;            // rows staged from host memory (stage_rows)
  GrowBuf<unsigned char> tmp;   // rocprim's scratch, shared by the sorts and the scan
  std::string err;
  static std::string& create_error() { thread_local std::string s; return s; }   // svnicp_map_last_error(nullptr)
};

namespace svnicp {

inline MapTableMut table_mut(svnicp_map* m) {
  return MapTableMut{m->table.keys.p, m->table.counts.p, m->table.pts.p, m->table.cap, m->max_points, (float)m->voxel, m->table.stats.p};
}
inline MapTableView table_view(svnicp_map* m) { return table_mut(m).view(); }

// every call that changes the map ends by reading the statistics: the live voxels are known without asking the device
inline int64_t known_live(const svnicp_map* m) { return m->table.h_stats[kStatLive] > 0 ? m->table.h_stats[kStatLive] : 0; }

// Everything derived from the table's contents stops describing it: the last query's selection and its normals.  Every
// call that changes the table starts with this — a stale selection would hand the solver stale normals with no error.
inline void drop_derived(svnicp_map* m) { m->sel.valid = false; m->nrm.M = 0; }

// 0 <= n <= 2^31-1 rows, and a pointer where there are any
inline bool rows_ok(const float* rows, int64_t n) { return n >= 0 && n <= 0x7fffffffLL && (n == 0 || rows); }

// The gate of the scoring and the search: the 3x3x3 block holds the nearest point only up to the voxel size.
inline bool gate_ok(const svnicp_map* m, double max_corr_dist) {
  return std::isfinite(max_corr_dist) && max_corr_dist > 0.0 && max_corr_dist <= m->voxel;
}
inline std::string gate_message(const char* fn) {
  return std::string(fn) + ": max_corr_dist must be finite, > 0 and <= voxel_size (the 3x3x3 block holds the nearest point only up to that gate)";
}

// rows[n][3] float32 -> where the kernels read them: the pointer itself for device memory, else a copy queued on the map's
// stream into the ONE staging buffer.  Sound because every entry point that stages rows synchronises the stream before it
// returns: no earlier call's rows are still being read when the next call overwrites them.
inline hipError_t stage_rows(svnicp_map* m, const float* rows, int64_t n, int mem_kind, const float** dev) {
  *dev = rows;
  if (n <= 0 || mem_kind == SVNICP_MEM_DEVICE) return hipSuccess;
  HIPTRY(m->in.ensure((size_t)n * 3));
  HIPTRY(hipMemcpyAsync(m->in.p, rows, (size_t)n * 12, hipMemcpyHostToDevice, m->stream));
  *dev = m->in.p;
  return hipSuccess;
}

}  // namespace svnicp
