// map_table.hpp — host-side interface of map_table.hip: the voxel map's hash table (layout and determinism: voxel_map.hip's
// header comment; design: DESIGN.md §4.4), its views as the kernels take them, the buffers of each of its jobs grouped by
// owner, and its launch chains.  Like map_score.hpp, everything here takes plain views, owners and a stream and returns
// hipError_t; voxel_map.hip owns the svnicp_map object, checks arguments and turns errors into the C ABI's codes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "device_buffer.hpp"

namespace svnicp {

// the four statistics words of a table, on the device (MapTable::stats) and as the host last read them (MapTable::h_stats)
enum MapStat : int {
  kStatLive = 0,      // live voxels
  kStatTombs = 1,     // tombstones since the last rebuild
  kStatFlags = 2,     // kFlagTableFull
  kStatSkipped = 3,   // points of the last insertion outside the index range or NaN
  kMapStats = 4
};
constexpr int kFlagTableFull = 2;              // kStatFlags: a probe sequence went round a full table
constexpr unsigned int kNoSlot = 0xffffffffu;  // slot of a point that is not stored; sorts behind every real slot

struct MapPose { double R[9]; double t[3]; };   // map <- sensor, passed to the kernels by value
inline MapPose map_pose(const double R_rowmajor[9], const double t[3]) {
  MapPose p;
  for (int i = 0; i < 9; ++i) p.R[i] = R_rowmajor[i];
  for (int i = 0; i < 3; ++i) p.t[i] = t[i];
  return p;
}

struct MapTableView {   // the table as the kernels read it
  const unsigned long long* keys;
  const int* counts;
  const float* pts;
  int64_t cap;
  int max_points;
  float voxel;
};

struct MapTableMut {   // the table as the kernels that change it take it
  unsigned long long* keys;
  int* counts;
  float* pts;
  int64_t cap;
  int max_points;
  float voxel;
  int* stats;   // [kMapStats]
  MapTableView view() const { return MapTableView{keys, counts, pts, cap, max_points, voxel}; }
};

struct MapTable {   // keys[cap] | counts[cap] | pts[cap][max_points][3], and the statistics
  GrowBuf<unsigned long long> keys;
  GrowBuf<int> counts;
  GrowBuf<float> pts;
  int64_t cap = 0;
  GrowBuf<int> stats;
  int h_stats[kMapStats] = {0, 0, 0, 0};   // as of the last call that changed the map: each ends by reading them
  int64_t rebuilds = 0;   // map_table_rebuild calls since creation
  int64_t skipped = 0;    // points no insertion stored (outside the index range or NaN), since creation / clear
};

struct MapInsertScratch {   // per point of the cloud being inserted
  GrowBuf<float> q;                  // transformed points
  GrowBuf<unsigned int> slot, sslot; // slot of each point; sorted
  GrowBuf<int> sidx_in, sidx;        // input index; sorted along
};

// A query's selection: the voxels it took in ascending key (key2 / slot2 / cnt / off over last_live entries; entries the
// selection did not fill have the key ~0 and count zero) and their rows.  `valid`: it still describes the table.
struct MapSelection {
  GrowBuf<unsigned long long> key, key2;
  GrowBuf<unsigned int> slot, slot2;
  GrowBuf<int> cnt, off;
  GrowBuf<int> nsel;     // one counter on the device: k_map_select's; between queries free for the jobs that read the selection
  GrowBuf<double> out;   // float64 rows [last_M][3]
  int64_t last_M = 0, last_live = 0;
  bool valid = false;
};

#define HIPTRY(expr)                         \
  do {                                       \
    const hipError_t e_ = (expr);            \
    if (e_ != hipSuccess) return e_;         \
  } while (0)

// every kernel launch of the map goes through here: each is followed by its own hipGetLastError
template <typename Kernel, typename... Args>
inline hipError_t launch_checked(Kernel kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
  return hipGetLastError();
}
inline unsigned blocks_of(int64_t n, int per_block = 256) { return (unsigned)((n + per_block - 1) / per_block); }

// (Re)allocates T for `cap` slots (a power of two) and queues its clearing; the statistics are not touched.
hipError_t map_table_alloc(MapTable& T, int64_t cap, int max_points, hipStream_t stream);
// Empties the table and every counter, on the device and on the host; capacity and rebuild count stay.  Synchronises.
hipError_t map_table_clear(MapTable& T, hipStream_t stream);
// T.h_stats <- T.stats.  Synchronises.
hipError_t map_table_read_stats(MapTable& T, hipStream_t stream);
// Room for n more points in the worst case (every point a new voxel): keeps the load factor below 1/2 and rebuilds, at the
// same capacity, once a quarter of the slots are tombstones.  Synchronises.
hipError_t map_table_reserve(MapTable& T, int max_points, int64_t n, hipStream_t stream);
// Re-inserts every live voxel into a fresh table of new_cap slots: no tombstones afterwards.  Synchronises.
hipError_t map_table_rebuild(MapTable& T, int max_points, int64_t new_cap, hipStream_t stream);
// Queues the insertion of in[n][3] (device, n > 0) at `pose`: locate -> iota -> stable radix sort -> place -> count.
hipError_t map_table_insert(const MapTableMut& T, const float* in, int64_t n, const MapPose& pose, MapInsertScratch& S,
                            GrowBuf<unsigned char>& tmp, hipStream_t stream);
// Queues RemoveFarPointCloud: every voxel whose first point is farther than sqrt(r2) from `centre` becomes a tombstone.
hipError_t launch_map_remove_far(const MapTableMut& T, const double centre[3], double r2, hipStream_t stream);
// After map_table_read_stats: adds the insertion's skipped points to T.skipped, clears that word and the flags on the device
// and returns the flags.  Synchronises if either was set.
hipError_t map_table_take_flags(MapTable& T, hipStream_t stream, int* flags);
// Queues the selection of the voxels whose first point is closer than sqrt(r2) to (px, py, pz) (r2 < 0: every voxel), in any
// order, at sel_key / sel_slot [0, *nsel); at most `limit` entries are written.
hipError_t launch_map_select(const MapTableView& T, double px, double py, double pz, double r2, unsigned long long* sel_key,
                             unsigned int* sel_slot, int* nsel, int limit, hipStream_t stream);
// GetMap: select + sort + counts + scan + gather into S (sized by `live` > 0, the live voxels the host knows) -> rows.
// Synchronises: the rows are complete when it returns.
hipError_t map_table_query(const MapTableView& T, double px, double py, double pz, double r2, size_t live, MapSelection& S,
                           GrowBuf<unsigned char>& tmp, hipStream_t stream, int64_t* rows);

}  // namespace svnicp
