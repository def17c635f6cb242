// map_visibility.hpp — host-side interface of map_visibility.hip (svnicp_map_clear_seen_through; the contract is in
// include/svnicp_hip.h, the design in DESIGN.md §4.15): drop the stored points a new scan sees through.
#pragma once
#include "map_table.hpp"
#include "range_project_device.hpp"

namespace svnicp {

struct VisOpt { int wr, wc; float margin_abs, margin_rel, max_range; };

enum VisStat : int { kVisPixelsFilled = 0, kVisPointsTested = 1, kVisPointsRemoved = 2, kVisVoxelsEmptied = 3, kVisStats = 4 };

struct MapVisibility {
  GrowBuf<unsigned int> img;           // the minimum-range image (float bit patterns), [N][H]
  GrowBuf<unsigned long long> stats;   // the call's statistics, [kVisStats]
};

// Queues the whole pass on `stream`: fill -> select every live voxel -> range image of scan[n][3] (device, sensor frame) ->
// clear.  `live` > 0 is the number of live voxels the host knows; the selection's key / slot / nsel are scratch here (the
// caller has dropped the selection: the table changes).  V.stats holds the call's statistics once the stream has drained.
hipError_t launch_map_clear_seen_through(const MapTableMut& T, const float* scan, int64_t n, const MapPose& pose, const RangeSensor& S,
                                         const VisOpt& O, int64_t live, MapSelection& sel, MapVisibility& V, hipStream_t stream);

}  // namespace svnicp
