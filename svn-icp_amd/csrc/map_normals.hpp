// map_normals.hpp — host-side interface of map_normals.hip (svnicp_map_query_normals; the contract is in include/svnicp_hip.h,
// the design in DESIGN.md §4.4): the normals of a query's rows from the 27-voxel blocks of the map.
#pragma once
#include "map_table.hpp"

namespace svnicp {

struct MapNormals {
  GrowBuf<double> rows;  // [M][3], row for row with the selection's `out`; a zero row means no normal
  int64_t M = 0;         // rows that belong to the last query (0 until the normals were computed for it)
};

// Once per process and size class, at map creation: k_map_normals' dynamic LDS above 48 KB has to be asked for.
hipError_t map_normals_prepare(int max_points);
// Queues the normals of S's rows (S valid, last_M > 0) into out[last_M][3] from normal_k neighbours each; *with_normal
// (device; cleared here) counts the rows that got one.
hipError_t launch_map_normals(const MapTableView& T, const MapSelection& S, int normal_k, double* out, int* with_normal,
                              hipStream_t stream);

}  // namespace svnicp
