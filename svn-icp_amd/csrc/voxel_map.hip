// voxel_map.hip — the local map of the scan-to-map loop, resident in HBM: the svnicp_map_* surface of the C ABI.
//
// SURVEY.md §8(f)-4 (second half).  Device counterpart of svnicp::VoxelHashMap
// (the reference's src/core/VoxelHashMap.cpp:22-101, include/core/VoxelHashMap.h): a hash map
// voxel -> at most max_points points in insertion order, with
//   AddPointCloud(cloud, pose)  (:22-42)  transform by the pose (float32 like pcl::PointXYZ), voxel index = coordinates /
//                                          voxel_size truncated toward zero (:29), append while the voxel has room, then
//   RemoveFarPointCloud(pos)    (:89-97)  drop every voxel whose FIRST point is farther than max_range,
//   GetMap(pose, r) / GetMap()  (:44-58)  all points of the voxels whose first point is closer than r (or of all voxels).
// Not in the reference: the normals of a query's rows from the map's own voxels (svnicp_map_query_normals), the
// visibility-based clearing of stored points a new scan sees through (svnicp_map_clear_seen_through), the scoring of candidate
// poses (svnicp_map_score_poses) and the coarse-to-fine search over them (svnicp_map_search_poses).
// The reference keeps it in a tsl::robin_map on the host and re-uploads the query result for every scan
// (OdometryPipeline.cpp:577-582); here the table lives in HBM and a query writes float64 rows straight into a device
// buffer the solver copies device-to-device (svnicp_set_target, SVNICP_MEM_DEVICE) — per scan only the new points go over
// PCIe.
//
// Layout: open addressing, linear probing; keys[cap] = packed voxel index (3 x 21 bits, offset 2^20) or EMPTY / TOMB;
// counts[cap]; pts[cap][max_points] float3.  Determinism: a point's slot is found (or created by atomicCAS) in parallel,
// but WHICH points a voxel keeps is decided in input order — the (slot, input index) pairs are radix-sorted (stable), a
// point's rank inside its voxel is its position in the sorted run, and it is stored at counts[slot] + rank if that is
// below max_points: exactly the points the sequential loop of the reference keeps, in the same order.  A query emits
// voxels in ascending (x, y, z) voxel index (radix sort of the selected keys), so the output is reproducible and equals
// the ordered host map of svn-icp_amd/host/registration_pipeline.hpp point for point.
//
// This file holds the entry points only: argument checks, the object's bookkeeping and the copies to the host.  The object
// and the checks every entry point shares are in map_state.hpp; the kernels and their launch chains are in
//   map_table.hip       the table: insert, remove-far, select / gather (query), rebuild
//   map_normals.hip     normals of a query's rows
//   map_visibility.hip  visibility-based clearing
//   map_score.hip       pose scoring
//   map_search.hip      the coarse-to-fine search
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/svnicp_hip.h"
#include "map_state.hpp"

using namespace svnicp;

namespace {

int create_table(svnicp_map* m, int64_t cap) {
  HIPCHK(m, map_table_alloc(m->table, cap, m->max_points, m->stream));
  return 0;
}

// the first min(M, cap_points) of rows[M][3] to the host; *n_out = M
int download_rows(svnicp_map* m, const double* rows, int64_t M, double* out_xyz, int64_t cap_points, int64_t* n_out) {
  HIPCHK(m, hipSetDevice(m->device));
  *n_out = M;
  const int64_t n = M < cap_points ? M : cap_points;
  if (n > 0 && out_xyz) {
    HIPCHK(m, hipMemcpyAsync(out_xyz, rows, (size_t)n * 24, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
  }
  return SVNICP_OK;
}

}  // namespace

extern "C" {

const char* svnicp_map_last_error(const svnicp_map* m) { return m ? m->err.c_str() : svnicp_map::create_error().c_str(); }

int svnicp_map_create(int device, double voxel_size, double max_range, int max_points, int64_t capacity_voxels, svnicp_map** out) {
  if (!out || !(voxel_size > 0) || max_points < 1 || max_points > 256)
    return fail<svnicp_map>(nullptr, SVNICP_ERR_INVALID, "svnicp_map_create: need voxel_size > 0 and 1 <= max_points <= 256");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail<svnicp_map>(nullptr, SVNICP_ERR_NO_DEVICE, "svnicp_map_create: no HIP device visible (this library has no CPU path)");
  if (device < 0 || device >= ndev) return fail<svnicp_map>(nullptr, SVNICP_ERR_INVALID, "svnicp_map_create: bad device ordinal");
  if (hipSetDevice(device) != hipSuccess) return fail<svnicp_map>(nullptr, SVNICP_ERR_HIP, "hipSetDevice failed");
  svnicp_map* m = new svnicp_map();
  m->device = device; m->voxel = voxel_size; m->max_range = max_range; m->max_points = max_points;
  int64_t cap = 1 << 16;
  const int64_t want = capacity_voxels > 0 ? capacity_voxels : (int64_t)1 << 20;
  while (cap < want) cap <<= 1;
  if (m->stream.create(hipStreamNonBlocking) != hipSuccess) { delete m; return fail<svnicp_map>(nullptr, SVNICP_ERR_HIP, "hipStreamCreate failed"); }
  int rc = create_table(m, cap);
  if (!rc && (m->table.stats.ensure(kMapStats) != hipSuccess || m->sel.nsel.ensure(1) != hipSuccess)) rc = SVNICP_ERR_NOMEM;
  if (!rc && hipMemsetAsync(m->table.stats.p, 0, kMapStats * sizeof(int), m->stream) != hipSuccess) rc = SVNICP_ERR_HIP;
  if (!rc && hipStreamSynchronize(m->stream) != hipSuccess) rc = SVNICP_ERR_HIP;
  if (!rc && map_normals_prepare(max_points) != hipSuccess) rc = SVNICP_ERR_HIP;
  if (rc) { svnicp_map::create_error() = m->err.empty() ? "svnicp_map_create: allocation failed" : m->err; svnicp_map_destroy(m); return rc; }
  *out = m;
  return SVNICP_OK;
}

void svnicp_map_destroy(svnicp_map* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  delete m;
}

int svnicp_map_clear(svnicp_map* m) {
  if (!m) return SVNICP_ERR_INVALID;
  HIPCHK(m, hipSetDevice(m->device));
  HIPCHK(m, map_table_clear(m->table, m->stream));
  drop_derived(m);
  return SVNICP_OK;
}

int svnicp_map_skipped_points(svnicp_map* m, int64_t* out) {
  if (!m || !out) return SVNICP_ERR_INVALID;
  *out = m->table.skipped;
  return SVNICP_OK;
}

int svnicp_map_table_info(svnicp_map* m, int64_t* capacity_slots, int64_t* tombstones, int64_t* rebuilds) {
  if (!m) return SVNICP_ERR_INVALID;
  if (capacity_slots) *capacity_slots = m->table.cap;
  if (tombstones) *tombstones = m->table.h_stats[kStatTombs];
  if (rebuilds) *rebuilds = m->table.rebuilds;
  return SVNICP_OK;
}

int svnicp_map_size(svnicp_map* m, int64_t* voxels) {
  if (!m || !voxels) return SVNICP_ERR_INVALID;
  HIPCHK(m, hipSetDevice(m->device));
  HIPCHK(m, map_table_read_stats(m->table, m->stream));
  *voxels = m->table.h_stats[kStatLive];
  return SVNICP_OK;
}

int svnicp_map_add_cloud(svnicp_map* m, const float* xyz, int64_t n, int mem_kind, const double R_rowmajor[9], const double t[3]) {
  if (!m || !R_rowmajor || !t || !rows_ok(xyz, n)) return fail(m, SVNICP_ERR_INVALID, "svnicp_map_add_cloud: bad argument");
  HIPCHK(m, hipSetDevice(m->device));
  drop_derived(m);
  if (n > 0) {
    HIPCHK(m, map_table_reserve(m->table, m->max_points, n, m->stream));
    const float* din = nullptr;
    HIPCHK(m, stage_rows(m, xyz, n, mem_kind, &din));
    HIPCHK(m, map_table_insert(table_mut(m), din, n, map_pose(R_rowmajor, t), m->ins, m->tmp, m->stream));
  }
  HIPCHK(m, launch_map_remove_far(table_mut(m), t, m->max_range * m->max_range, m->stream));
  HIPCHK(m, map_table_read_stats(m->table, m->stream));
  int flags = 0;
  HIPCHK(m, map_table_take_flags(m->table, m->stream, &flags));
  // cannot happen: the table is grown to twice the voxels this cloud could add before anything is inserted
  if (flags & kFlagTableFull) return fail(m, SVNICP_ERR_NOMEM, "svnicp_map_add_cloud: hash table full");
  return SVNICP_OK;
}

int svnicp_map_clear_seen_through(svnicp_map* m, const float* scan_xyz, int64_t n, int mem_kind, const double R_rowmajor[9], const double t[3],
                                  const svnicp_seg_params* sensor, const svnicp_visibility_opt* opt, svnicp_visibility_stats* out) {
  if (!m) return SVNICP_ERR_INVALID;
  if (!R_rowmajor || !t || !sensor || !opt || !out || !rows_ok(scan_xyz, n))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_clear_seen_through: bad argument");
  if (sensor->struct_size != (int32_t)sizeof(svnicp_seg_params) || opt->struct_size != (int32_t)sizeof(svnicp_visibility_opt))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_clear_seen_through: struct_size != sizeof(svnicp_seg_params) / sizeof(svnicp_visibility_opt)");
  if (!(sensor->n_scan >= 1 && sensor->n_scan <= 128 && sensor->horizon_scan >= 1 &&
        (int64_t)sensor->n_scan * sensor->horizon_scan <= (int64_t)1 << 19))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_clear_seen_through: need 1 <= n_scan <= 128, horizon_scan >= 1 and n_scan * horizon_scan <= 2^19");
  if (!(std::isfinite(sensor->ang_res_x) && sensor->ang_res_x > 0.0f && std::isfinite(sensor->ang_res_y) && sensor->ang_res_y > 0.0f &&
        std::isfinite(sensor->ang_bottom) && std::isfinite(sensor->min_range)))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_clear_seen_through: ang_res_x / ang_res_y must be finite and positive, ang_bottom / min_range finite");
  if (!(opt->window_rows >= 0 && opt->window_rows <= 4 && opt->window_cols >= 0 && opt->window_cols <= 8))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_clear_seen_through: window_rows must be 0..4 and window_cols 0..8");
  if (!(std::isfinite(opt->margin_abs) && opt->margin_abs >= 0.0f && std::isfinite(opt->margin_rel) && opt->margin_rel >= 0.0f))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_clear_seen_through: margin_abs / margin_rel must be finite and >= 0");
  if (!(std::isfinite(opt->max_range) && opt->max_range > 0.0f))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_clear_seen_through: max_range must be finite and > 0");
  HIPCHK(m, hipSetDevice(m->device));
  drop_derived(m);
  *out = svnicp_visibility_stats{0, 0, 0, 0};
  const int64_t live = known_live(m);
  if (n == 0 || live == 0) return SVNICP_OK;
  const RangeSensor S{sensor->n_scan, sensor->horizon_scan, sensor->ang_res_x, sensor->ang_res_y, sensor->ang_bottom, sensor->min_range};
  const VisOpt O{opt->window_rows, opt->window_cols, opt->margin_abs, opt->margin_rel, opt->max_range};
  const float* din = nullptr;
  HIPCHK(m, stage_rows(m, scan_xyz, n, mem_kind, &din));
  HIPCHK(m, launch_map_clear_seen_through(table_mut(m), din, n, map_pose(R_rowmajor, t), S, O, live, m->sel, m->vis, m->stream));
  unsigned long long vs[kVisStats] = {0, 0, 0, 0};
  HIPCHK(m, hipMemcpyAsync(vs, m->vis.stats.p, sizeof vs, hipMemcpyDeviceToHost, m->stream));
  // the only host synchronisation: live voxels and tombstones as the next call needs them
  HIPCHK(m, map_table_read_stats(m->table, m->stream));
  out->pixels_filled = (int64_t)vs[kVisPixelsFilled]; out->points_tested = (int64_t)vs[kVisPointsTested];
  out->points_removed = (int64_t)vs[kVisPointsRemoved]; out->voxels_emptied = (int64_t)vs[kVisVoxelsEmptied];
  return SVNICP_OK;
}

int svnicp_map_query(svnicp_map* m, const double center[3], double max_range, int64_t* count_out) {
  if (!m || !count_out) return SVNICP_ERR_INVALID;
  HIPCHK(m, hipSetDevice(m->device));
  const double r2 = (center && max_range >= 0.0) ? max_range * max_range : -1.0;
  const double c0 = center ? center[0] : 0.0, c1 = center ? center[1] : 0.0, c2 = center ? center[2] : 0.0;
  const int64_t live = known_live(m);
  *count_out = 0;
  drop_derived(m);
  m->sel.last_M = 0; m->sel.last_live = live;
  if (live > 0) HIPCHK(m, map_table_query(table_view(m), c0, c1, c2, r2, (size_t)live, m->sel, m->tmp, m->stream, &m->sel.last_M));
  m->sel.valid = true;
  *count_out = m->sel.last_M;
  return SVNICP_OK;
}

int svnicp_map_query_normals(svnicp_map* m, int normal_k, int64_t* with_normal_out) {
  if (!m) return SVNICP_ERR_INVALID;
  if (with_normal_out) *with_normal_out = 0;
  if (!m->sel.valid)
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_query_normals: no svnicp_map_query yet, or the map changed (add_cloud / clear_seen_through / clear) since the last one");
  const int kn = normal_k ? normal_k : 16;
  if (kn < 4 || kn > 64) return fail(m, SVNICP_ERR_INVALID, "svnicp_map_query_normals: normal_k must be 4..64 (0 = 16)");
  HIPCHK(m, hipSetDevice(m->device));
  m->nrm.M = 0;
  if (m->sel.last_M == 0) return SVNICP_OK;   // an empty selection: nothing to write
  HIPCHK(m, m->nrm.rows.ensure((size_t)m->sel.last_M * 3));
  int* counter = m->sel.nsel.p;   // the query's counter, free again: here the rows with a normal
  HIPCHK(m, launch_map_normals(table_view(m), m->sel, kn, m->nrm.rows.p, counter, m->stream));
  int with = 0;
  HIPCHK(m, hipMemcpyAsync(&with, counter, sizeof(int), hipMemcpyDeviceToHost, m->stream));
  HIPCHK(m, hipStreamSynchronize(m->stream));   // complete when the call returns, like the query
  m->nrm.M = m->sel.last_M;
  if (with_normal_out) *with_normal_out = with;
  return SVNICP_OK;
}

void* svnicp_map_normals_devptr(svnicp_map* m) { return m && m->nrm.M > 0 ? (void*)m->nrm.rows.p : nullptr; }

int svnicp_map_download_normals(svnicp_map* m, double* out_xyz, int64_t cap_points, int64_t* n_out) {
  if (!m || !n_out) return SVNICP_ERR_INVALID;
  return download_rows(m, m->nrm.rows.p, m->nrm.M, out_xyz, cap_points, n_out);
}

int svnicp_map_score_poses(svnicp_map* m, const float* src_xyz, int64_t n, int src_mem_kind, const double* posesCx12, int64_t C,
                           int poses_mem_kind, double max_corr_dist, double* outCx4) {
  if (!m) return SVNICP_ERR_INVALID;
  if (!rows_ok(src_xyz, n)) return fail(m, SVNICP_ERR_INVALID, "svnicp_map_score_poses: need 0 <= n <= 2^31-1 and rows for n > 0");
  if (!posesCx12 || C < 1 || C > ((int64_t)1 << 20))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_score_poses: need poses and 1 <= C <= 2^20");
  if (!gate_ok(m, max_corr_dist)) return fail(m, SVNICP_ERR_INVALID, gate_message("svnicp_map_score_poses"));
  HIPCHK(m, hipSetDevice(m->device));
  const double thr2 = max_corr_dist * max_corr_dist;
  MapScoreBufs& B = m->sc;
  const float* din = nullptr;
  HIPCHK(m, stage_rows(m, src_xyz, n, src_mem_kind, &din));
  const double* dposes = posesCx12;
  if (poses_mem_kind != SVNICP_MEM_DEVICE) {
    HIPCHK(m, B.poses.ensure((size_t)C * 12));
    HIPCHK(m, hipMemcpyAsync(B.poses.p, posesCx12, (size_t)C * 96, hipMemcpyHostToDevice, m->stream));
    dposes = B.poses.p;
  }
  const int64_t chunks = map_score_chunks(n);
  const size_t recs = (size_t)(C < kScorePoseBatch ? C : kScorePoseBatch) * (size_t)chunks;
  B.C = 0;
  HIPCHK(m, B.out.ensure((size_t)C * SVNICP_MAP_SCORE_FIELDS));
  HIPCHK(m, B.pcnt.ensure(2 * recs)); HIPCHK(m, B.psum.ensure(recs));
  HIPCHK(m, launch_map_score(table_view(m), din, n, dposes, C, thr2, B.pcnt.p, B.psum.p, B.out.p, m->stream));
  if (outCx4) HIPCHK(m, hipMemcpyAsync(outCx4, B.out.p, (size_t)C * SVNICP_MAP_SCORE_FIELDS * 8, hipMemcpyDeviceToHost, m->stream));
  HIPCHK(m, hipStreamSynchronize(m->stream));   // complete when the call returns: the caller's rows and poses are free again
  B.C = C;
  return SVNICP_OK;
}

void* svnicp_map_scores_devptr(svnicp_map* m) { return m && m->sc.C > 0 ? (void*)m->sc.out.p : nullptr; }

int svnicp_map_search_poses(svnicp_map* m, const float* src_xyz, int64_t n, int src_mem_kind, const double* guess_R, const double* guess_t,
                            const svnicp_map_search_opt* opt, svnicp_map_search* out) {
  if (!m) return SVNICP_ERR_INVALID;
  if (!guess_R || !guess_t || !opt || !out)
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_search_poses: guess_R, guess_t, opt and out must not be NULL");
  if (!rows_ok(src_xyz, n)) return fail(m, SVNICP_ERR_INVALID, "svnicp_map_search_poses: need 0 <= n <= 2^31-1 and rows for n > 0");
  if (!gate_ok(m, opt->max_corr_dist)) return fail(m, SVNICP_ERR_INVALID, gate_message("svnicp_map_search_poses"));
  MapSearchPlan P{};
  if (const char* why = plan_map_search(opt->extent, opt->step, opt->levels, opt->keep, P))
    return fail(m, SVNICP_ERR_INVALID, std::string("svnicp_map_search_poses: ") + why);
  for (int j = 0; j < 12; ++j) {
    P.grid.G[j] = j < 9 ? guess_R[j] : guess_t[j - 9];
    if (!std::isfinite(P.grid.G[j])) return fail(m, SVNICP_ERR_INVALID, "svnicp_map_search_poses: the guess must be finite");
  }
  HIPCHK(m, hipSetDevice(m->device));
  MapSearchBufs& B = m->se;
  B.done = false;
  const double thr2 = opt->max_corr_dist * opt->max_corr_dist;
  const float* din = nullptr;
  HIPCHK(m, stage_rows(m, src_xyz, n, src_mem_kind, &din));
  // every buffer at its final size before the first launch: growing one would drop the levels it already holds
  const int64_t chunks = map_score_chunks(n);
  const size_t recs = (size_t)(P.max_count < kScorePoseBatch ? P.max_count : kScorePoseBatch) * (size_t)chunks;
  const int n_top = P.kept[P.levels - 1];
  const size_t stage_bytes = map_search_stage_bytes(n_top);
  HIPCHK(m, B.lat.ensure((size_t)P.total * 6));
  HIPCHK(m, B.poses.ensure((size_t)P.total * 12));
  HIPCHK(m, B.rec.ensure((size_t)P.total * SVNICP_MAP_SCORE_FIELDS));
  HIPCHK(m, B.kept.ensure((size_t)kSearchMaxLevels * kSearchMaxKeep));
  HIPCHK(m, B.pcnt.ensure(2 * recs)); HIPCHK(m, B.psum.ensure(recs));
  HIPCHK(m, B.stage.ensure(stage_bytes / 8));
  HIPCHK(m, hipMemsetAsync(B.kept.p, 0, (size_t)kSearchMaxLevels * kSearchMaxKeep * 4, m->stream));
  const MapTableView T = table_view(m);
  for (int l = 0; l < P.levels; ++l) {   // per level: nodes, score (one or two launches per 32768 poses), rank
    int32_t* lat = B.lat.p + 6 * P.first[l];
    double* poses = B.poses.p + 12 * P.first[l];
    double* rec = B.rec.p + SVNICP_MAP_SCORE_FIELDS * P.first[l];
    int32_t* kept = B.kept.p + (size_t)l * kSearchMaxKeep;
    HIPCHK(m, launch_map_search_nodes(P.grid, l, P.levels, P.count[l], l ? B.lat.p + 6 * P.first[l - 1] : nullptr,
                                      l ? kept - kSearchMaxKeep : nullptr, lat, poses, m->stream));
    HIPCHK(m, launch_map_score(T, din, n, poses, P.count[l], thr2, B.pcnt.p, B.psum.p, rec, m->stream));
    HIPCHK(m, launch_map_search_rank(rec, lat, P.count[l], P.kept[l], kept, m->stream));
  }
  const int last = P.levels - 1;
  HIPCHK(m, launch_map_search_gather(P.grid, B.lat.p + 6 * P.first[last], B.poses.p + 12 * P.first[last],
                                     B.rec.p + SVNICP_MAP_SCORE_FIELDS * P.first[last], B.kept.p + (size_t)last * kSearchMaxKeep, n_top,
                                     B.rec.p + SVNICP_MAP_SCORE_FIELDS * P.zero_index, B.stage.p, m->stream));
  B.host.resize(stage_bytes / 8);
  HIPCHK(m, hipMemcpyAsync(B.host.data(), B.stage.p, stage_bytes, hipMemcpyDeviceToHost, m->stream));
  HIPCHK(m, hipStreamSynchronize(m->stream));   // complete when the call returns: the caller's rows are free again
  B.plan = P;
  B.done = true;
  std::memset(out, 0, sizeof *out);
  out->levels = P.levels; out->active_axes = P.active_axes; out->nodes_scored = P.total;
  for (int l = 0; l < P.levels; ++l) { out->level_count[l] = P.count[l]; out->level_kept[l] = P.kept[l]; }
  std::memcpy(out->fine_step, P.grid.fine, sizeof out->fine_step);
  const double* h = B.host.data();
  std::memcpy(out->zero_record, h, 4 * 8);
  std::memcpy(out->best_correction, h + 4, 6 * 8);
  std::memcpy(out->best_pose, h + 10, 12 * 8);
  std::memcpy(out->best_record, h + 22, 4 * 8);
  std::memcpy(out->best_lattice, h + 4 + kSearchTopDoubles * n_top, 6 * 4);
  return SVNICP_OK;
}

int svnicp_map_search_top(svnicp_map* m, int cap, int32_t* latticeNx6, double* correctionsNx6, double* posesNx12, double* recordsNx4,
                          int* n_out) {
  if (!m) return SVNICP_ERR_INVALID;
  if (!m->se.done) return fail(m, SVNICP_ERR_INVALID, "svnicp_map_search_top: no successful svnicp_map_search_poses yet");
  if (cap < 0) return fail(m, SVNICP_ERR_INVALID, "svnicp_map_search_top: cap must be >= 0");
  const int n_top = m->se.plan.kept[m->se.plan.levels - 1];
  if (n_out) *n_out = n_top;
  const int k = cap < n_top ? cap : n_top;
  const double* h = m->se.host.data() + 4;
  const int32_t* hl = reinterpret_cast<const int32_t*>(h + kSearchTopDoubles * n_top);
  for (int i = 0; i < k; ++i, h += kSearchTopDoubles) {
    if (latticeNx6) std::memcpy(latticeNx6 + 6 * i, hl + 6 * i, 6 * 4);
    if (correctionsNx6) std::memcpy(correctionsNx6 + 6 * i, h, 6 * 8);
    if (posesNx12) std::memcpy(posesNx12 + 12 * i, h + 6, 12 * 8);
    if (recordsNx4) std::memcpy(recordsNx4 + 4 * i, h + 18, 4 * 8);
  }
  return SVNICP_OK;
}

int svnicp_map_search_level(svnicp_map* m, int level, int64_t cap, int32_t* latticeCx6, double* posesCx12, double* recordsCx4,
                            int32_t* kept_indices, int64_t* count_out, int* kept_out) {
  if (!m) return SVNICP_ERR_INVALID;
  if (!m->se.done) return fail(m, SVNICP_ERR_INVALID, "svnicp_map_search_level: no successful svnicp_map_search_poses yet");
  const MapSearchBufs& B = m->se;
  const MapSearchPlan& P = B.plan;
  if (level < 0 || level >= P.levels || cap < 0)
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_search_level: need 0 <= level < levels of the last search and cap >= 0");
  HIPCHK(m, hipSetDevice(m->device));
  if (count_out) *count_out = P.count[level];
  if (kept_out) *kept_out = P.kept[level];
  const size_t c = (size_t)(cap < P.count[level] ? cap : P.count[level]);
  const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
  if (c && latticeCx6) HIPCHK(m, hipMemcpyAsync(latticeCx6, B.lat.p + 6 * P.first[level], c * 24, d2h, m->stream));
  if (c && posesCx12) HIPCHK(m, hipMemcpyAsync(posesCx12, B.poses.p + 12 * P.first[level], c * 96, d2h, m->stream));
  if (c && recordsCx4) HIPCHK(m, hipMemcpyAsync(recordsCx4, B.rec.p + 4 * P.first[level], c * 32, d2h, m->stream));
  if (kept_indices)
    HIPCHK(m, hipMemcpyAsync(kept_indices, B.kept.p + (size_t)level * kSearchMaxKeep, (size_t)P.kept[level] * 4, d2h, m->stream));
  HIPCHK(m, hipStreamSynchronize(m->stream));
  return SVNICP_OK;
}

void* svnicp_map_points_devptr(svnicp_map* m) { return m ? (void*)m->sel.out.p : nullptr; }

int svnicp_map_download(svnicp_map* m, double* out_xyz, int64_t cap_points, int64_t* n_out) {
  if (!m || !n_out) return SVNICP_ERR_INVALID;
  return download_rows(m, m->sel.out.p, m->sel.last_M, out_xyz, cap_points, n_out);
}

}  // extern "C"
