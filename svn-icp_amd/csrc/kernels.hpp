// kernels.hpp — argument blocks and host launchers of the HIP kernels (internal to libsvnicp_hip.so)
#pragma once
#include "device_math.hpp"
#include "registration_plan.hpp"
#include "stage_a_plan.hpp"

namespace svnicp {

// ---------------- Stage A (knn_topk.hip) ----------------
struct KnnArgs {
  const double* src;  // [B][3] source cloud (un-transformed)
  Pose0 pose;         // R0, t0
  const double *tx, *ty, *tz;  // target SoA in permuted order, padded to Mp with NaN
  const int32_t* torig;        // [Mp] original target index of each slot
  int64_t M, Mp;
  int64_t b_lo, b_hi;  // query rows handled by this launch
  int K, S;            // S = pool capacity (power of two >= K + 128)
  double* pool_d;      // [B][S]
  int32_t* pool_i;     // [B][S]
  int32_t* out_idx;    // [B][K]
  double* out_d2;      // [B][K]
  const int32_t* qlist;     // list mode (fallback of k_knn_scan): query indices, else nullptr
  const int* qlist_count;   // device scalar: number of entries of qlist
  int list_grid;            // list mode: number of workgroups
  int list_qw;              // list mode: queries per wave chunk (pool rows = list_grid*4*list_qw)
  // sliced list mode (lists of at most slice_max_queries): every listed query is scanned by `slices` waves over
  // disjoint target ranges; per-slice top-K lists in sl_d/sl_i [slice_max_queries][slices][K], merged by
  // k_knn_merge_slices (merge_n = power of two >= slices*K).  slices = 0: plain list mode.
  int slices, slice_max_queries, merge_n;
  double* sl_d;
  int32_t* sl_i;
  const double* qthr;  // sliced list mode, optional: starting threshold of each listed query (from k_knn_tiles)
};
hipError_t launch_knn_merge_slices(const KnnArgs& a, hipStream_t st);

// ---------------- Stage A for small registrations (knn_brute.hip) ----------------
struct KnnBruteArgs {
  const double* src;   // [B][3] source cloud (un-transformed)
  Pose0 pose;          // R0, t0
  const double* tgt;   // [M][3] target cloud as given (no re-ordered copy)
  int64_t M;
  int64_t b_lo, b_hi;  // query rows of this launch
  int K;
  int32_t* out_idx;    // [B][K]
  double* out_d2;      // [B][K]
  unsigned long long* phase_cycles;   // optional [8]: thread-0 cycles per phase, summed over the workgroups (option debug)
};
int knn_brute_queries_per_block(int64_t n, int num_cus);
// queries_per_block: 0 = knn_brute_queries_per_block(n, num_cus); 1..6 = as given (option brute_qb, A/B)
hipError_t launch_knn_brute(const KnnBruteArgs& a, int num_cus, int queries_per_block, hipStream_t st);

// ---------------- Stage A fast variant (knn_scan.hip) ----------------
struct KnnScanArgs {
  const double* src;
  Pose0 pose;
  const double *tx, *ty, *tz;     // f64 permuted SoA (exact distances of the survivors)
  const float *txf, *tyf, *tzf;   // f32 copies (pre-filter)
  const int32_t* torig;
  const unsigned long long* emax_bits;  // max |target coordinate| as the bits of a non-negative double
  int64_t M, Mp, Ms;              // Ms = slots scanned in the seed phase
  int64_t b_lo, b_hi;
  int K, S2, seed_rank;
  int32_t* pool;                  // [B][S2] slots
  int32_t* out_idx;               // [B][K]
  double* out_d2;                 // [B][K]
  int32_t* fail_list;             // [B]
  int* fail_count;
};
hipError_t launch_targets_soa2(const double* tgt, int64_t M, int64_t Mp, double* tx, double* ty, double* tz,
                               float* txf, float* tyf, float* tzf, int32_t* torig, unsigned long long* emax_bits,
                               hipStream_t st);
hipError_t launch_knn_scan(const KnnScanArgs& a, hipStream_t st);
hipError_t launch_knn_topk(const KnnArgs& a, hipStream_t st);

// ---------------- Stage A pruned variant (spatial_prep.hip, knn_tiles.hip) ----------------
struct KnnTilesArgs {
  const double* src;
  Pose0 pose;
  const int32_t* qorder;          // [b_hi-b_lo] original query rows in Morton order
  const double *tx, *ty, *tz;     // Morton-ordered target SoA (f64), NaN padded to Mp
  const float *txf, *tyf, *tzf;   // f32 copies
  const int32_t* torig;
  const float* tile_box;          // [6][n_tiles]: lo xyz, hi xyz (outward rounded)
  const unsigned long long* emax_bits;
  // tile-local rows of the matrix-pipe pre-filter (spatial_prep.hip: k_targets_sorted)
  const float4* tile_a;           // [n_tiles][8][64]: (x', y', z', |t'|²) of the tile's 512 slots in MFMA A-operand order
  const float4* tile_o;           // [n_tiles]: the tile's origin (float32) | C_t = max |t'|₂, rounded up (+inf: no bound)
  int prefilter_mfma;             // 1: the scan kernel scores on the bf16 matrix pipe, 0: the float32 VALU loop
  int seed_rank_full;             // 0: the seed kernel's rank phase scores only the tiles that can still be picked (seed_rank = bounded), 1: all of a visited group (full)
  int64_t M, Mp;
  int n_tiles;
  int64_t b_lo, b_hi;
  int K, S2;                      // S2 = most survivors a query may hold: kTilesBase + kTilesChunks * kTilesChunk
  int32_t* pool;                  // [B][kTilesBase]: the first survivors of each query position
  int32_t* arena;                 // [arena_cap][kTilesChunk]: overflow chunks, handed out on demand to the few heavy queries
  int32_t* chunk_tab;             // [B][kTilesChunks] chunk id per (query position, chunk), -1 = none; [B*kTilesChunks] = allocation counter (starts at -1)
  int arena_cap;
  int64_t tab_rows;               // B of the allocation (rows of chunk_tab); after the table: the chunk allocation counter
  int scan_split;                 // waves per 64-query workgroup of the scan kernel: 4 or 8
  unsigned int group_stride;      // scan kernel: workgroup i serves group (i * group_stride) mod n_groups (coprime to n_groups)
  int32_t* out_idx;
  double* out_d2;                 // nullptr: the distances are not stored (svnicp_get_candidate_dist2 recomputes them: launch_candidate_dist2)
  // the select kernel writes the split variant's search table rows itself (registration_plan.hpp: select_writes_table), as
  // k_build_table3 (stein_split.hip) would from out_idx; tbl_a == nullptr: it does not
  const double* tgt;              // [M][3] as given
  float4* tbl_a;                  // [B][2][64]
  double* tbl_anchor;             // [B][3]
  float* tbl_cmax;                // [B]
  int32_t* fail_list;
  int* fail_count;
  int32_t* stat_n;                // optional [B]: survivors of the f32 filter per query (first pass)
  unsigned long long* phase_cycles;  // optional [8]: summed wave cycles per phase (debug, SVNICP_DEBUG)
  void* qrec;         // [B] 48-byte per-query records (position, threshold, survivor count) between the two kernels
  double* fail_tau;   // optional [B]: a valid threshold (>= K-th distance) of each failed query, +inf if none
};
hipError_t launch_knn_tiles(const KnnTilesArgs& a, hipStream_t st);
// d2[b][k] of idx [B][K] again, for a stage A that did not store it: the query as the seed kernel forms it, the unfused
// ((dx·dx)+dy·dy)+dz·dz, and 0.0 for the entries a row was padded with (knn_cpu.cpp:25-26)
hipError_t launch_candidate_dist2(const double* src, const Pose0& pose, const double* tgt, int64_t M, const int32_t* idx, int64_t B, int K,
                                  double* d2, hipStream_t st);
size_t sort_temp_bytes(size_t n, int key_bits);   // 30: one cloud's Morton keys, 31: the joint sort of target and queries
hipError_t launch_bbox(const double* pts, int64_t n, unsigned long long* bbox, bool cleared, hipStream_t st);
// rocprim_sort: rocprim::radix_sort_pairs (option sort_kernel = merge) instead of the file's own radix chain; fill_ff[0, fill_words): set
// to -1 by the (query) key kernel on the way
hipError_t launch_morton_order(const double* pts, int64_t i0, int64_t n, int transform, const Pose0& pose,
                               const unsigned long long* bbox, unsigned int* keys_a, unsigned int* keys_b,
                               int32_t* vals_a, int32_t* order, void* temp, size_t temp_bytes, bool rocprim_sort, int32_t* fill_ff,
                               size_t fill_words, hipStream_t st);
hipError_t launch_morton_order_joint(const double* tgt, int64_t M, const double* qsrc, int64_t n, const Pose0& pose,
                                     const unsigned long long* bbox, unsigned int* keys_a, unsigned int* keys_b,
                                     int32_t* vals_a, int32_t* order, void* temp, size_t temp_bytes, bool rocprim_sort, int32_t* fill_ff,
                                     size_t fill_words, hipStream_t st);
hipError_t launch_targets_sorted(const double* tgt, int64_t M, int64_t Mp, const int32_t* order, double* tx, double* ty,
                                 double* tz, float* txf, float* tyf, float* tzf, int32_t* torig, float* tile_box,
                                 unsigned long long* emax_bits, bool emax_cleared, float4* tile_a, float4* tile_o, hipStream_t st);

// ---------------- Stage B (stein_iter.hip) ----------------
struct AccumArgs {
  const double* src;    // [B][3]
  const double* table;  // [B][K][3] candidate coordinates (f64, absolute)
  const float4* tablef; // [B][K] float32 local coordinates + |c'|² (fast variant)
  const float4* tablea; // [B][2][64] float32 local rows in MFMA A-operand order (stein_split.hip: k_build_table3)
  const float* cmax;    // [B] max |c'| per source point (fast variants)
  int* ambig_count;     // optional statistic: wave steps that took the exact path, or nullptr
  const double* Rtot;   // [P][12]: R_total row-major (9) + t_total (3)
  int64_t B;
  int K, RS;            // RS = LDS row stride in doubles (odd)
  int p_lo, p_hi;       // particle shard of this GPU
  int TP;               // source points per LDS tile
  int tiles_per_block;
  int64_t n_tiles;
  int Ppad;             // padded shard size = gridDim.y * particles per workgroup
  double max_dist;
  double* partial;      // [gridDim.x][Ppad][kNSums]
  const int* ctl;       // ctl[0] = stop flag
  int32_t* corr;        // optional trace [P][B] (this iteration), or nullptr
  int svgd;             // SVGD-ICP mode: slot 4 of the sums counts non-zero rows (SVGDICP.cpp:404)
  // split variant: no f64 candidate table — winners are gathered as tgt[cand[b][k]] (6 MB + 4 B/candidate instead of
  // 24 B/candidate of HBM traffic), the local frame's origin comes from anchor[b]
  const double* tgt;    // [M][3]
  const int32_t* cand;  // [B][K] candidate indices (stage A)
  const double* anchor; // [B][3] = tgt[cand[b][0]]
  int64_t M;
  uint8_t* kbest;       // split variant: winner slot per (source point, particle of the shard), [B][Ppad]
  int32_t* kidx;        // … and the winner's TARGET index cand[b][slot], [B][Ppad]: the accumulate kernel's gather then starts one
                        // dependent load later (byte -> index -> coordinates becomes index -> coordinates)
  const int32_t* full_idx;  // correspondence = full: nearest target index of every (particle, source point), [P][B]; else nullptr
  int pts_per_block, spts_per_block;  // split variant: source points per workgroup (accumulate / search kernel)
  unsigned int* ticket;               // fused one-particle iteration: arrival counter of the accumulate kernel's workgroups
  // the PREVIOUS iteration's early-stop decision, taken by workgroup (0, 0) of the search kernel instead of a k_upd_finish
  // launch of its own (svnicp_align's loop; fin_iteration < 0: nothing to decide)
  int fin_iteration, fin_P;
  double fin_thr;
  const double* fin_norms;            // [P] step norms of that iteration (uctl + UCTL_NORM)
  const double* fin_pose;             // [6][P] pose_out
  float* fin_history;                 // [I][6][P]
  int* fin_ctl;                       // [0] stop flag, [1] finish_iter
};
// completes the registration's stage-B plan (registration_plan.hpp: plan_stage_b — variant, shape, `small`) with what depends
// on the device: the grids of B rows per iteration from the kernels' occupancy, the LDS tiles of the fused variants
AccumPlan plan_accumulate(AccumPlan shape, int64_t B, int num_cus, const Tuning& tune);
hipError_t launch_search_split(const AccumPlan& plan, AccumArgs a, hipStream_t st);         // split variant, kernel 1
hipError_t launch_accumulate_split(const AccumPlan& plan, const AccumArgs& a, hipStream_t st);  // split variant, kernel 2 (via launch_accumulate)
void split_occupancy_blocks(int PW, int WP, int K, size_t smem, int* search, int* accum);
// table may be nullptr (split variant): then only anchor / tablea / cmax are written
hipError_t launch_build_table3(const int32_t* idx, int64_t B, int K, const double* tgt, int64_t M, double* table,
                               double* anchor, float4* tablea, float* cmax, hipStream_t st);
// the rows list[0 … *count) only, both read on the device (stage A's fallback rows behind a select kernel that writes the table)
hipError_t launch_build_table3_list(const int32_t* idx, const int32_t* list, const int* count, int64_t B, int K, const double* tgt,
                                    int64_t M, double* anchor, float4* tablea, float* cmax, hipStream_t st);
hipError_t launch_build_table2(const int32_t* idx, int64_t B, int K, const double* tgt, int64_t M, double* table,
                               float4* tablef, float* cmax, hipStream_t st);
// q[b] = (s·R^T) + t with the stage-B expression (SVNICP.cpp:62-64); pose12 = device [R row-major | t]
hipError_t launch_transform_cloud(const double* src, int64_t B, const double* pose12, double* q, const int* ctl, hipStream_t st);
// ---------------- particle update (particle_update.hip, small_registration.hip, particle_state.hip, reduce_partials.hip) ----------------
struct UpdateArgs {
  const double* sums;  // [P][kNSums] (all particles); source-row sharding: [n_ranks][P][kNSums], summed in rank order on load
  int n_ranks;         // 1, or the number of row-shard records behind `sums`
  int sums_stride;     // doubles between two records of `sums` (0: P * kNSums); small chain: the accumulate kernel's partial rows
  double* sums_out;    // small chain: k_upd_prepare stores each particle's reduced record here, or nullptr
  double* R;           // [P][9]
  double* t;           // [P][3]
  double* Rtot;        // [P][12]
  Pose0 pose;
  int P, iteration, iterations;
  double lr, conv_thr;
  int check_early_stop, full_grad;
  double* work;        // workspace, see update_workspace_doubles()
  float* history;      // [I][6][P]
  double* pose_out;    // [6][P]
  int* ctl;            // [0] stop flag, [1] finish_iter
  double *trH, *trb, *trN, *trphi, *trh;  // optional traces (per-iteration slices) or nullptr
  int h_in_lds;        // set by launch_update: per-particle H fits in LDS
  // SVGD-ICP mode (k_particle_update_svgd)
  double* eul;         // [P][6] optimizer parameters x,y,z,roll,pitch,yaw
  double* opt;         // [3][P][6] optimizer state
  int svgd;            // 1: SVGD-ICP mode through the workgroup-parallel chain (k_upd_prepare … k_upd_finish)
  int optimizer;       // SVNICP_OPT_*
  double n_src;        // gradient_scaling_factor_ = B (SVGDICP.cpp:58)
  double* uctl;        // multi-workgroup update path: small control / norm area
  unsigned long long* dbg;  // optional [8]: cycle stamps of the fused kernel's phases (SVNICP_DEBUG)
  const double* plane_Hb;   // point-to-plane mode: [P][42] = H | b as k_plane_finalize left them — the kernels then skip load_sums +
                            // finalize_Hb (wave-uniform; nullptr in point mode).  With a pose prior (pose_prior.hip), in either mode:
                            // the record k_pose_prior wrote, the base record with the prior's terms added
};
size_t update_workspace_doubles(int P);
// areas k_init_particles clears at the start of a registration (whole 32-bit words), and the control words it resets
// (ones: an area set to all ones instead — stage A's bounding-box minima)
struct BeginZero { unsigned int* ptr[10]; unsigned int dwords[10]; int n; int* ctl; int iterations; unsigned int* ones; unsigned int ones_dwords; };
hipError_t launch_init_particles(const double* init6xP, int P, const Pose0& pose, int mode, double* R, double* t,
                                 double* Rtot, double* pose_out, int refresh_pose, double* eul, hipStream_t st, const BeginZero* zero = nullptr);
// stage B accumulate (fused variants: whole stage B); single: see stein_iter.hip — the one-particle iteration in one launch
int single_particle_grid(int64_t B);   // workgroups of the one-particle iteration kernel (rows of `partial` it writes)
hipError_t launch_accumulate(const AccumPlan& plan, AccumArgs a, const UpdateArgs* single, hipStream_t st);
hipError_t launch_update_svgd(const UpdateArgs& a, hipStream_t st);
hipError_t launch_update(const UpdateArgs& a, hipStream_t st);
// the Stein step of P >= 2 particles in three pieces (particle_update.hip): pair statistics (second stream), sums -> H, b,
// Newton steps, direction + pose update
hipError_t launch_update_median(const UpdateArgs& a, int num_cus, int max_p_one_workgroup, hipStream_t st);
hipError_t launch_update_prepare(const UpdateArgs& a, hipStream_t st);
hipError_t launch_update_prepare_median(const UpdateArgs& a, hipStream_t st);   // small chain: both in one launch (2 <= P <= 128)
// small chain, all iterations in one cooperative launch (small_registration.hip: k_small_registration)
hipError_t launch_small_registration(const AccumPlan& plan, AccumArgs a, const UpdateArgs& u, int iterations, unsigned int* bar,
                                     int num_cus, hipStream_t st);
hipError_t launch_update_direction(const UpdateArgs& a, hipStream_t st, bool finish = true);   // finish: k_upd_finish behind it when the step needs one
const double* update_step_norms(const UpdateArgs& a);   // [P] norms the early-stop decision averages
hipError_t launch_reduce_partials(const double* partial, int nblk, int Ppad, int p_lo, int n_particles, double* sums, const int* ctl,
                                  hipStream_t st);
size_t update_uctl_doubles(int P);
// ---------------- Gaussian pose prior on the correction (pose_prior.hip; PosePrior: pose_prior.hpp) ----------------
struct PosePrior;
// record [P][42] = particle_Hb(a) + the prior's JᵀΛJ | JᵀΛe at the poses a.R, a.t; `a` as the Stein step WITHOUT a prior would
// get it (its plane_Hb is the plane record or nullptr, never `record`)
hipError_t launch_pose_prior(const UpdateArgs& a, const PosePrior& pr, double* record, hipStream_t st);
// ---------------- point-to-plane residual (plane_icp.hip) ----------------
constexpr int kPlaneSums = 29;             // per (workgroup, particle): H upper triangle (21) | b (6) | accepted pairs | Σ w·r²
struct PlaneArgs {
  const double* src;    // [B][3]
  const double* rec;    // [M][6] target xyz | unit normal (0 = no normal here)
  const double* Rtot;   // [P][12]
  int64_t B, M;
  int p_lo, p_hi;
  int Ppad;             // set by the launcher from the plan, like pts_per_block
  int pts_per_block;
  double max_dist, delta;
  double* partial;      // [plan.grid_x][Ppad][kPlaneSums]
  const int* ctl;       // ctl[0] = stop flag
  const int32_t* kidx;  // [B][Ppad] the search kernel's winner (target index)
  const uint8_t* kbest; // [B][Ppad] … and its slot among the K candidates (read for the trace only)
  int32_t* corr;        // optional trace [P][B] (this iteration), or nullptr
};
// normals of target rows [row_lo, row_lo + rows) from their kn nearest target points nbr [rows][kn] into rec [M][6]
hipError_t launch_target_normals(const double* tgt, int64_t M, const int32_t* nbr, int64_t row_lo, int64_t rows, int kn, double* rec,
                                 hipStream_t st);
hipError_t launch_pack_normals(const double* tgt, const double* nrm, int64_t M, double* rec, hipStream_t st);
hipError_t launch_plane_accumulate(const AccumPlan& plan, PlaneArgs a, hipStream_t st);
hipError_t launch_plane_finalize(const double* partial, int nblk, int Ppad, int p_lo, int n_particles, double* Hb, double* stats,
                                 const int* ctl, hipStream_t st);
// ---------------- generalized-ICP residual (gicp_icp.hip) ----------------
// the accumulate kernel only: its records have plane mode's layout (kPlaneSums) and go through launch_plane_finalize; the
// source's record [B][6] is made by launch_target_normals / launch_pack_normals with the source as the cloud
struct GicpArgs {
  const double* srec;   // [B][6] source xyz | unit normal (0 = no normal here)
  const double* rec;    // [M][6] target xyz | unit normal (0 = no normal here)
  const double* Rtot;   // [P][12]
  int64_t B, M;
  int p_lo, p_hi;
  int Ppad;             // set by the launcher from the plan, like pts_per_block
  int pts_per_block;
  double max_dist, delta, eps;
  double* partial;      // [plan.grid_x][Ppad][kPlaneSums]
  const int* ctl;       // ctl[0] = stop flag
  const int32_t* kidx;  // [B][Ppad] the search kernel's winner (target index)
  const uint8_t* kbest; // [B][Ppad] … and its slot among the K candidates (read for the trace only)
  int32_t* corr;        // optional trace [P][B] (this iteration), or nullptr
};
hipError_t launch_gicp_accumulate(const AccumPlan& plan, GicpArgs a, hipStream_t st);
// ---------------- evaluate a registration (evaluate.hip) ----------------
constexpr int kEvalRecord = 5;   // per workgroup: evaluated, inliers, plane inliers (counts, exact in float64), sum d2, sum r2
constexpr int kEvalResult = 8;   // the record's five totals | fitness, inlier rmse, plane rmse
struct EvalPose { double R[9]; double t[3]; };   // the pose under evaluation, row-major, by value
struct EvalArgs {
  const double* q;      // [B][3] transformed source
  const double* tgt;    // [M][3]
  const double* rec;    // [M][6] target xyz | unit normal when the context holds normals of this target, else nullptr
  int64_t B, M;
  double thr2;          // max_corr_dist^2
  int32_t* idx;         // [B] in: stage A's nearest target (K = 1); out: the same, -1 = not evaluated
  double* d2;           // [B] out: d2 recomputed from q and that row, NaN = not evaluated
  double* partial;      // [evaluate_blocks(B)][kEvalRecord]
};
int64_t evaluate_blocks(int64_t B);
hipError_t launch_evaluate_transform(const double* src, int64_t B, const EvalPose& T, double* q, hipStream_t st);
// k_evaluate_pairs + k_evaluate_finalize: result[kEvalResult] in device memory
hipError_t launch_evaluate_pairs(const EvalArgs& a, double* result, hipStream_t st);
// ---------------- information matrix of a registration (information.hip) ----------------
constexpr int kInfoPointRecord = 18;   // per workgroup: pairs, sum w, sum w d2 | sum w s (3) | sum w s s^T (6) | sum w c (3) | sum w s x c (3)
constexpr int kInfoPlaneRecord = 30;   // per workgroup: pairs, sum w, sum w r^2 | sum w j j^T upper triangle (21) | sum w r j (6)
constexpr int kInfoResult = 45;        // H[36] row-major | b[6] | pairs, sum w, sum w r^2
struct InfoArgs {
  const double* src;    // [B][3] source cloud as given
  const double* q;      // [B][3] the last evaluate's transformed source
  const double* tgt;    // [M][3]
  const double* rec;    // [M][6] target xyz | unit normal when that evaluate had normals, else nullptr (the plane form needs it)
  const int32_t* idx;   // [B] that evaluate's nearest target row, -1 = not evaluated
  const double* d2;     // [B] its d2, NaN = not evaluated
  int64_t B, M;
  double thr2;          // that evaluate's max_corr_dist^2
  double delta;         // Huber delta, +inf = unweighted
  EvalPose T;           // that evaluate's pose
  double* partial;      // [evaluate_blocks(B)][record of the form]
  const double* srec;   // the GICP form only: [B][6] source xyz | unit normal, 0 = no normal here (nullptr for the other forms)
  double eps;           // the GICP form only: epsilon of the surface covariances
};
// form 0 = point, 1 = plane (SVNICP_INFO_*), 2 = the GICP form of svnicp_eval_information_gicp (gicp_pair_device.hpp; the record
// has the plane form's layout).  k_information_pairs + k_information_finalize: result[kInfoResult] in device memory
hipError_t launch_information(int form, const InfoArgs& a, double* result, hipStream_t st);
// ---------------- score and weight the particles (particle_score.hip) ----------------
constexpr int kScoreRecord = 5;        // per (workgroup, particle): evaluated, inliers, plane inliers (exact counts), sum d2, sum r2 (forms 1, 2: accepted, sum h)
constexpr int kScoreFields = 6;        // per particle: the record's five totals | cost  (SVNICP_SCORE_FIELDS)
constexpr int kScoreRowsPerBlock = 64; // source rows a workgroup owns: a multiple of every row step of the geometry
struct ScoreArgs {
  const double* src;    // [B][3]
  const double* tgt;    // [M][3]
  const double* rec;    // [M][6] target xyz | unit normal when the context holds normals of this target, else nullptr
  const int32_t* cand;  // [B][K] the registration's candidate target indices (stage A)
  const double* Rtot;   // [P][12] the poses that are scored
  int64_t B, M;
  int K, P;
  int Ppad, TH;         // set by the launcher: padded particle count, source rows per LDS tile
  double thr2;          // max_corr_dist^2
  double* partial;      // [score_blocks(B)][Ppad][kScoreRecord]
  // svnicp_score_particles_objective; all zero: the point cost above
  int form;             // SVNICP_SCORE_POINT | _PLANE | _GICP (resolved, never AS_SOLVED); forms 1 and 2 need rec, form 2 srec
  const double* srec;   // [B][6] source xyz | unit normal (GicpState::rec), form 2
  double delta, eps;    // the robust term's delta (+inf: none), the GICP epsilon
  double cap;           // h(max_corr_dist): what a row that is not accepted costs in forms 1 and 2
};
int64_t score_blocks(int64_t B);
int score_padded_particles(int P, int K);
// source rows per LDS tile for this K (0: one row's candidates do not fit, the launch is refused)
int score_tile_rows(int P, int K, bool normals);
// k_particle_score + k_particle_score_finalize: scores [P][kScoreFields] in device memory
hipError_t launch_particle_score(ScoreArgs a, double* scores, hipStream_t st);
// w[p] = exp(-(cost_p - cost_min) / temperature) / Z, Z added in particle order (one workgroup)
hipError_t launch_particle_weights(const double* scores, int P, double temperature, double* w, hipStream_t st);

// ---------------- particle modes (particle_modes.hip) ----------------
constexpr int kModesMax = 32;          // SVNICP_MODES_MAX
constexpr int kModesMaxP = 2048;       // particles one workgroup stages: 72 bytes of LDS each (147 KB); more is refused
constexpr int kModesHeader = 8;        // particles, nonfinite, n_modes, n_reported, sweeps, W_all, 0, 0
constexpr int kModesRecord = 48;       // per reported mode: label, count, best, mass, cost_min, cost_mean, mean[6], cov[36]
constexpr int kModesResult = kModesHeader + kModesMax * kModesRecord;   // doubles; the int32 labels [P] follow them
struct ModesArgs {
  const double* pose;    // [6][P] component-major (pose_out)
  const double* w;       // [P], or nullptr: every weight is 1.0
  const double* scores;  // [P][kScoreFields] of a scoring of exactly these particles, or nullptr
  int P, max_modes;
  double lt2, lr2;       // link_trans^2, link_rot^2
  double* result;        // [kModesResult] doubles (the integers exact), then int32 [P]: rank of each particle's mode, -1 = non-finite
};
inline size_t modes_result_bytes(int P) { return (size_t)kModesResult * sizeof(double) + (size_t)P * sizeof(int32_t); }
// k_particle_modes: one workgroup; hipErrorInvalidValue for P outside [1, kModesMaxP] or max_modes outside [1, kModesMax]
hipError_t launch_particle_modes(const ModesArgs& a, hipStream_t st);

// ---------------- mini-batch tables (minibatch.hip) ----------------
struct MinibatchArgs {
  const int32_t* explicit_idx;  // [n] a caller's table (validated by the draw kernel), or nullptr: generated from `base`
  int32_t* idx;                 // [n] the table this registration uses (n = iterations * batch, epoch-major)
  int64_t n, B;                 // table positions, source rows
  unsigned long long base;      // splitmix64(seed * 1000003 + registration): idx[j] = umul64hi(splitmix64(base + j), B)
  int32_t* flag;                // [B] 1 = row drawn
  int32_t* pos;                 // [B] position of a drawn row among the unique rows (ascending), -1 = not drawn
  int32_t* block_sums;          // [minibatch_scan_blocks(B)]
  int* mbctl;                   // [0] an explicit table held a value outside [0, B), [1] unique rows U
  int* ctl;                     // the registration's control words: [0] stop flag, raised with mbctl[0]
  const double* src;            // [B][3]
  double* src_u;                // [n_q][3] unique rows, then copies of the last one
  int64_t n_q;                  // queries stage A runs: min(B, n)
};
unsigned long long minibatch_stream_base(unsigned long long seed, unsigned long long registration);
int64_t minibatch_scan_blocks(int64_t B);
// memsets + draw/mark + scan + compaction + fill of src_u; no host synchronisation
hipError_t launch_minibatch_draw_compact(const MinibatchArgs& a, hipStream_t st);
// src_mb [n][3] = src[idx[j]], cand_mb [n][K] = cand_u[pos[idx[j]]] (one wave per position)
hipError_t launch_minibatch_expand(const MinibatchArgs& a, const int32_t* cand_u, int K, double* src_mb, int32_t* cand_mb,
                                   hipStream_t st);

struct StatsArgs { const double* pose; int P; int mode; double* out; /* mean6,var6,cov36,weightsP */ };
hipError_t launch_stats(const StatsArgs& a, hipStream_t st);
// the same block with the weights w[P] of launch_particle_weights (SVN mode; SVNICP.cpp:286-308 as written, for any weights)
hipError_t launch_stats_weighted(const StatsArgs& a, const double* w, hipStream_t st);

}  // namespace svnicp
