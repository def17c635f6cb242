// registration_plan.hpp — the rules of a registration behind stage A: how many rows each part works on, what is refused,
// which stage-B variant and shape the particle shard gets, which launches carry the Stein step and how svnicp_align drives
// them (host only; no HIP needed, so the CPU tests compile it on its own).  Pure functions of the options (Tuning) and of
// the facts svnicp_align_begin reads off the context (RegistrationFacts); plan_accumulate (stein_iter.hip) only completes
// the shape with the device-dependent grid sizes.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "stage_a_plan.hpp"

namespace svnicp {

// test / profiling knobs of a context (svnicp_set_option); the defaults are the product configuration
struct Tuning {
  KnnOption knn;                 // stage A kernel: automatic, or v1 | v2 | tiles | brute (stage_a_plan.hpp: plan_stage_a)
  int knn_prefilter_mfma = 1;    // stage A tile scan: 1 = pre-filter on the bf16 matrix pipe (knn_prefilter = mfma), 0 = float32 VALU loop (valu)
  int seed_rank_full = 0;        // stage A tile seed: 0 = the rank phase skips tiles behind the wave-wide bound (seed_rank = bounded), 1 = scores every tile of a visited group (full, A/B)
  int fallback_sliced_max = -1; // stage A: failed queries redone by target slices up to this many (-1 default)
  int accum = 3;                 // stage B: 0 f64 baseline, 1 f32 VALU search (fused), 3 search + accumulate kernels
  int update_fused = 0;          // Stein update: 1 = one fused kernel for 2 <= P <= fused_update_max_p
  int fused_update_max_p = 128;  // above this the Stein step runs as workgroup-parallel kernels
  int wgpcu_search = 0, wgpcu_accum = 0;   // workgroups per CU the stage-B grids are sized for (0 = automatic)
  int tp = 0;                    // fused stage-B variants: source points per LDS tile (0 = automatic)
  int accum_min_steps = 0;       // least wave steps per accumulate workgroup (0 = default 4)
  int group_stride = 0;          // stage A scan: group order stride (0 = default, 1 = natural order)
  int scan_split = 0;            // stage A scan: waves per 64-query workgroup, 4 or 8 (0 = default)
  int debug = 0;                 // print plans and per-phase cycle counters to stderr
  int single_fused = 1;          // one particle: reduce + Stein step in the accumulate kernel's last workgroup (0: three launches, A/B)
  int small_chain = 1;           // small registrations: no k_reduce_partials, Stein-step front in one launch on the main stream (0: the general chain, A/B)
  int persistent = 0;            // 1: svnicp_align runs all iterations of a small-chain registration in ONE cooperative launch (k_small_registration;
                                 // measured SLOWER than the four launches per iteration on this eight-XCD part: off by default, option chain=persistent)
  int median_inline = -1;        // pair statistics in the prepare kernel's launch on the main stream also in the general chain: -1 automatic (P <= 128), 0 never (second stream), 1 the same as automatic
  int brute_qb = 0;              // brute-force stage A: queries per workgroup, 0 automatic (knn_brute_queries_per_block)
  int sort_joint = 1;            // 1: ONE Morton sort for target and queries where joint_morton_sort allows (sort = joint), 0: two (separate, A/B)
  int sort_merge = 0;            // Morton sorts: 0 = the project's three-pass radix chain (spatial_prep.hip), 1 = rocPRIM's radix_sort_pairs, its merge
                                 // path at these sizes (sort_kernel = radix | merge: A/B and the tests' second opinion)
  int table_select = 1;          // 1: stage A's select kernel writes the search table where select_writes_table allows (table = select), 0: k_build_table3 always (gather, A/B)
  int full_corr = 0;             // 1: correspondence = full — per-particle exact NN over the whole target (SVGDICP.cpp:274-298)
};

// what the rules read of the context besides its options, at svnicp_align_begin
struct RegistrationFacts {
  int P = 0, K = 0, I = 0;             // particles, knn_count, params.iterations
  int64_t B = 0, M = 0;                // source and target rows
  bool svgd = false, check_early_stop = false, record_trace = false;
  bool profiling = false;              // svnicp_set_profile
  bool shard_set = false;              // svnicp_set_shard: this context's particles are [p_lo, p_hi), else [0, P)
  int p_lo = 0, p_hi = 0;
  int row_world = 1;                   // svnicp_set_row_shard
  int batch = 0;                       // svnicp_set_minibatch, 0 = off
  bool explicit_tab = false;           // … with a caller's table of tab_I iterations
  int tab_I = 0;
  bool plane = false;                  // svnicp_set_residual: point-to-plane
  bool normals_supplied = false;
  int normal_k = 16;
  bool gicp = false;                   // svnicp_set_residual_gicp: generalized ICP (then `plane` is set too: it runs the plane residual's launch shape)
  bool source_normals_supplied = false;
  int weighting = 0;                   // svnicp_set_particle_weighting: SVNICP_WEIGHT_* (0 = uniform, the reference)
  int weighting_form = 0;              // … in which cost: the resolved SVNICP_SCORE_* form (0 = the point cost; _objective setter: 1 plane, 2 GICP)
  bool target_normals = false;         // the context holds normals of the current target, or this registration estimates them
  bool source_normals = false;         // … of the current source
  bool prior = false;                  // svnicp_set_pose_prior: a Gaussian prior on the correction is added in front of the Stein step
  int nshard() const { return p_hi - p_lo; }
  bool whole_shard() const { return p_lo == 0 && p_hi == P; }
};

// ---------------- row counts ----------------
constexpr int64_t kMinibatchMaxRows = 1ll << 22;   // iterations * batch: about 2.5 KB of per-row tables each (10 GB)
struct RegistrationRows {
  bool mb;       // this registration runs on a mini-batch table
  int64_t Bq;    // rows stage A runs on (mini-batch: no more than the table can draw)
  int64_t Bt;    // rows of the candidate tables (mini-batch: one per table position, epoch-major)
  int64_t Bi;    // rows one iteration works on
};
inline RegistrationRows registration_rows(int batch, int I, int64_t B) {
  if (batch == 0 || I <= 0) return {false, B, B, B};
  const int64_t n = (int64_t)I * batch;
  return {true, B < n ? B : n, n, batch};
}

// ---------------- refusals ----------------
// Each ladder is a list of (condition, reason): the first condition that holds is the one reported.
struct Refusal { bool holds; const char* why; };
inline const char* first_refusal(std::initializer_list<Refusal> ladder) {
  for (const Refusal& r : ladder)
    if (r.holds) return r.why;
  return nullptr;
}
constexpr const char* kMinibatchRefusal = "svnicp_align: mini-batch mode (svnicp_set_minibatch) is not available here: ";
constexpr const char* kPlaneRefusal = "svnicp_align: the point-to-plane residual (svnicp_set_residual) is not available here: ";
constexpr const char* kGicpRefusal = "svnicp_align: the generalized-ICP residual (svnicp_set_residual_gicp) is not available here: ";
constexpr const char* kWeightingRefusal = "svnicp_align: particle weighting (svnicp_set_particle_weighting) is not available here: ";
constexpr const char* kPriorRefusal = "svnicp_align: the pose prior (svnicp_set_pose_prior) is not available here: ";
constexpr const char* kScoringRefusal = "svnicp_score_particles: the last registration cannot be scored: ";

// A cloud's row count: row indices are int32 everywhere behind stage A (cand, kidx, torig, full_idx, the Morton sorts'
// values); a row's byte offset 24 * index is formed in 64 bits.
constexpr int64_t kMaxCloudRows = 0x7fffffffLL;   // 2^31 - 1: 24 * (kMaxCloudRows - 1) < 2^36
inline const char* cloud_rows_refusal(int64_t rows) { return rows > kMaxCloudRows ? "cloud too large" : nullptr; }

// mini-batch: what it is not combined with (nullptr: nothing, or mini-batch is off)
inline const char* minibatch_refusal(const RegistrationFacts& f, const Tuning& t) {
  if (f.batch == 0) return nullptr;
  return first_refusal({
      {f.batch < 0, "batch_size must be positive"},
      {f.shard_set && !f.whole_shard(), "a partial particle shard (svnicp_set_shard) is set"},
      {f.row_world > 1, "a source-row shard (svnicp_set_row_shard) is set"},
      {t.full_corr != 0, "option correspondence=full is set"},
      {t.persistent != 0, "option chain=persistent is set"},
      {(int64_t)f.I * f.batch > kMinibatchMaxRows, "iterations * batch_size exceeds 2^22 table rows (about 2.5 KB of tables per row)"},
      {f.explicit_tab && f.tab_I != f.I, "the explicit index table's iteration count differs from params.iterations"},
  });
}
// point-to-plane residual: what it is not combined with (all left for later).  What passes has accum = split, K <= 128 and
// the whole shard: stage_b_variant then gives the split kernels for any particle count.
inline const char* plane_refusal(const RegistrationFacts& f, const Tuning& t) {
  if (!f.plane) return nullptr;
  return first_refusal({
      {f.svgd, "SVGD mode has no Hessian to put the plane residual in"},
      {f.shard_set && !f.whole_shard(), "a partial particle shard (svnicp_set_shard) is set"},
      {f.row_world > 1, "a source-row shard (svnicp_set_row_shard) is set: the rank exchange carries the 22 point-to-point sums"},
      {f.batch != 0, "mini-batch mode (svnicp_set_minibatch) is set"},
      {t.full_corr != 0, "option correspondence=full is set"},
      {t.persistent != 0, "option chain=persistent is set"},
      {t.accum != 3, "option accum is not split: the plane kernel consumes the search kernel's winner index"},
      {f.K > 128, "knn_count exceeds 128: the plane kernel consumes the matrix-pipe search kernel's winner index"},
      {!f.normals_supplied && f.M < f.normal_k, "the target has fewer points than normal_k and no normals were supplied"},
  });
}
// generalized-ICP residual: everything the plane residual is not combined with (its accumulate kernel has the plane
// kernel's place and inputs), and a source too small for its own normal pass
inline const char* gicp_refusal(const RegistrationFacts& f, const Tuning& t) {
  if (!f.gicp) return nullptr;
  RegistrationFacts as_plane = f;
  as_plane.plane = true;
  if (const char* why = plane_refusal(as_plane, t)) return why;
  return first_refusal({
      {!f.source_normals_supplied && f.B < f.normal_k, "the source has fewer points than normal_k and no source normals were supplied"},
  });
}
// scoring the particles through the registration's candidate table (svnicp_score_particles): what the registration must
// not have run with.  The table is [B][K] of the whole scan for all particles; allowed in SVGD mode, in plane mode, for
// every stage-B variant and chain and any K the registration accepted.
inline const char* scoring_refusal(const RegistrationFacts& f, const Tuning& t) {
  return first_refusal({
      {f.shard_set && !f.whole_shard(), "a partial particle shard (svnicp_set_shard) is set"},
      {f.row_world > 1, "a source-row shard (svnicp_set_row_shard) is set: this context holds a part of the scan"},
      {f.batch != 0, "mini-batch mode (svnicp_set_minibatch) is set: its candidate tables are per drawn position"},
      {t.full_corr != 0, "option correspondence=full is set: the iterations did not search the candidate table"},
  });
}
// the objective a scoring runs in (svnicp_score_objective, include/svnicp_hip.h).  form: SVNICP_SCORE_*
struct ScoreObjective {
  int form = 0;                          // -1 = as solved, 0 = point, 1 = plane, 2 = GICP
  double gate = 0.0, delta = 0.0, eps = 0.0;
};
constexpr int kScoreAsSolved = -1, kScorePoint = 0, kScorePlane = 1, kScoreGicp = 2;
// what the struct's values themselves must satisfy, whoever takes them (the scoring, the weighting setter); eps_min:
// svnicp_set_residual_gicp's lower bound
inline const char* score_objective_refusal(const ScoreObjective& o, double eps_min) {
  return first_refusal({
      {o.form < kScoreAsSolved || o.form > kScoreGicp, "unknown form (SVNICP_SCORE_AS_SOLVED, _POINT, _PLANE or _GICP)"},
      {!(o.gate > 0.0) || !(o.gate <= 1.7976931348623157e308), "max_corr_dist must be finite and positive"},
      {!(o.delta >= 0.0), "huber_delta must be positive (+inf: no robust weight) or 0 (the solver's own)"},
      {o.eps != 0.0 && !(o.eps >= eps_min && o.eps <= 1.0), "epsilon must be 0 (the solver's own) or in [1e-6, 1]"},
  });
}
// AS_SOLVED becomes the form of the residual that ran (or is about to run), with the solver's delta and epsilon; an
// explicit form keeps its own and takes the solver's where it says 0.  The point form has neither.
inline ScoreObjective resolve_score_objective(ScoreObjective o, bool ran_plane, bool ran_gicp, double solver_delta, double solver_eps) {
  if (o.form == kScoreAsSolved) {
    o.form = ran_gicp ? kScoreGicp : ran_plane ? kScorePlane : kScorePoint;
    o.delta = solver_delta; o.eps = solver_eps;
  }
  if (o.delta == 0.0) o.delta = solver_delta;
  if (o.eps == 0.0) o.eps = solver_eps;
  if (o.form == kScorePoint) o.delta = 0.0;
  if (o.form != kScoreGicp) o.eps = 0.0;
  return o;
}
// the normals a resolved form reads (no normal pass is ever run by a scoring)
inline const char* score_normals_refusal(int form, bool target_normals, bool source_normals) {
  return first_refusal({
      {form == kScorePlane && !target_normals, "form PLANE needs normals of the current target in the context (svnicp_set_target_normals, or a registration that estimated them)"},
      {form == kScoreGicp && !target_normals, "form GICP needs normals of the current target in the context (svnicp_set_target_normals, or a registration that estimated them)"},
      {form == kScoreGicp && !source_normals, "form GICP needs normals of the current source in the context (svnicp_set_source_normals, or a registration in generalized-ICP mode that estimated them)"},
  });
}
// weighting the particle set at the end of a registration (nullptr: nothing, or the weights are uniform).  The setters
// themselves refuse a non-finite or non-positive max_corr_dist or temperature.
inline const char* weighting_refusal(const RegistrationFacts& f, const Tuning& t) {
  if (f.weighting == 0) return nullptr;
  if (f.weighting != 1) return "unknown weighting kind";
  if (f.svgd) return "SVGD mode: the weight option belongs to SVNICP's constructor only";
  if (const char* why = scoring_refusal(f, t)) return why;
  return score_normals_refusal(f.weighting_form, f.target_normals, f.source_normals);
}
// pose prior: what it is not combined with (all left for later).  What passes runs the prior's launch between the sums and the
// Stein step: small_registration and plan_step keep the two shapes that have no place for it (SmallChain, single_fused) away.
inline const char* prior_refusal(const RegistrationFacts& f, const Tuning& t) {
  if (!f.prior) return nullptr;
  return first_refusal({
      {f.svgd, "SVGD mode: its gradient does not pass through the H | b record the prior is added to"},
      {f.shard_set && !f.whole_shard(), "a partial particle shard (svnicp_set_shard) is set"},
      {f.row_world > 1, "a source-row shard (svnicp_set_row_shard) is set"},
      {t.persistent != 0, "option chain=persistent is set"},
  });
}
// correspondence = full (the whole message): its per-particle searches feed the split accumulate kernel and run through
// stage A's working set with K = 1 (stage_a_k1: StageAPlan::can_search(1)).  An empty particle shard searches nothing.
inline const char* full_corr_refusal(const RegistrationFacts& f, const Tuning& t, int variant, bool stage_a_k1) {
  if (!t.full_corr || f.nshard() <= 0) return nullptr;
  return first_refusal({
      {variant != 3, "correspondence = full needs the split stage B (accum = split, more than 8 particles or knn_count <= 128)"},
      {!stage_a_k1, "correspondence = full needs knn_count <= 128 (Morton-tile stage A) or knn = v1"},
  });
}

// ---------------- stage B: variant and shape ----------------
struct AccumPlan { int PW, WP, TP, grid_x, grid_y, tiles_per_block, Ppad, RS, f32, K, sgrid_x, pts_per_block, spts_per_block; int64_t n_tiles; size_t smem;
                   int small; /* split variant, few (point, particle) pairs: at most kSmallChainBlocks accumulate workgroups (small_registration) */ };
constexpr int kSmallChainBlocks = 32;

// AccumPlan::f32: 0 = float64 baseline, 1 = float32 VALU search (fused with the accumulation), 3 = bf16 matrix-pipe search
// kernel + accumulation kernel.  Option accum asks; the MFMA tiles are 16 particles wide and 128 candidate rows deep, so
// K > 128 and shards of <= 8 particles get the fused f32 kernels instead — except that correspondence = full and the
// point-to-plane residual consume the split kernels' winner index and keep them for any particle count.
inline int stage_b_variant(int accum, int K, int nshard, bool full_corr, bool plane) {
  if (accum != 3) return accum;
  if (nshard <= 0 || K > 128 || (nshard <= 8 && !full_corr && !plane)) return 1;
  return 3;
}
// particles per wave (PW), waves along the particles (WP), workgroups along the particles, row stride; an empty shard has
// a variant and no grid
inline AccumPlan stage_b_shape(int variant, int nshard, int K) {
  AccumPlan pl{};
  pl.f32 = variant;
  if (nshard <= 0) return pl;
  int PW = variant == 3 ? 16 : 8;
  while (PW < 64 && PW < nshard) PW <<= 1;
  int WP = 1;
  if (PW == 64) { WP = (nshard + 63) / 64; if (WP >= 3) WP = 4; }
  pl.PW = PW; pl.WP = WP; pl.K = K;
  pl.grid_y = (nshard + PW * WP - 1) / (PW * WP);
  pl.Ppad = pl.grid_y * PW * WP;
  pl.RS = (3 * K) | 1;
  return pl;
}
// a run-time (PW, WP) of stage_b_shape's split layout as a compile-time tag: f(Lanes<PW, WP>{}) for the five geometries the
// lane <-> particle kernels are instantiated for, e.g.
//   dispatch_lanes(plan.PW, plan.WP, [&](auto l) { return launch<l.PW, l.WP>(plan, a, st); });
// (the stage-B kernels of stein_iter.hip also run PW = 8, shards of at most eight particles: they ask for it first)
template <int PW_, int WP_> struct Lanes { static constexpr int PW = PW_, WP = WP_; };
template <class F>
auto dispatch_lanes(int PW, int WP, F&& f) {
  switch (PW) {
    case 16: return f(Lanes<16, 1>{});
    case 32: return f(Lanes<32, 1>{});
    default:
      if (WP == 1) return f(Lanes<64, 1>{});
      if (WP == 2) return f(Lanes<64, 2>{});
      return f(Lanes<64, 4>{});
  }
}
// small registration (few pairs, one context holds everything, 2 <= P <= 128): the accumulate kernel runs at most
// kSmallChainBlocks workgroups (plan_accumulate clamps its grid), so the update kernels add their records themselves
inline bool small_registration(const AccumPlan& shape, const RegistrationFacts& f, const Tuning& t, int64_t Bi) {
  return shape.f32 == 3 && shape.grid_y == 1 && Bi * f.nshard() <= (1 << 19) && t.small_chain && f.P >= 2 && f.P <= 128 &&
         f.P <= t.fused_update_max_p && !t.update_fused && f.row_world == 1 && f.whole_shard() && !t.full_corr && !f.plane && !f.prior;
}
// the stage-B plan of a registration as far as it does not depend on the device
inline AccumPlan plan_stage_b(const RegistrationFacts& f, const Tuning& t, int64_t Bi) {
  AccumPlan pl = stage_b_shape(stage_b_variant(t.accum, f.K, f.nshard(), t.full_corr != 0, f.plane), f.nshard(), f.K);
  pl.small = small_registration(pl, f, t, Bi) ? 1 : 0;
  return pl;
}

// ---------------- stage A hands its result to stage B ----------------
// Does the select kernel of the tile family write the split variant's search table (rows, anchor, C_b) from the entries it
// has just ranked, instead of k_build_table3 gathering them again from cand_idx?  Only where the registration's own search
// covers the table's rows in one call: the tile kernels, the split stage B, no mini-batch (its table has one row per drawn
// position) and no particle shard (the host gathers the candidate rows of other contexts before the table is built).  The
// select kernel then stores no distances either: svnicp_get_candidate_dist2 recomputes them.  A call of
// svnicp_stage_candidates for a part of the rows is the sharded flow and keeps the gather.
inline bool select_writes_table(const RegistrationFacts& f, const Tuning& t, const StageAPlan& a, const AccumPlan& b) {
  return t.table_select && a.kernel == KnnKernel::Tiles && a.K == f.K && b.f32 == 3 && f.batch == 0 && !f.shard_set;
}

// Are the target and the registration's queries Morton-sorted by ONE radix sort (spatial_prep.hip:
// launch_morton_order_joint)?  Where the tile kernels' target layout has to be (re)built for this registration and its own
// search takes the whole source in one call; StageA then leaves the layout to that search.  Any other search that comes
// first (the plane residual's normal pass), a held target, row ranges of a sharded flow and mini-batch sort separately.
inline bool joint_morton_sort(const RegistrationFacts& f, const Tuning& t, const StageAPlan& a) {
  return t.sort_joint && a.kernel == KnnKernel::Tiles && a.rows == f.B && f.batch == 0 && !f.shard_set;
}

// ---------------- the Stein step ----------------
// which launches carry the Stein step of 2 <= P particles (P = 1 and option update=fused: OneKernel); chosen once per
// registration by plan_step at the end of svnicp_align_begin
enum class StepChain {
  // P = 1 (no pair statistics) and option update=fused: the whole Stein step is one one-workgroup kernel on the main stream
  OneKernel,
  // few (point, particle) pairs: the accumulate kernel runs at most kSmallChainBlocks workgroups, nothing reduces their records
  // (the prepare lanes add them), and the pair statistics share the prepare kernel's launch on the main stream
  SmallChain,
  // general chain, up to 128 particles (the one-workgroup pair statistics): they run as the last workgroup of the prepare
  // kernel's launch on the main stream.  The second stream hid their 12 us behind the search kernel, but its fork and join
  // (event record / wait on both sides, one more launch) cost more: C3 7.25 -> 6.99 ms, C2 2.72 -> 2.56 ms per registration,
  // and 0.25 ms less host time to enqueue a registration.  Above 128 particles the three-kernel chain stays on the second stream.
  InlineMedian,
  // the pair statistics of iteration `it` (bandwidth h from the exact median of the pair distances): they depend on the
  // poses only, so they are forked onto the second stream at the START of the iteration and run beside the search and
  // accumulate kernels; svnicp_iter_update joins before the Stein direction
  SideStream,
};
constexpr int kMedianInlineMaxP = 128;   // the one-workgroup pair statistics

struct StepPlan {
  StepChain chain = StepChain::OneKernel;
  // ONE particle, no exchange between ranks ahead, the fused f32 kernel: its last workgroup reduces the partial sums and
  // runs the Stein step (for P = 1 the Newton step and the pose update) — the iteration is this one launch
  bool single_fused = false;
};
// from the options and the stage-B plan of the registration (its variant and `small`)
inline StepPlan plan_step(const RegistrationFacts& f, const Tuning& t, const AccumPlan& pl) {
  StepPlan s;
  if (f.P < 2 || (t.update_fused && f.P <= t.fused_update_max_p)) s.chain = StepChain::OneKernel;
  else if (pl.small) s.chain = StepChain::SmallChain;
  else if (f.P <= kMedianInlineMaxP && f.P <= t.fused_update_max_p && t.median_inline != 0) s.chain = StepChain::InlineMedian;
  else s.chain = StepChain::SideStream;
  s.single_fused = f.P == 1 && !f.svgd && f.row_world == 1 && f.p_lo == 0 && f.p_hi == 1 && !t.full_corr && t.single_fused && pl.f32 == 1 &&
                   !f.plane && !f.prior;
  return s;
}

// (PW, WP) of the plan and knn_count for which the persistent kernel is instantiated (small_registration.hip:
// launch_small_registration; the others run the four-launch chain)
inline bool small_registration_supported(int PW, int WP, int K) {
  return K >= 97 && K <= 100 && ((WP == 1 && (PW == 16 || PW == 32 || PW == 64)) || (PW == 64 && WP == 2));
}

// ---------------- how svnicp_align / svnicp_align_async drive the iterations ----------------
// blocking svnicp_align with early stop: the stop flag follows every kChunk iterations into pinned memory
constexpr int kChunk = 4;   // (2: 1.29 ms at the shipped settings against 1.26 — the host then waits more often than it saves launches)
struct DrivePlan {
  bool persistent_try = false;   // all iterations in ONE cooperative launch, if the runtime takes it
  bool defer_fin = false;        // early stop: iteration i's decision is taken by iteration i + 1's search kernel (the last iteration keeps k_upd_finish)
  bool follow = false;           // the host enqueues in chunks and stops soon after the device has
};
inline DrivePlan plan_drive(const RegistrationFacts& f, const Tuning& t, const AccumPlan& pl, const StepPlan& s, bool blocking) {
  DrivePlan d;
  d.persistent_try = s.chain == StepChain::SmallChain && t.persistent && !f.record_trace && !f.profiling && f.I > 0 &&
                     small_registration_supported(pl.PW, pl.WP, f.K);
  d.defer_fin = f.check_early_stop && !f.record_trace && pl.f32 == 3 && !t.full_corr && s.chain != StepChain::OneKernel;
  d.follow = blocking && f.check_early_stop && f.I > 2 * kChunk;
  return d;
}

}  // namespace svnicp
