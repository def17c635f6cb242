// api.hip — the C ABI of libsvnicp_hip.so (include/svnicp_hip.h): context, device buffers,
// launch sequencing.  Host-side mirror of the reference's solver object state
// (include/core/SVGDICP.h:170-210): clouds, R0/t0, particles R_/t_, pose_particles_, history.
// What a registration decides is not here: stage A's kernel and sizes are stage_a_plan.hpp / stage_a_host.hpp, everything
// behind it (rows, refusals, stage-B variant and shape, step chain, how svnicp_align drives the iterations) is
// registration_plan.hpp, sized by stage_b_host.hpp.  svnicp_align_begin asks once and stores the answers.
// No CPU fallback: every compute entry point needs a gfx950 device and fails loudly without one.
#include "../../include/svnicp_hip.h"

#include <cmath>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "device_buffer.hpp"
#include "gicp_pair_device.hpp"
#include "information_solve.hpp"
#include "kernels.hpp"
#include "pose_prior.hpp"
#include "stage_a_host.hpp"
#include "stage_b_host.hpp"

using namespace svnicp;
using namespace svnicp_host;

namespace {

// the members of svnicp_ctx, grouped by what owns the fields
struct CloudState {   // the clouds as given (the re-ordered target copies are stage A's: stage_a_host.hpp)
  DevBuf<double> src, tgt;
  bool src_set = false, tgt_set = false;
};

struct SteinState {   // particle and Stein-step state
  DevBuf<double> init_pose, R, t, Rtot, pose_out, eul, opt, uctl, work, stats;
  DevBuf<float> history;
  DevBuf<int> ctl;
  int hist_I = 0, hist_P = 0;
  // pinned host staging: the initial particles go up and the result block (mean, variance, covariance, weights) comes down
  // without a stream synchronisation of their own
  PinnedBuf<double> h_init, h_stats;
  bool host_stats_valid = false;   // h_stats holds the last registration's results (after the stream has been synchronised)
  Event ev_init;
  bool init_in_flight = false;
  StepPlan step;     // the launches of this registration's Stein step (svnicp_align_begin; svnicp_set_option chooses again)
  DrivePlan drive;   // svnicp_align / svnicp_align_async: how their loop runs the iterations; defer_fin holds inside that loop only
  int single_done_it = -1;   // iteration whose Stein step the accumulate kernel's last workgroup has already enqueued (P = 1)
  Event ev_fork, ev_join;   // the second queue is forked from and joined into `stream`: the caller still sees one ordered queue
  bool median_pending = false;
  DevBuf<unsigned int> small_bar;   // persistent small-registration kernel: arrivals, generation, error word
  bool small_launched = false;      // the last svnicp_align_async ran the persistent kernel (its error word is checked at the next synchronisation)
  // blocking svnicp_align with early stop: the stop flag follows every few iterations into pinned memory, so that the host
  // stops enqueuing soon after the device has stopped (three slots, the host runs two chunks ahead)
  Event ev_chunk[3];
  PinnedBuf<int> h_flags;   // pinned [3]
  bool finish_seen = true;   // the stop flag of the last registration has been folded into finish_iter
  int finish_iter = 0;   // finish_iter_: constructor value, changed only by an SVGD-mode early stop (SVGDICP.cpp:42,128)
};

struct Sharding {   // row / particle sharding
  int p_lo = 0, p_hi = 0;
  bool set = false;
  // source-row sharding (svnicp_set_row_shard): this context holds rows of a larger scan; its per-iteration sums are one of
  // row_world partial records that the host all-gathers into rank_sums [row_world][P][22]
  int row_rank = 0, row_world = 1;
  int64_t B_total = 0;
  DevBuf<double> rank_sums;
};

// mini-batch (svnicp_set_minibatch / svnicp_set_minibatch_indices; csrc/minibatch.hip).  batch 0 = off.
struct MiniBatch {
  int batch = 0;
  uint64_t seed = 0, n = 0;         // generated tables: seed, registrations begun since svnicp_set_minibatch
  bool explicit_tab = false;        // an explicit table (tab [tab_I][batch]) instead of generated ones
  int tab_I = 0;
  std::vector<int32_t> tab_h;       // the explicit table when it came from host memory: range-checked on the host …
  int64_t tab_checked_B = -1;       // … once per source size
  bool on = false, have = false;    // this registration runs on a table; its taps are valid (stage A has been enqueued)
  bool check = false;               // an explicit DEVICE table: its validation flag is read at the next synchronisation
  int64_t rows = 0, nq = 0;         // iterations * batch; queries of stage A = min(B, rows)
  unsigned long long base = 0;
  DevBuf<int32_t> tab, idx, flag, pos, bsum, cand;
  DevBuf<int> ctl;
  DevBuf<double> src_u, src;
};

// point-to-plane residual (svnicp_set_residual; csrc/plane_icp.hip).  residual 0 = the reference's point-to-point
struct PlaneState {
  int residual = SVNICP_RESIDUAL_POINT;
  double delta = 0.1;
  int normal_k = 16;
  bool supplied = false;      // rec holds normals the caller gave for the current target (dropped by svnicp_set_target)
  bool estimated = false;     // rec holds normals estimated from the current target with est_k neighbours
  int est_k = 0;
  int64_t passes = 0;         // normal passes run since creation
  bool on = false;            // the registration begun last runs the plane residual
  DevBuf<double> rec;         // [M][6] xyz | unit normal, 0 = no normal here
  DevBuf<double> nsup;        // upload staging of supplied normals
  DevBuf<int32_t> nbr;        // [rows of one pass block][normal_k] neighbour indices
  DevBuf<double> nbr_d2;
  DevBuf<double> partial, Hb, stats;   // [grid_x][Ppad][kPlaneSums], [P][42], [P][2] (the last two allocated max(P, Ppad) rows long)
};

// generalized-ICP residual (svnicp_set_residual_gicp; csrc/gicp_icp.hip).  It runs in plane mode's place
// (PlaneState::residual == SVNICP_RESIDUAL_GICP, PlaneState::on, the same partial / Hb / stats) and adds the source's side.
struct GicpState {
  double eps = kGicpEpsilonDefault;
  bool supplied = false;      // rec holds normals the caller gave for the current source (dropped by svnicp_set_source)
  bool estimated = false;     // rec holds normals estimated from the current source with est_k neighbours
  int est_k = 0;
  int64_t passes = 0;         // source normal passes run since creation
  bool on = false;            // the registration begun last runs the generalized-ICP residual
  DevBuf<double> rec;         // [B][6] xyz | unit normal, 0 = no normal here
  DevBuf<double> nsup;        // upload staging of supplied normals
  StageA sa;                  // the source as its own target (M = B), planned for K = normal_k: the exact neighbours of the source's
                              // normal pass, block by block in its own result buffers cand_idx / cand_d2
  Pose0 ident{};              // … searched at the identity
};

// svnicp_evaluate (csrc/evaluate.hip): its own buffers, nothing of the registration's
struct EvalState {
  DevBuf<double> q, d2, partial, result;   // [B][3] transformed source, [B], [evaluate_blocks(B)][kEvalRecord], [kEvalResult]
  DevBuf<int32_t> idx;                     // [B]
  PinnedBuf<double> h_result;              // pinned [kEvalResult]
  bool have = false;                       // idx / d2 hold the rows of an evaluation of `rows` source rows
  int64_t rows = 0;
  // svnicp_eval_information (csrc/information.hip) reads the rows of the last evaluate: `have` is never
  // cleared (svnicp_get_eval_pairs keeps answering), `fresh` is — by the source, target and normals setters and by
  // svnicp_align_begin — and holds again once an evaluate has succeeded
  bool fresh = false;
  const char* stale = "no svnicp_evaluate yet";   // why not, for the refusal
  void mark_stale(const char* why) { fresh = false; if (have) stale = why; }
  bool normals = false;                    // that evaluate's has_normals
  double max_corr_dist = 0.0;              // its gate
  EvalPose T{};                            // its pose
  DevBuf<double> info_partial, info_result;   // [evaluate_blocks(B)][record of the form], [kInfoResult]
  PinnedBuf<double> h_info;                // pinned [kInfoResult]
};

// svnicp_score_particles / svnicp_set_particle_weighting (csrc/particle_score.hip): its own buffers
struct ScoreState {
  int kind = SVNICP_WEIGHT_UNIFORM;        // what the next registration ends with
  ScoreObjective cfg;                      // … scored in this objective, as configured (svnicp_set_particle_weighting: the point cost at its gate)
  double temperature = 0.0;
  ScoreObjective begun;                    // cfg resolved by the svnicp_align_begin of the registration begun last
  ScoreObjective last;                     // the resolved objective of the scoring `scores` holds (svnicp_get_score_objective)
  bool on = false;                         // the registration begun last ends with a scoring and weighted statistics
  const char* reg_refusal = nullptr;       // why the registration begun last cannot be scored (registration_plan.hpp: scoring_refusal)
  DevBuf<double> partial, scores, poses, w;   // [score_blocks(B)][Ppad][kScoreRecord], [P][kScoreFields], [P][12], [P]
  bool have = false;                       // scores / poses hold a scoring of `P` particles
  int P = 0;
  bool of_result = false;                  // … of the particles pose_out holds now: cleared by svnicp_align_begin and svnicp_set_particles
};

// svnicp_particle_modes (csrc/particle_modes.hip): its own buffers
struct ModesState {
  DevBuf<double> in_pose, in_w;            // a caller's set: [6][P], [P]
  DevBuf<double> result;                   // modes_result_bytes(P)
  PinnedBuf<double> h_in, h_result;        // pinned staging of a caller's set; of the result block and the labels behind it
  bool have = false;                       // h_result holds the labels of a clustering of `P` particles
  int P = 0;
};

// Gaussian pose prior on the correction (svnicp_set_pose_prior; csrc/pose_prior.hip)
struct PriorState {
  bool set = false;             // what the next registration runs with: mean6 / info36 as the getter returns them, `next` as the kernel takes them
  double mean6[6] = {}, info36[36] = {};
  PosePrior next{};
  bool on = false;              // the registration begun last runs with `args`
  PosePrior args{};
  DevBuf<double> rec;           // [P][42] = H | b with the prior added: what the Stein-step kernels read through UpdateArgs::plane_Hb
};

struct Trace { DevBuf<double> H, b, N, phi, h; DevBuf<int32_t> corr; };   // record_trace

struct Profiling {   // timing events
  Event ev[3];   // registration begin, candidate table built, finish (svnicp_get_gpu_ms)
  // optional per-kernel-class timing (svnicp_set_profile): event pairs around every launch
  bool on = false;
  unsigned mask = 0;                    // classes that are bracketed (bit = class index)
  int pcur = -1;                        // class of the open bracket, -1 = none
  std::vector<Event> pev;               // pairs: [2*i] start, [2*i+1] stop
  std::vector<int> pcls;                // kernel class of pair i
  size_t pused = 0;
};

struct DebugCounters {   // option debug (stage A keeps its own: StageA::dbg_phase)
  DevBuf<unsigned long long> upd;     // phase cycles of k_particle_update
};

struct Progress {   // of the registration
  bool particles_set = false, began = false, have_candidates = false, have_result = false;
  bool table_built = false;   // stage A's select kernel has written the search table: svnicp_build_candidate_table launches nothing
  bool d2_due = false;        // … and stored no distances: svnicp_get_candidate_dist2 recomputes them first, once
};

}  // namespace

struct svnicp_ctx {
  svnicp_params prm{};
  int device = 0, num_cus = 256;
  // the streams come before every buffer: members are destroyed in reverse order.  `side` is the second queue: the pair
  // statistics of the Stein step (they need the poses only) run there, beside the stage-B kernels of the same iteration
  Stream own_stream, side;
  hipStream_t stream = nullptr;   // own_stream, or the caller's (svnicp_set_stream)
  std::string err;
  static std::string& create_error() { thread_local std::string s; return s; }   // svnicp_last_error(nullptr)

  int64_t B = 0, M = 0;
  int K = 0, P = 0;
  Pose0 pose0{};
  Tuning tune{};
  CloudState cloud; StageA sa; StageB sb; SteinState st;
  Sharding shard; MiniBatch mb; PlaneState pl; GicpState gi; PriorState pr; EvalState ev; ScoreState sc; ModesState md;
  Trace tr; Profiling prof; DebugCounters dbg; Progress run;
};

// Tuning::fused_update_max_p default 128: measured crossover (C3: equal, P=256: 4.5x); above it the Stein step runs as
// workgroup-parallel kernels
enum { KC_KNN = 0, KC_TABLE = 1, KC_SEARCH = 2, KC_ACCUM = 3, KC_REDUCE = 4, KC_UPDATE = 5, KC_COUNT = SVNICP_KERNEL_CLASSES };

static hipError_t prof_begin(svnicp_ctx* c, int cls) {
  c->prof.pcur = -1;
  if (!c->prof.on || !((c->prof.mask >> cls) & 1u)) return hipSuccess;
  c->prof.pcur = cls;
  if (c->prof.pused * 2 + 2 > c->prof.pev.size()) {
    for (int i = 0; i < 2; ++i) {
      Event e;
      hipError_t r = e.create();
      if (r != hipSuccess) return r;
      c->prof.pev.push_back(std::move(e));
    }
    c->prof.pcls.push_back(cls);
  }
  c->prof.pcls[c->prof.pused] = cls;
  return hipEventRecord(c->prof.pev[2 * c->prof.pused], c->stream);
}
static hipError_t prof_end(svnicp_ctx* c) {
  if (!c->prof.on || c->prof.pcur < 0) return hipSuccess;
  c->prof.pcur = -1;
  hipError_t r = hipEventRecord(c->prof.pev[2 * c->prof.pused + 1], c->stream);
  c->prof.pused += 1;
  return r;
}

#define CTX_CHECK(ctx) do { if (!(ctx)) return SVNICP_ERR_INVALID; } while (0)

static int bind(svnicp_ctx* c) {
  HIPCHK(c, hipSetDevice(c->device));
  return 0;
}

static StageAEnv stage_a_env(const svnicp_ctx* c) {
  return {c->stream, c->tune, c->num_cus, c->prm.record_trace != 0, c->cloud.tgt.p, c->B, c->M, c->pose0};
}

// stage A's view of the source cloud as a target of its own (the source's normal pass in generalized-ICP mode)
static StageAEnv source_stage_a_env(const svnicp_ctx* c) {
  return {c->stream, c->tune, c->num_cus, false, c->cloud.src.p, c->B, c->B, c->gi.ident};
}

// what the rules of registration_plan.hpp read of the context; plane, gicp, prior: what this registration runs with (gicp
// runs the plane residual's launch shape: plane is then set as well)
static RegistrationFacts registration_facts(const svnicp_ctx* c, bool plane, bool gicp, bool prior) {
  RegistrationFacts f;
  f.P = c->P; f.K = c->K; f.I = c->prm.iterations; f.B = c->B; f.M = c->M;
  f.svgd = c->prm.mode == SVNICP_MODE_SVGD; f.check_early_stop = c->prm.check_early_stop != 0; f.record_trace = c->prm.record_trace != 0;
  f.profiling = c->prof.on;
  f.shard_set = c->shard.set; f.p_lo = c->shard.p_lo; f.p_hi = c->shard.p_hi; f.row_world = c->shard.row_world;
  f.batch = c->mb.batch; f.explicit_tab = c->mb.explicit_tab; f.tab_I = c->mb.tab_I;
  f.plane = plane || gicp; f.normals_supplied = c->pl.supplied; f.normal_k = c->pl.normal_k;
  f.gicp = gicp; f.source_normals_supplied = c->gi.supplied;
  f.weighting = c->sc.kind;
  f.weighting_form = resolve_score_objective(c->sc.cfg, f.plane, gicp, c->pl.delta, c->gi.eps).form;
  f.target_normals = f.plane || c->pl.supplied || c->pl.estimated;
  f.source_normals = gicp || c->gi.supplied || c->gi.estimated;
  f.prior = prior;
  return f;
}

extern "C" {

int svnicp_abi_version(void) { return SVNICP_ABI_VERSION; }

const char* svnicp_last_error(const svnicp_ctx* ctx) { return ctx ? ctx->err.c_str() : svnicp_ctx::create_error().c_str(); }

int svnicp_create(const svnicp_params* params, int device, const double* init_pose6xP, int P, svnicp_ctx** out) {
  if (!params || !out) return fail<svnicp_ctx>(nullptr, SVNICP_ERR_INVALID, "svnicp_create: null argument");
  if (params->struct_size != (int32_t)sizeof(svnicp_params))
    return fail<svnicp_ctx>(nullptr, SVNICP_ERR_INVALID, "svnicp_create: svnicp_params.struct_size mismatch");
  if (params->iterations < 0 || params->knn_count < 1)
    return fail<svnicp_ctx>(nullptr, SVNICP_ERR_INVALID, "svnicp_create: iterations >= 0 and knn_count >= 1 required");
  if (params->mode != SVNICP_MODE_SVN && params->mode != SVNICP_MODE_SVGD)
    return fail<svnicp_ctx>(nullptr, SVNICP_ERR_INVALID, "svnicp_create: unknown mode");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail<svnicp_ctx>(nullptr, SVNICP_ERR_NO_DEVICE, "svnicp_create: no HIP device visible (this library has no CPU path)");
  if (device < 0 || device >= ndev) return fail<svnicp_ctx>(nullptr, SVNICP_ERR_INVALID, "svnicp_create: bad device ordinal");
  hipDeviceProp_t prop;
  if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess)
    return fail<svnicp_ctx>(nullptr, SVNICP_ERR_HIP, "svnicp_create: hipGetDeviceProperties failed");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail<svnicp_ctx>(nullptr, SVNICP_ERR_NO_DEVICE,
                std::string("svnicp_create: device is ") + prop.gcnArchName + ", this library carries gfx950 code only");
  svnicp_ctx* c = new svnicp_ctx();
  c->prm = *params;
  c->device = device;
  c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  c->K = params->knn_count;
  c->st.finish_iter = params->iterations;
  const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  std::memcpy(c->pose0.R0, I3, sizeof I3);  // SVGDICP.cpp:38-39
  c->pose0.t0[0] = c->pose0.t0[1] = c->pose0.t0[2] = 0.0;
  if (c->own_stream.create(hipStreamNonBlocking) != hipSuccess) { delete c; return fail<svnicp_ctx>(nullptr, SVNICP_ERR_HIP, "svnicp_create: hipStreamCreate failed"); }
  if (c->side.create(hipStreamNonBlocking) != hipSuccess ||
      c->st.ev_fork.create(hipEventDisableTiming) != hipSuccess || c->st.ev_join.create(hipEventDisableTiming) != hipSuccess ||
      c->st.ev_init.create(hipEventDisableTiming) != hipSuccess) {
    delete c;
    return fail<svnicp_ctx>(nullptr, SVNICP_ERR_HIP, "svnicp_create: hipStreamCreate / hipEventCreate failed");
  }
  c->stream = c->own_stream;
  for (auto& e : c->prof.ev)
    if (e.create() != hipSuccess) { delete c; return fail<svnicp_ctx>(nullptr, SVNICP_ERR_HIP, "hipEventCreate failed"); }
  if (c->st.ctl.ensure(4) != hipSuccess) { delete c; return fail<svnicp_ctx>(nullptr, SVNICP_ERR_NOMEM, "hipMalloc failed"); }
  *out = c;
  if (const char* e = getenv("SVNICP_OPTIONS")) {   // read ONCE, at creation: "name=value;name=value" for profiling scripts
    std::string all(e);
    size_t pos = 0;
    while (pos < all.size()) {
      const size_t end = all.find(';', pos) == std::string::npos ? all.size() : all.find(';', pos);
      const std::string kv = all.substr(pos, end - pos);
      const size_t eq = kv.find('=');
      if (eq != std::string::npos && svnicp_set_option(c, kv.substr(0, eq).c_str(), kv.substr(eq + 1).c_str()) != 0) {
        svnicp_ctx::create_error() = c->err; svnicp_destroy(c); *out = nullptr; return SVNICP_ERR_INVALID;
      }
      pos = end + 1;
    }
  }
  if (init_pose6xP) {
    int rc = svnicp_set_particles(c, init_pose6xP, P);
    if (rc != 0) { svnicp_ctx::create_error() = c->err; svnicp_destroy(c); *out = nullptr; return rc; }
  }
  return SVNICP_OK;
}

void svnicp_destroy(svnicp_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->side) (void)hipStreamSynchronize(c->side);
  delete c;
}

int svnicp_set_stream(svnicp_ctx* c, void* hip_stream) {
  CTX_CHECK(c);
  if (bind(c)) return SVNICP_ERR_HIP;
  HIPCHK(c, hipStreamSynchronize(c->stream));  // nothing of ours may still be in flight on the old stream
  c->stream = hip_stream == SVNICP_OWN_STREAM ? c->own_stream : reinterpret_cast<hipStream_t>(hip_stream);
  return SVNICP_OK;
}

static int check_small_kernel(svnicp_ctx* c);
static int check_minibatch_table(svnicp_ctx* c);
int svnicp_synchronize(svnicp_ctx* c) {
  CTX_CHECK(c);
  if (bind(c)) return SVNICP_ERR_HIP;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (const int rc = check_small_kernel(c)) return rc;
  if (const int rc = check_minibatch_table(c)) return rc;
  if (c->run.have_result && c->st.h_stats.p) c->st.host_stats_valid = true;   // svnicp_finish's copy of the result block has landed
  return SVNICP_OK;
}

// copy a caller's [n][3] cloud (host or device memory) into `buf` on the context's stream
static int upload_cloud(svnicp_ctx* c, DevBuf<double>& buf, const double* xyz, int64_t n, int mem_kind) {
  if (bind(c)) return SVNICP_ERR_HIP;
  HIPCHK(c, buf.ensure((size_t)n * 3));
  const hipMemcpyKind kind = mem_kind == SVNICP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIPCHK(c, hipMemcpyAsync(buf.p, xyz, (size_t)n * 24, kind, c->stream));
  if (mem_kind != SVNICP_MEM_DEVICE) HIPCHK(c, hipStreamSynchronize(c->stream));  // caller may reuse its host buffer
  c->run.have_candidates = false;
  return SVNICP_OK;
}

int svnicp_set_source(svnicp_ctx* c, const double* src, int64_t B, int mem_kind) {
  CTX_CHECK(c);
  if (!src || B < 1) return fail(c, SVNICP_ERR_INVALID, "svnicp_set_source: need B >= 1");
  if (const char* why = cloud_rows_refusal(B)) return fail(c, SVNICP_ERR_INVALID, std::string("svnicp_set_source: ") + why);
  if (const int rc = upload_cloud(c, c->cloud.src, src, B, mem_kind)) return rc;
  c->B = B;
  c->cloud.src_set = true;
  c->gi.supplied = false; c->gi.estimated = false;   // normals belong to the source they were given or estimated for
  c->ev.mark_stale("the source changed since the last svnicp_evaluate");
  return SVNICP_OK;
}

int svnicp_set_target(svnicp_ctx* c, const double* tgt, int64_t M, int mem_kind) {
  CTX_CHECK(c);
  if (!tgt || M < 1) return fail(c, SVNICP_ERR_INVALID, "svnicp_set_target: need M >= 1");
  if (const char* why = cloud_rows_refusal(M)) return fail(c, SVNICP_ERR_INVALID, std::string("svnicp_set_target: ") + why);
  if (const int rc = upload_cloud(c, c->cloud.tgt, tgt, M, mem_kind)) return rc;
  c->M = M;
  c->sa.held = TargetLayout::None;  // the SoA copies are (re)built in svnicp_align_begin, once K is final
  c->cloud.tgt_set = true;
  c->pl.supplied = false; c->pl.estimated = false;   // normals belong to the target they were given or estimated for
  c->ev.mark_stale("the target changed since the last svnicp_evaluate");
  return SVNICP_OK;
}

int svnicp_set_clouds(svnicp_ctx* c, const double* src, int64_t B, const double* tgt, int64_t M, int mem_kind) {
  CTX_CHECK(c);
  if (!src || !tgt || B < 1 || M < 1) return fail(c, SVNICP_ERR_INVALID, "svnicp_set_clouds: need B >= 1, M >= 1");
  if (const char* why = cloud_rows_refusal(M > B ? M : B)) return fail(c, SVNICP_ERR_INVALID, std::string("svnicp_set_clouds: ") + why);
  if (const int rc = svnicp_set_source(c, src, B, mem_kind)) return rc;
  return svnicp_set_target(c, tgt, M, mem_kind);
}

int svnicp_set_particles(svnicp_ctx* c, const double* init, int P) {
  CTX_CHECK(c);
  if (!init || P < 1) return fail(c, SVNICP_ERR_INVALID, "svnicp_set_particles: need P >= 1");
  if (bind(c)) return SVNICP_ERR_HIP;
  HIPCHK(c, c->st.init_pose.ensure((size_t)P * 6));
  HIPCHK(c, c->st.R.ensure((size_t)P * 9));
  HIPCHK(c, c->st.t.ensure((size_t)P * 3));
  HIPCHK(c, c->st.Rtot.ensure((size_t)P * 12));
  HIPCHK(c, c->st.pose_out.ensure((size_t)P * 6));
  HIPCHK(c, c->sb.sums.ensure((size_t)P * kNSums));
  HIPCHK(c, c->st.stats.ensure((size_t)48 + P));
  HIPCHK(c, c->st.work.ensure(update_workspace_doubles(P)));
  HIPCHK(c, c->st.eul.ensure((size_t)P * 6));
  HIPCHK(c, c->st.opt.ensure((size_t)P * 18));
  HIPCHK(c, c->st.uctl.ensure(update_uctl_doubles(P)));
  // through pinned staging: the caller's buffer is free when this returns and the stream is not synchronised (a second
  // call before the first copy has run would overwrite the staging area: wait for the stream only then)
  if ((size_t)P * 6 > c->st.h_init.cap || (size_t)P + 48 > c->st.h_stats.cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, c->st.h_init.alloc((size_t)P * 6));
    HIPCHK(c, c->st.h_stats.alloc((size_t)P + 48));
  } else if (c->st.init_in_flight) {
    HIPCHK(c, hipEventSynchronize(c->st.ev_init));
  }
  std::memcpy(c->st.h_init.p, init, (size_t)P * 48);
  HIPCHK(c, hipMemcpyAsync(c->st.init_pose.p, c->st.h_init.p, (size_t)P * 48, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->st.ev_init, c->stream));
  c->st.init_in_flight = true;
  c->st.host_stats_valid = false;
  const bool first = !c->run.particles_set || P != c->P;
  if (P != c->P) c->sc.have = false;   // the last scoring was of another particle count
  c->sc.of_result = false;
  if (first && c->shard.row_world > 1) { c->shard.row_world = 1; c->shard.row_rank = 0; c->shard.B_total = 0; }   // the record array is sized by P: set the row shard again
  c->P = P;
  if (!c->shard.set || first) { c->shard.p_lo = 0; c->shard.p_hi = P; c->shard.set = false; }
  // ctor semantics: pose_particles_ is formed from the initial pose (SVNICP.cpp:36-37, SVGDICP.cpp:33-35);
  // add_cloud semantics: R_, t_ are reset, pose_particles_ is left alone (SVGDICP.cpp:46-62)
  HIPCHK(c, launch_init_particles(c->st.init_pose.p, P, c->pose0, c->prm.mode, c->st.R.p, c->st.t.p, c->st.Rtot.p, c->st.pose_out.p,
                                  (first || c->prm.mode == SVNICP_MODE_SVN) ? 1 : 0, c->st.eul.p, c->stream));
  c->run.particles_set = true;
  return SVNICP_OK;
}

int svnicp_set_initial_mean(svnicp_ctx* c, const double R0[9], const double t0[3]) {
  CTX_CHECK(c);
  if (!R0 || !t0) return fail(c, SVNICP_ERR_INVALID, "svnicp_set_initial_mean: null argument");
  std::memcpy(c->pose0.R0, R0, 9 * sizeof(double));
  std::memcpy(c->pose0.t0, t0, 3 * sizeof(double));
  c->run.have_candidates = false;
  return SVNICP_OK;
}

int svnicp_set_k(svnicp_ctx* c, int k) {
  CTX_CHECK(c);
  if (k < 1) return fail(c, SVNICP_ERR_INVALID, "svnicp_set_k: k >= 1 required");
  c->K = k;
  c->run.have_candidates = false;
  return SVNICP_OK;
}

int svnicp_set_max_dist(svnicp_ctx* c, double md) {
  CTX_CHECK(c);
  c->prm.max_dist = md;
  return SVNICP_OK;
}

int svnicp_set_option(svnicp_ctx* c, const char* name, const char* value) {
  CTX_CHECK(c);
  if (!name || !value) return fail(c, SVNICP_ERR_INVALID, "svnicp_set_option: null argument");
  const std::string k(name), v(value);
  Tuning& t = c->tune;
  auto num = [&](int lo, int hi, int* out) { char* end = nullptr; const long x = strtol(v.c_str(), &end, 10);
                                             if (end == v.c_str() || *end || x < lo || x > hi) return false; *out = (int)x; return true; };
  bool ok = true;
  if (k == "knn") { if (v == "auto") t.knn = {}; else if (v == "v1") t.knn = {false, KnnKernel::Stream}; else if (v == "v2") t.knn = {false, KnnKernel::SeededScan};
                    else if (v == "brute") t.knn = {false, KnnKernel::Brute}; else if (v == "tiles") t.knn = {false, KnnKernel::Tiles}; else ok = false; }
  else if (k == "knn_prefilter") { if (v == "mfma") t.knn_prefilter_mfma = 1; else if (v == "valu") t.knn_prefilter_mfma = 0; else ok = false; }
  else if (k == "seed_rank") { if (v == "bounded") t.seed_rank_full = 0; else if (v == "full") t.seed_rank_full = 1; else ok = false; }
  else if (k == "fallback_sliced_max") ok = num(-1, 1 << 20, &t.fallback_sliced_max);
  else if (k == "accum") { if (v == "f64") t.accum = 0; else if (v == "valu") t.accum = 1; else if (v == "split") t.accum = 3; else ok = false; }
  else if (k == "update") { if (v == "auto") t.update_fused = 0; else if (v == "fused") t.update_fused = 1; else ok = false; }
  else if (k == "fused_update_max_p") ok = num(1, 700, &t.fused_update_max_p);   // P = 1 has no pair statistics; the fused kernel's LDS ends near P = 800
  else if (k == "wgpcu") { int x = 0, y = 0; ok = sscanf(v.c_str(), "%d,%d", &x, &y) == 2 && x >= 0 && x <= 64 && y >= 0 && y <= 16; if (ok) { t.wgpcu_search = x; t.wgpcu_accum = y; } }
  else if (k == "tp") ok = num(0, 1 << 16, &t.tp);
  else if (k == "debug") ok = num(0, 1, &t.debug);
  else if (k == "scan_split") ok = num(0, 16, &t.scan_split);
  else if (k == "group_stride") ok = num(0, 1 << 30, &t.group_stride);
  else if (k == "accum_min_steps") ok = num(0, 1 << 20, &t.accum_min_steps);
  else if (k == "brute_qb") { ok = num(0, 6, &t.brute_qb); }   // queries per workgroup of k_knn_brute, 0 = automatic
  else if (k == "single") { if (v == "fused") t.single_fused = 1; else if (v == "split") t.single_fused = 0; else ok = false; }
  else if (k == "chain") { if (v == "auto") { t.small_chain = 1; t.persistent = 0; } else if (v == "persistent") { t.small_chain = 1; t.persistent = 1; }
                           else if (v == "general") { t.small_chain = 0; t.persistent = 0; } else ok = false; }
  else if (k == "median") { if (v == "auto") t.median_inline = -1; else if (v == "stream") t.median_inline = 0; else if (v == "inline") t.median_inline = 1; else ok = false; }
  else if (k == "sort") { if (v == "joint") t.sort_joint = 1; else if (v == "separate") t.sort_joint = 0; else ok = false; }
  else if (k == "sort_kernel") { if (v == "radix") t.sort_merge = 0; else if (v == "merge") t.sort_merge = 1; else ok = false; }
  else if (k == "table") { if (v == "select") t.table_select = 1; else if (v == "gather") t.table_select = 0; else ok = false; }
  else if (k == "correspondence") { if (v == "fast") t.full_corr = 0; else if (v == "full") t.full_corr = 1; else ok = false; }
  else return fail(c, SVNICP_ERR_INVALID, "svnicp_set_option: unknown option '" + k + "'");
  if (!ok) return fail(c, SVNICP_ERR_INVALID, "svnicp_set_option: bad value '" + v + "' for option '" + k + "'");
  c->run.have_candidates = false;
  c->sa.held = TargetLayout::None;
  // svnicp_iter_accumulate now refuses until the next svnicp_align_begin; svnicp_iter_update goes on and follows the new options
  if (c->run.began) c->st.step = plan_step(registration_facts(c, c->pl.on, c->gi.on, c->pr.on), c->tune, c->sb.plan);
  return SVNICP_OK;
}

int svnicp_set_shard(svnicp_ctx* c, int p_lo, int p_hi) {
  CTX_CHECK(c);
  if (!c->run.particles_set || p_lo < 0 || p_hi > c->P || p_lo > p_hi)
    return fail(c, SVNICP_ERR_INVALID, "svnicp_set_shard: need 0 <= p_lo <= p_hi <= P after svnicp_set_particles");
  c->shard.p_lo = p_lo; c->shard.p_hi = p_hi; c->shard.set = true;
  return SVNICP_OK;
}

int svnicp_set_row_shard(svnicp_ctx* c, int row_rank, int row_world, int64_t total_source_points) {
  CTX_CHECK(c);
  if (!c->run.particles_set || row_world < 1 || row_rank < 0 || row_rank >= row_world || (row_world > 1 && total_source_points < 1))
    return fail(c, SVNICP_ERR_INVALID, "svnicp_set_row_shard: need 0 <= row_rank < row_world and the whole scan's point count, after svnicp_set_particles");
  if (bind(c)) return SVNICP_ERR_HIP;
  c->shard.row_rank = row_rank; c->shard.row_world = row_world;
  c->shard.B_total = row_world > 1 ? total_source_points : 0;
  if (row_world > 1) {
    HIPCHK(c, c->shard.rank_sums.ensure((size_t)row_world * c->P * kNSums));
    // a rank whose particle shard is empty in a 2-D split never writes its record: keep it defined
    HIPCHK(c, hipMemsetAsync(c->shard.rank_sums.p, 0, (size_t)row_world * c->P * kNSums * sizeof(double), c->stream));
  }
  return SVNICP_OK;
}

void* svnicp_rank_sums_devptr(svnicp_ctx* c) { return (c && c->shard.row_world > 1) ? (void*)c->shard.rank_sums.p : nullptr; }

// plane mode: this registration estimates the target's normals itself — none were supplied, and the ones at hand were not
// estimated from this target with this normal_k
static bool normal_pass_due(const svnicp_ctx* c) {
  return c->pl.on && !c->pl.supplied && !(c->pl.estimated && c->pl.est_k == c->pl.normal_k);
}

static bool source_normal_pass_due(const svnicp_ctx* c) {
  return c->gi.on && !c->gi.supplied && !(c->gi.estimated && c->gi.est_k == c->pl.normal_k);
}

static int prepare_plane(svnicp_ctx* c);
static int prepare_gicp(svnicp_ctx* c);
int svnicp_align_begin(svnicp_ctx* c) {
  CTX_CHECK(c);
  if (!c->cloud.src_set || !c->cloud.tgt_set || !c->run.particles_set)
    return fail(c, SVNICP_ERR_INVALID, "svnicp_align: svnicp_set_clouds and svnicp_set_particles must come first");
  if (bind(c)) return SVNICP_ERR_HIP;
  const int I = c->prm.iterations, P = c->P;
  const int64_t B = c->B;
  const bool gicp = c->pl.residual == SVNICP_RESIDUAL_GICP;
  const bool plane = c->pl.residual == SVNICP_RESIDUAL_PLANE || gicp;   // the generalized-ICP residual runs in the plane residual's place
  const RegistrationFacts f = registration_facts(c, plane, gicp, c->pr.set);
  if (const char* why = minibatch_refusal(f, c->tune)) return fail(c, SVNICP_ERR_INVALID, std::string(kMinibatchRefusal) + why);
  if (c->mb.batch != 0 && c->mb.explicit_tab && !c->mb.tab_h.empty() && c->mb.tab_checked_B != B) {
    for (const int32_t v : c->mb.tab_h)
      if (v < 0 || (int64_t)v >= B)
        return fail(c, SVNICP_ERR_INVALID, "svnicp_align: the mini-batch index table holds " + std::to_string(v) + ", outside [0, " + std::to_string(B) + ")");
    c->mb.tab_checked_B = B;
  }
  if (const char* why = gicp_refusal(f, c->tune)) return fail(c, SVNICP_ERR_INVALID, std::string(kGicpRefusal) + why);
  if (!gicp)
    if (const char* why = plane_refusal(f, c->tune)) return fail(c, SVNICP_ERR_INVALID, std::string(kPlaneRefusal) + why);
  if (const char* why = weighting_refusal(f, c->tune)) return fail(c, SVNICP_ERR_INVALID, std::string(kWeightingRefusal) + why);
  if (f.weighting && score_tile_rows(P, c->K, true) < 1)
    return fail(c, SVNICP_ERR_INVALID, std::string(kWeightingRefusal) + "knn_count is too large for one row's candidates to fit the scoring kernel's LDS tile");
  if (const char* why = prior_refusal(f, c->tune)) return fail(c, SVNICP_ERR_INVALID, std::string(kPriorRefusal) + why);
  const RegistrationRows r = registration_rows(c->mb.batch, I, B);
  const AccumPlan shape = plan_stage_b(f, c->tune, r.Bi);
  // (the stage-A plan StageA::begin is about to make: every refusal comes before the context changes)
  const bool stage_a_k1 = StageA::plan_for(stage_a_env(c), r.Bq, c->K).can_search(1);
  if (const char* why = full_corr_refusal(f, c->tune, shape.f32, stage_a_k1)) return fail(c, SVNICP_ERR_INVALID, why);
  c->pl.on = plane; c->gi.on = gicp;
  c->pr.on = f.prior; c->pr.args = c->pr.next;
  c->ev.mark_stale("a registration began after the last svnicp_evaluate");   // svnicp_eval_information wants one afterwards
  c->sc.on = f.weighting != 0; c->sc.reg_refusal = scoring_refusal(f, c->tune);
  c->sc.begun = resolve_score_objective(c->sc.cfg, plane, gicp, c->pl.delta, c->gi.eps);
  c->mb.on = r.mb; c->mb.have = false; c->mb.check = false;
  c->mb.rows = r.mb ? r.Bt : 0;
  c->mb.nq = r.mb ? r.Bq : 0;
  HIPCHK(c, hipEventRecord(c->prof.ev[0], c->stream));
  // stage A: kernel, scratch for every search of this registration (its own, the normal pass, correspondence = full), layout
  const bool joint = joint_morton_sort(f, c->tune, StageA::plan_for(stage_a_env(c), r.Bq, c->K));
  if (const int rc = c->sa.begin(c, stage_a_env(c), r.Bq, c->K, {c->K, normal_pass_due(c) ? c->pl.normal_k : c->K, c->tune.full_corr ? 1 : c->K}, joint)) return rc;
  c->sa.writes_table = select_writes_table(f, c->tune, c->sa.plan, shape);   // decided here, once; the calls below only follow it
  c->run.table_built = false; c->run.d2_due = false;
  if (r.mb) {
    HIPCHK(c, c->mb.idx.ensure((size_t)r.Bt)); HIPCHK(c, c->mb.flag.ensure((size_t)B)); HIPCHK(c, c->mb.pos.ensure((size_t)B));
    HIPCHK(c, c->mb.bsum.ensure((size_t)minibatch_scan_blocks(B))); HIPCHK(c, c->mb.ctl.ensure(2));
    HIPCHK(c, c->mb.src_u.ensure((size_t)r.Bq * 3)); HIPCHK(c, c->mb.src.ensure((size_t)r.Bt * 3));
    HIPCHK(c, c->mb.cand.ensure((size_t)r.Bt * c->K));
  }
  if (const int rc = c->sb.begin(c, f, c->tune, r, shape, c->num_cus)) return rc;
  if (c->pr.on) HIPCHK(c, c->pr.rec.ensure((size_t)P * 42));
  HIPCHK(c, c->st.history.ensure((size_t)(I > 0 ? I : 1) * 6 * P));
  c->st.hist_I = I; c->st.hist_P = P;
  if (c->prm.record_trace) {
    const size_t IP = (size_t)I * P;
    HIPCHK(c, c->tr.corr.ensure(IP * r.Bi));
    HIPCHK(c, hipMemsetAsync(c->tr.corr.p, 0xff, IP * r.Bi * 4, c->stream));
    const struct { DevBuf<double>& buf; size_t n; } dbl[] = {{c->tr.H, IP * 36}, {c->tr.b, IP * 6}, {c->tr.N, IP * 6}, {c->tr.phi, IP * 6}, {c->tr.h, (size_t)I + 1}};
    for (const auto& x : dbl) {
      HIPCHK(c, x.buf.ensure(x.n));
      HIPCHK(c, hipMemsetAsync(x.buf.p, 0, x.n * 8, c->stream));
    }
  }
  c->prof.pused = 0;
  c->st.single_done_it = -1;
  if (c->st.median_pending) HIPCHK(c, hipStreamWaitEvent(c->stream, c->st.ev_join, 0));   // a registration that was abandoned between its two per-iteration calls
  c->st.median_pending = false;
  if (!c->st.finish_seen && c->prm.mode == SVNICP_MODE_SVGD && c->prm.check_early_stop) {
    // finish_iter_ is sticky across registrations (SVGDICP.cpp:42,128): fold the previous registration's stop flag in before
    // the control words are reset, in case nobody asked for svnicp_get_runtime in between (SVGD mode with early stop only)
    int v[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(v, c->st.ctl.p, sizeof v, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (v[0]) c->st.finish_iter = v[1];
    c->st.finish_seen = true;
  }
  // ONE launch for everything small that a registration starts from: control words {stop flag, finish_iter (SVGDICP.cpp:42)},
  // tickets / counters / pair histogram, the float32 history (SVGDICP.cpp:172-174), statistics counters, a fresh optimizer
  // state (SVGDICP.cpp:73,142-170) — and the total pose of iteration 0 from the CURRENT R_, t_ and R0, t0 (SVNICP.cpp:58-59).
  // (Five fill / copy launches before: 5-8 us each, a tenth of a scan-to-map registration.)
  {
    BeginZero z{};
    auto add = [&](void* p, size_t bytes) { if (p && bytes) { z.ptr[z.n] = static_cast<unsigned int*>(p); z.dwords[z.n] = (unsigned int)(bytes / 4); ++z.n; } };
    add(c->st.uctl.p, update_uctl_doubles(P) * sizeof(double));
    add(c->st.history.p, (size_t)(I > 0 ? I : 1) * 6 * P * sizeof(float));
    add(c->sb.ambig.p, 2 * sizeof(int));
    if (c->sa.plan.kernel == KnnKernel::Brute) add(c->sa.fail_count.p, sizeof(int));
    HIPCHK(c, c->st.small_bar.ensure(8));
    add(c->st.small_bar.p, 8 * sizeof(unsigned int));
    if (c->prm.mode == SVNICP_MODE_SVGD) add(c->st.opt.p, (size_t)P * 18 * sizeof(double));
    // stage A's joint search comes next (StageA::begin left the layout to it): the bounding box's minima (all ones) and maxima,
    // the largest coordinate and the fallback count start here too, instead of four fills between its kernels
    const bool sa_words = c->sa.layout_pending;
    if (sa_words) {
      add(c->sa.bbox.p + 3, 3 * sizeof(unsigned long long)); add(c->sa.emax.p, sizeof(unsigned long long)); add(c->sa.fail_count.p, sizeof(int));
      z.ones = reinterpret_cast<unsigned int*>(c->sa.bbox.p); z.ones_dwords = 6;
    }
    z.ctl = c->st.ctl.p; z.iterations = I;
    HIPCHK(c, launch_init_particles(c->st.init_pose.p, P, c->pose0, 2, c->st.R.p, c->st.t.p, c->st.Rtot.p, c->st.pose_out.p, 0,
                                    nullptr, c->stream, &z));
    c->sa.start_words_set = sa_words;
  }
  if (c->mb.batch > 0 && !c->mb.explicit_tab) {   // the table of the n-th registration after svnicp_set_minibatch
    c->mb.base = minibatch_stream_base(c->mb.seed, c->mb.n);
    c->mb.n += 1;
  }
  if (plane)
    if (const int rc = prepare_plane(c)) return rc;
  if (gicp)
    if (const int rc = prepare_gicp(c)) return rc;
  c->st.step = plan_step(f, c->tune, c->sb.plan);
  c->run.began = true;
  c->st.finish_seen = false;
  c->run.have_result = false;
  c->sc.of_result = false;   // the scoring at hand is of the previous registration's particles
  return SVNICP_OK;
}

// option debug: allocate and clear the phase counters of the Stein-step kernels (UpdateArgs::dbg)
static int ensure_dbg_upd(svnicp_ctx* c) {
  if (!c->tune.debug || c->dbg.upd.p) return SVNICP_OK;
  HIPCHK(c, c->dbg.upd.ensure(8));
  HIPCHK(c, hipMemset(c->dbg.upd.p, 0, 8 * sizeof(unsigned long long)));
  return SVNICP_OK;
}

// download and print dbg.upd: the separate launches' counters so far, or the persistent kernel's
static int print_update_phases(svnicp_ctx* c, bool persistent) {
  unsigned long long h[8];
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!persistent) HIPCHK(c, hipStreamSynchronize(c->side));
  HIPCHK(c, hipMemcpy(h, c->dbg.upd.p, sizeof h, hipMemcpyDeviceToHost));
  if (persistent)
    fprintf(stderr, "[svnicp] k_small_registration, workgroup 0, cycles over %d iterations: search %llu | barrier %llu | accumulate %llu | barrier %llu | prepare %llu | barrier %llu | direction %llu | barrier %llu\n",
            c->prm.iterations, h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]);
  else
    fprintf(stderr, "[svnicp] Stein step thread-0 cycles (summed over launches so far; fused kernel: prepare / median / direction / pose / tail; k_upd_median: state / histogram / bin scan / collect / rank): %llu %llu %llu %llu %llu\n", h[0], h[1], h[2], h[3], h[4]);
  return SVNICP_OK;
}

// plane mode, end of svnicp_align_begin: the per-registration buffers, and the target's normals when none were supplied and
// the ones at hand were not estimated from this target with this normal_k.  The neighbours come from stage A itself (target
// as the query cloud, identity pose, K = normal_k) in blocks of the rows its scratch is sized for.
static int prepare_plane(svnicp_ctx* c) {
  HIPCHK(c, c->pl.partial.ensure((size_t)c->sb.plan.grid_x * c->sb.plan.Ppad * kPlaneSums));
  // (room for the padded particles of the stage-B grid, which no kernel writes: the kernel-by-kernel tests watch those rows)
  const size_t rec_rows = (size_t)std::max(c->P, c->sb.plan.Ppad);
  HIPCHK(c, c->pl.Hb.ensure(rec_rows * 42));
  HIPCHK(c, c->pl.stats.ensure(rec_rows * 2));
  HIPCHK(c, hipMemsetAsync(c->pl.stats.p, 0, (size_t)c->P * 2 * sizeof(double), c->stream));
  const int kn = c->pl.normal_k;
  if (!normal_pass_due(c)) return SVNICP_OK;
  if (!c->sa.plan.can_search(kn))
    return fail(c, SVNICP_ERR_INVALID, "svnicp_align: the seeded-scan stage A (option knn=v2, or a target beyond the tile kernel's range) cannot "
                                       "search with normal_k neighbours: supply the normals (svnicp_set_target_normals)");
  const int64_t M = c->M, rows = c->sa.block_rows(M);
  HIPCHK(c, c->pl.rec.ensure((size_t)M * 6));
  HIPCHK(c, c->pl.nbr.ensure((size_t)rows * kn));
  HIPCHK(c, c->pl.nbr_d2.ensure((size_t)rows * kn));
  const int rc = c->sa.search_blocks(c, stage_a_env(c), c->cloud.tgt.p, M, kn, c->pl.nbr.p, c->pl.nbr_d2.p, 0, [&](int64_t lo, int64_t n) {
    HIPCHK(c, launch_target_normals(c->cloud.tgt.p, M, c->pl.nbr.p, lo, n, kn, c->pl.rec.p, c->stream));
    return (int)SVNICP_OK;
  });
  if (rc) return rc;
  c->pl.estimated = true; c->pl.est_k = kn;
  c->pl.passes += 1;
  return SVNICP_OK;
}

// generalized-ICP mode, behind prepare_plane: the source's record [B][6], estimated when no source normals were supplied and
// the ones at hand were not estimated from this source with this normal_k.  The same per-point kernel as the target's pass;
// the neighbours come from a stage A of the mode's own whose target is the source cloud (M = B), so whichever kernel family
// it plans gives the exact normal_k nearest source points.  That stage A is planned for K = normal_k itself, so every family
// can search (prepare_plane's refusal of the seeded scan is for a K other than the plan's), and its result buffers
// [B][normal_k] hold one block's neighbour lists at a time.
static int prepare_gicp(svnicp_ctx* c) {
  const int kn = c->pl.normal_k;
  if (!source_normal_pass_due(c)) return SVNICP_OK;
  GicpState& g = c->gi;
  g.ident = Pose0{};
  g.ident.R0[0] = g.ident.R0[4] = g.ident.R0[8] = 1.0;
  const int64_t B = c->B;
  const StageAEnv env = source_stage_a_env(c);
  g.sa.held = TargetLayout::None;   // the layout at hand is of an earlier source
  if (const int rc = g.sa.begin(c, env, B, kn, {kn})) return rc;
  HIPCHK(c, g.rec.ensure((size_t)B * 6));
  const int rc = g.sa.search_blocks(c, env, c->cloud.src.p, B, kn, g.sa.cand_idx.p, g.sa.cand_d2.p, 0, [&](int64_t lo, int64_t n) {
    HIPCHK(c, launch_target_normals(c->cloud.src.p, B, g.sa.cand_idx.p, lo, n, kn, g.rec.p, c->stream));
    return (int)SVNICP_OK;
  });
  if (rc) return rc;
  g.estimated = true; g.est_k = kn;
  g.passes += 1;
  return SVNICP_OK;
}

int svnicp_stage_candidates(svnicp_ctx* c, int64_t b_lo, int64_t b_hi) {
  CTX_CHECK(c);
  if (!c->run.began) return fail(c, SVNICP_ERR_INVALID, "svnicp_stage_candidates: call svnicp_align_begin first");
  if (b_lo < 0 || b_hi > c->B || b_lo > b_hi) return fail(c, SVNICP_ERR_INVALID, "svnicp_stage_candidates: bad row range");
  if (bind(c)) return SVNICP_ERR_HIP;
  if (c->mb.on) {
    // mini-batch: draw (or validate) the table, compact the drawn rows, stage A on those, expand to the epoch-major layout
    if (b_lo != 0 || b_hi != c->B)
      return fail(c, SVNICP_ERR_INVALID, "svnicp_stage_candidates: in mini-batch mode only the whole range (0, B) is accepted");
    MinibatchArgs m{};
    m.explicit_idx = c->mb.explicit_tab ? c->mb.tab.p : nullptr; m.idx = c->mb.idx.p; m.n = c->mb.rows; m.B = c->B; m.base = c->mb.base;
    m.flag = c->mb.flag.p; m.pos = c->mb.pos.p; m.block_sums = c->mb.bsum.p; m.mbctl = c->mb.ctl.p; m.ctl = c->st.ctl.p;
    m.src = c->cloud.src.p; m.src_u = c->mb.src_u.p; m.n_q = c->mb.nq;
    HIPCHK(c, prof_begin(c, KC_KNN));
    HIPCHK(c, launch_minibatch_draw_compact(m, c->stream));
    const int rc = c->sa.search(c, stage_a_env(c), c->mb.src_u.p, c->pose0, c->K, c->sa.cand_idx.p, c->sa.cand_d2.p, 0, c->mb.nq);
    if (rc) return rc;
    HIPCHK(c, launch_minibatch_expand(m, c->sa.cand_idx.p, c->K, c->mb.src.p, c->mb.cand.p, c->stream));
    HIPCHK(c, prof_end(c));
    c->mb.have = true;
    c->mb.check = c->mb.explicit_tab && c->mb.tab_h.empty();
    return SVNICP_OK;
  }
  HIPCHK(c, prof_begin(c, KC_KNN));
  // the whole source in one search, planned to hand the table over (a part of the rows is the sharded flow: gather)
  const bool whole = b_lo == 0 && b_hi == c->B;
  const bool hand_over = c->sa.writes_table && whole;
  const TableOut tbl{c->sb.tablea.p, c->sb.anchor.p, c->sb.cmaxb.p};
  if (const int rc = c->sa.search(c, stage_a_env(c), c->cloud.src.p, c->pose0, c->K, c->sa.cand_idx.p, c->sa.cand_d2.p, b_lo, b_hi,
                                  hand_over ? &tbl : nullptr, whole)) return rc;
  c->run.table_built = hand_over; c->run.d2_due = hand_over;
  if (c->tune.full_corr)   // the per-particle searches of every iteration reuse stage A's fallback list
    if (const int rc = c->sa.keep_stage_fallbacks(c, stage_a_env(c))) return rc;
  HIPCHK(c, prof_end(c));
  return SVNICP_OK;
}


int svnicp_build_candidate_table(svnicp_ctx* c) {
  CTX_CHECK(c);
  if (!c->run.began) return fail(c, SVNICP_ERR_INVALID, "svnicp_build_candidate_table: call svnicp_align_begin first");
  if (bind(c)) return SVNICP_ERR_HIP;
  if (c->mb.on && !c->mb.have) return fail(c, SVNICP_ERR_INVALID, "svnicp_build_candidate_table: call svnicp_stage_candidates(0, B) first");
  HIPCHK(c, prof_begin(c, KC_TABLE));
  const int32_t* cand = c->mb.on ? c->mb.cand.p : c->sa.cand_idx.p;   // mini-batch: one table row per drawn position
  const int64_t rows = c->mb.on ? c->mb.rows : c->B;
  if (!c->run.table_built)
    if (const int rc = c->sb.build_table(c, cand, rows, c->K, c->cloud.tgt.p, c->M, c->stream)) return rc;
  HIPCHK(c, prof_end(c));
  HIPCHK(c, hipEventRecord(c->prof.ev[1], c->stream));
  c->run.have_candidates = true;
  return SVNICP_OK;
}

// argument block of the Stein-step kernels for iteration `it`; with_prior = false: as a registration without a pose prior
// would get it — what the prior's own kernel forms its base record from
static UpdateArgs update_args(svnicp_ctx* c, int it, bool with_prior = true) {
  UpdateArgs u{};
  u.sums = c->shard.row_world > 1 ? c->shard.rank_sums.p : c->sb.sums.p; u.n_ranks = c->shard.row_world; u.R = c->st.R.p; u.t = c->st.t.p; u.Rtot = c->st.Rtot.p; u.pose = c->pose0;
  u.P = c->P; u.iteration = it; u.iterations = c->prm.iterations;
  u.lr = c->prm.lr; u.conv_thr = c->prm.convergence_threshold;
  u.check_early_stop = c->prm.check_early_stop; u.full_grad = c->prm.svn_full_grad;
  u.work = c->st.work.p; u.history = c->st.history.p; u.pose_out = c->st.pose_out.p; u.ctl = c->st.ctl.p;
  if (c->prm.record_trace) {
    u.trH = c->tr.H.p + (size_t)it * c->P * 36; u.trb = c->tr.b.p + (size_t)it * c->P * 6;
    u.trN = c->tr.N.p + (size_t)it * c->P * 6; u.trphi = c->tr.phi.p + (size_t)it * c->P * 6; u.trh = c->tr.h.p + it;
  }
  u.eul = c->st.eul.p; u.opt = c->st.opt.p; u.optimizer = c->prm.optimizer;
  u.n_src = (double)(c->shard.row_world > 1 ? c->shard.B_total : c->B);   // gradient_scaling_factor_ = the whole scan's size (SVGDICP.cpp:58)
  u.uctl = c->st.uctl.p;
  u.dbg = c->tune.debug ? c->dbg.upd.p : nullptr;
  u.svgd = c->prm.mode == SVNICP_MODE_SVGD ? 1 : 0;
  u.plane_Hb = c->pl.on ? c->pl.Hb.p : nullptr;
  if (with_prior && c->pr.on) u.plane_Hb = c->pr.rec.p;   // H | b come finished from k_pose_prior, in point mode too
  return u;
}
// argument block of the stage-B kernels for iteration `it` (full_idx: set by the correspondence = full search)
static AccumArgs accum_args(svnicp_ctx* c, int it) {
  AccumArgs a{};
  a.src = c->cloud.src.p; a.table = c->sb.table.p; a.tablef = c->sb.tablef.p; a.tablea = c->sb.tablea.p; a.kbest = c->sb.kbest.p; a.kidx = c->sb.kidx.p; a.tgt = c->cloud.tgt.p; a.cand = c->sa.cand_idx.p; a.anchor = c->sb.anchor.p; a.M = c->M; a.cmax = c->sb.cmaxb.p; a.ambig_count = c->sb.ambig.p;
  a.Rtot = c->st.Rtot.p; a.B = c->B; a.K = c->K;
  a.p_lo = c->shard.p_lo; a.p_hi = c->shard.p_hi; a.max_dist = c->prm.max_dist; a.partial = c->sb.partial.p; a.ctl = c->st.ctl.p;
  a.corr = c->prm.record_trace ? c->tr.corr.p + (size_t)it * c->P * c->B : nullptr;
  if (c->mb.on) {
    // mini-batch: the rows of this iteration lie contiguously at [it * batch, (it + 1) * batch) of the epoch-major tables, so
    // the kernels see a cloud of `batch` rows; kbest / kidx / partial are per-iteration scratch
    const size_t r0 = (size_t)it * c->mb.batch;
    a.src = c->mb.src.p + 3 * r0; a.cand = c->mb.cand.p + r0 * c->K; a.cmax = c->sb.cmaxb.p + r0; a.B = c->mb.batch;
    if (c->sb.table.p) a.table = c->sb.table.p + r0 * c->K * 3;
    if (c->sb.tablef.p) a.tablef = c->sb.tablef.p + r0 * c->K;
    if (c->sb.tablea.p) a.tablea = c->sb.tablea.p + r0 * 128;
    if (c->sb.anchor.p) a.anchor = c->sb.anchor.p + 3 * r0;
    if (c->prm.record_trace) a.corr = c->tr.corr.p + (size_t)it * c->P * c->mb.batch;
  }
  a.svgd = c->prm.mode == SVNICP_MODE_SVGD ? 1 : 0;
  a.fin_iteration = -1;
  if (c->st.drive.defer_fin && it >= 1) {   // the previous iteration's early-stop decision rides on this iteration's search launch
    const UpdateArgs up = update_args(c, it - 1);
    a.fin_iteration = it - 1; a.fin_P = c->P; a.fin_thr = c->prm.convergence_threshold; a.fin_norms = update_step_norms(up);
    a.fin_pose = c->st.pose_out.p; a.fin_history = c->st.history.p; a.fin_ctl = c->st.ctl.p;
  }
  a.ticket = reinterpret_cast<unsigned int*>(c->st.uctl.p + 41);
  return a;
}

// svnicp_align's own loop (defer_fin): iteration `it`'s early-stop decision is taken by iteration it + 1's search kernel, so
// its direction kernel is not followed by k_upd_finish; the last iteration keeps it
static bool step_finishes(const svnicp_ctx* c, int it) { return !(c->st.drive.defer_fin && it < c->prm.iterations - 1); }

// side-stream chain: fork the pair statistics of iteration `it` onto the second stream (once per iteration)
static int fork_median(svnicp_ctx* c, int it) {
  if (c->st.step.chain != StepChain::SideStream || c->st.median_pending) return SVNICP_OK;
  if (const int rc = ensure_dbg_upd(c)) return rc;
  const UpdateArgs u = update_args(c, it);
  HIPCHK(c, hipEventRecord(c->st.ev_fork, c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->side, c->st.ev_fork, 0));
  HIPCHK(c, launch_update_median(u, c->num_cus, c->tune.fused_update_max_p, c->side));
  HIPCHK(c, hipEventRecord(c->st.ev_join, c->side));
  c->st.median_pending = true;
  return SVNICP_OK;
}

int svnicp_iter_accumulate(svnicp_ctx* c, int it) {
  CTX_CHECK(c);
  if (!c->run.began || !c->run.have_candidates)
    return fail(c, SVNICP_ERR_INVALID, "svnicp_iter_accumulate: candidates not staged");
  if (it < 0 || it >= c->prm.iterations) return fail(c, SVNICP_ERR_INVALID, "svnicp_iter_accumulate: bad iteration");
  if (bind(c)) return SVNICP_ERR_HIP;
  if (const int rc = fork_median(c, it)) return rc;
  const int nshard = c->shard.p_hi - c->shard.p_lo;
  if (nshard <= 0) return SVNICP_OK;
  AccumArgs a = accum_args(c, it);
  if (c->tune.full_corr) {
    // correspondence = full (the reference's get_correspondence, SVGDICP.cpp:274-298): every particle's transformed source
    // against the WHOLE target, K = 1 — P exact nearest-neighbour searches per iteration through the stage-A machinery
    // (svnicp_align_begin has refused what this needs and does not have, and sized full_q / full_d2 / full_idx)
    HIPCHK(c, prof_begin(c, KC_SEARCH));
    for (int p = c->shard.p_lo; p < c->shard.p_hi; ++p) {
      HIPCHK(c, launch_transform_cloud(c->cloud.src.p, c->B, c->st.Rtot.p + 12 * (size_t)p, c->sb.full_q.p, c->st.ctl.p, c->stream));
      if (const int rc = c->sa.search_blocks(c, stage_a_env(c), c->sb.full_q.p, c->B, 1, c->sb.full_idx.p + (size_t)p * c->B, c->sb.full_d2.p, 1)) return rc;
    }
    HIPCHK(c, prof_end(c));
    a.full_idx = c->sb.full_idx.p;
  } else if (c->sb.plan.f32 == 3) {
    HIPCHK(c, prof_begin(c, KC_SEARCH));
    HIPCHK(c, launch_search_split(c->sb.plan, a, c->stream));
    HIPCHK(c, prof_end(c));
  }
  if (c->pl.on) {   // point-to-plane: the winner's record, Huber weight, H and b directly ([P][42] for the Stein step)
    HIPCHK(c, prof_begin(c, KC_ACCUM));
    if (c->gi.on) {   // generalized ICP: the same place, inputs and records, and the source's record beside the target's
      GicpArgs ga{};
      ga.srec = c->gi.rec.p; ga.rec = c->pl.rec.p; ga.Rtot = c->st.Rtot.p; ga.B = c->B; ga.M = c->M; ga.p_lo = c->shard.p_lo; ga.p_hi = c->shard.p_hi;
      ga.max_dist = c->prm.max_dist; ga.delta = c->pl.delta; ga.eps = c->gi.eps; ga.partial = c->pl.partial.p; ga.ctl = c->st.ctl.p;
      ga.kidx = c->sb.kidx.p; ga.kbest = c->sb.kbest.p; ga.corr = a.corr;
      HIPCHK(c, launch_gicp_accumulate(c->sb.plan, ga, c->stream));
    } else {
      PlaneArgs pa{};
      pa.src = c->cloud.src.p; pa.rec = c->pl.rec.p; pa.Rtot = c->st.Rtot.p; pa.B = c->B; pa.M = c->M; pa.p_lo = c->shard.p_lo; pa.p_hi = c->shard.p_hi;
      pa.max_dist = c->prm.max_dist; pa.delta = c->pl.delta; pa.partial = c->pl.partial.p; pa.ctl = c->st.ctl.p;
      pa.kidx = c->sb.kidx.p; pa.kbest = c->sb.kbest.p; pa.corr = a.corr;
      HIPCHK(c, launch_plane_accumulate(c->sb.plan, pa, c->stream));
    }
    HIPCHK(c, prof_end(c));
    HIPCHK(c, prof_begin(c, KC_REDUCE));
    HIPCHK(c, launch_plane_finalize(c->pl.partial.p, c->sb.plan.grid_x, c->sb.plan.Ppad, c->shard.p_lo, nshard, c->pl.Hb.p, c->pl.stats.p,
                                    c->st.ctl.p, c->stream));
    HIPCHK(c, prof_end(c));
    return SVNICP_OK;
  }
  const bool single = c->st.step.single_fused;   // the iteration is this one launch
  const UpdateArgs us = update_args(c, it);
  HIPCHK(c, prof_begin(c, KC_ACCUM));
  HIPCHK(c, launch_accumulate(c->sb.plan, a, single ? &us : nullptr, c->stream));
  HIPCHK(c, prof_end(c));
  if (single) { c->st.single_done_it = it; return SVNICP_OK; }
  if (c->st.step.chain == StepChain::SmallChain) return SVNICP_OK;   // the update kernels add the workgroups' records themselves
  HIPCHK(c, prof_begin(c, KC_REDUCE));
  // one rank: the particle's record; source-row sharding: this rank's slot of the [row_world][P][22] array
  double* rec = c->shard.row_world > 1 ? c->shard.rank_sums.p + (size_t)c->shard.row_rank * c->P * kNSums : c->sb.sums.p;
  HIPCHK(c, launch_reduce_partials(c->sb.partial.p, c->sb.plan.grid_x, c->sb.plan.Ppad, c->shard.p_lo, nshard, rec, c->st.ctl.p, c->stream));
  HIPCHK(c, prof_end(c));
  return SVNICP_OK;
}

int svnicp_iter_update(svnicp_ctx* c, int it) {
  CTX_CHECK(c);
  if (!c->run.began) return fail(c, SVNICP_ERR_INVALID, "svnicp_iter_update: call svnicp_align_begin first");
  if (it < 0 || it >= c->prm.iterations) return fail(c, SVNICP_ERR_INVALID, "svnicp_iter_update: bad iteration");
  if (bind(c)) return SVNICP_ERR_HIP;
  if (c->st.single_done_it == it) { c->st.single_done_it = -1; return SVNICP_OK; }   // done by the accumulate kernel's last workgroup
  if (const int rc = ensure_dbg_upd(c)) return rc;
  UpdateArgs u = update_args(c, it);
  HIPCHK(c, prof_begin(c, KC_UPDATE));
  if (c->pr.on)   // the prior's record first: every launch shape below reads it in place of the sums or the plane record
    HIPCHK(c, launch_pose_prior(update_args(c, it, false), c->pr.args, c->pr.rec.p, c->stream));
  if (c->tune.debug && it == c->prm.iterations - 1)   // phase cycles of the one-workgroup kernels so far
    if (const int rc = print_update_phases(c, false)) return rc;
  const StepChain chain = c->st.step.chain;
  if (chain == StepChain::OneKernel) {
    u.svgd = 0;   // the one-workgroup kernels are per mode
    if (c->prm.mode == SVNICP_MODE_SVGD) HIPCHK(c, launch_update_svgd(u, c->stream));
    else HIPCHK(c, launch_update(u, c->stream));
  } else {
    if (chain == StepChain::SmallChain) {   // the accumulate workgroups' records, added by the prepare lanes
      u.sums = c->sb.partial.p; u.n_ranks = c->sb.plan.grid_x; u.sums_stride = c->sb.plan.Ppad * kNSums; u.sums_out = c->sb.sums.p;
    }
    if (chain == StepChain::SideStream) {
      // pair statistics: forked at the start of the iteration; a caller that skipped svnicp_iter_accumulate gets them here
      if (const int rc = fork_median(c, it)) return rc;
      HIPCHK(c, launch_update_prepare(u, c->stream));
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->st.ev_join, 0));
      c->st.median_pending = false;
    } else {
      HIPCHK(c, launch_update_prepare_median(u, c->stream));
    }
    HIPCHK(c, launch_update_direction(u, c->stream, step_finishes(c, it)));
  }
  HIPCHK(c, prof_end(c));
  return SVNICP_OK;
}

// k_particle_score + k_particle_score_finalize on the context's stream: sc.scores [P][6] and sc.poses [P][12] (a copy of the
// total poses that were scored: the next svnicp_set_particles rewrites Rtot), in the resolved objective `o` (the point form:
// the launches and arguments of svnicp_score_particles)
static int enqueue_scoring(svnicp_ctx* c, const ScoreObjective& o) {
  const bool normals = c->pl.supplied || c->pl.estimated;
  if (const char* why = score_normals_refusal(o.form, normals, c->gi.supplied || c->gi.estimated))
    return fail(c, SVNICP_ERR_INVALID, std::string(kScoringRefusal) + why);
  if (score_tile_rows(c->P, c->K, normals) < 1)
    return fail(c, SVNICP_ERR_INVALID, std::string(kScoringRefusal) + "knn_count is too large for one row's candidates to fit the scoring kernel's LDS tile");
  ScoreState& sc = c->sc;
  sc.have = false;
  HIPCHK(c, sc.partial.ensure((size_t)score_blocks(c->B) * score_padded_particles(c->P, c->K) * kScoreRecord));
  HIPCHK(c, sc.scores.ensure((size_t)c->P * kScoreFields));
  HIPCHK(c, sc.poses.ensure((size_t)c->P * 12));
  ScoreArgs a{};
  a.src = c->cloud.src.p; a.tgt = c->cloud.tgt.p; a.rec = normals ? c->pl.rec.p : nullptr; a.cand = c->sa.cand_idx.p; a.Rtot = c->st.Rtot.p;
  a.B = c->B; a.M = c->M; a.K = c->K; a.P = c->P; a.thr2 = o.gate * o.gate; a.partial = sc.partial.p;
  if (o.form != kScorePoint) {
    a.form = o.form; a.delta = o.delta; a.eps = o.eps; a.cap = robust_cost(o.gate, a.thr2, o.delta);
    a.srec = o.form == kScoreGicp ? c->gi.rec.p : nullptr;
  }
  HIPCHK(c, launch_particle_score(a, sc.scores.p, c->stream));
  HIPCHK(c, hipMemcpyAsync(sc.poses.p, c->st.Rtot.p, (size_t)c->P * 12 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  sc.have = true; sc.P = c->P; sc.of_result = true; sc.last = o;
  return SVNICP_OK;
}

int svnicp_finish(svnicp_ctx* c) {
  CTX_CHECK(c);
  if (!c->run.began) return fail(c, SVNICP_ERR_INVALID, "svnicp_finish: call svnicp_align_begin first");
  if (bind(c)) return SVNICP_ERR_HIP;
  HIPCHK(c, hipEventRecord(c->prof.ev[2], c->stream));
  StatsArgs s{c->st.pose_out.p, c->P, c->prm.mode, c->st.stats.p};
  if (c->sc.on) {   // one scoring at the poses the iterations left, the weights, the reference's weighted expressions
    if (const int rc = enqueue_scoring(c, c->sc.begun)) return rc;
    HIPCHK(c, c->sc.w.ensure((size_t)c->P));
    HIPCHK(c, launch_particle_weights(c->sc.scores.p, c->P, c->sc.temperature, c->sc.w.p, c->stream));
    HIPCHK(c, launch_stats_weighted(s, c->sc.w.p, c->stream));
  } else {
    HIPCHK(c, launch_stats(s, c->stream));
  }
  // the result block follows the kernels down the stream into pinned memory: the getters then cost no GPU round trip
  c->st.host_stats_valid = false;
  if (c->st.h_stats.p && (size_t)c->P + 48 <= c->st.h_stats.cap)
    HIPCHK(c, hipMemcpyAsync(c->st.h_stats.p, c->st.stats.p, ((size_t)c->P + 48) * 8, hipMemcpyDeviceToHost, c->stream));
  c->run.have_result = true;
  return SVNICP_OK;
}

int svnicp_stopped(svnicp_ctx* c) {
  CTX_CHECK(c);
  if (bind(c)) return SVNICP_ERR_HIP;
  int v[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(v, c->st.ctl.p, sizeof v, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return v[0] ? 1 : 0;
}

void* svnicp_candidates_devptr(svnicp_ctx* c) { return c ? (void*)c->sa.cand_idx.p : nullptr; }
void* svnicp_sums_devptr(svnicp_ctx* c) { return c ? (void*)c->sb.sums.p : nullptr; }
void* svnicp_total_pose_devptr(svnicp_ctx* c) { return c ? (void*)c->st.Rtot.p : nullptr; }   // AccumArgs::Rtot, [P][12]
// plane mode's record and statistics of the begun registration (prepare_plane sized them), and stage B's grid: test-only taps
void* svnicp_plane_record_devptr(svnicp_ctx* c) { return (c && c->run.began && c->pl.on) ? (void*)c->pl.Hb.p : nullptr; }
void* svnicp_particle_pose_devptr(svnicp_ctx* c, int which) {   // the correction poses R [P][9] (0) and t [P][3] (1)
  return (c && c->run.particles_set && (which == 0 || which == 1)) ? (void*)(which == 0 ? c->st.R.p : c->st.t.p) : nullptr;
}
void* svnicp_plane_stats_devptr(svnicp_ctx* c) { return (c && c->run.began && c->pl.on) ? (void*)c->pl.stats.p : nullptr; }
int svnicp_get_stage_b_grid(svnicp_ctx* c, int out4[4]) {
  CTX_CHECK(c);
  if (!out4) return fail(c, SVNICP_ERR_INVALID, "svnicp_get_stage_b_grid: null argument");
  if (!c->run.began) return fail(c, SVNICP_ERR_INVALID, "svnicp_get_stage_b_grid: call svnicp_align_begin first");
  out4[0] = c->sb.plan.grid_x; out4[1] = c->sb.plan.grid_y; out4[2] = c->sb.plan.pts_per_block; out4[3] = c->sb.plan.Ppad;
  return SVNICP_OK;
}

// follow_stop: the caller is going to wait for the result anyway (svnicp_align) — with early stop on, the host then enqueues
// the iterations in chunks and waits for the stop flag of the chunk before the previous one before it goes on: after the
// device has stopped it enqueues at most two more chunks of launches that return at once, instead of all the remaining
// iterations (the shipped configurations run 100 iterations with early stop and stop after 30-50: 350 empty launches were
// 1.1 ms of a 2.3 ms registration)
static int align_enqueue(svnicp_ctx* c, bool follow_stop) {
  CTX_CHECK(c);
  if (c->prm.mode == SVNICP_MODE_SVGD && (c->prm.optimizer < 0 || c->prm.optimizer > 3))
    return SVNICP_NO_OPTIMIZER;  // set_optimizer() found no optimizer: stein_align returns at once (SVGDICP.cpp:73-75)
  int rc = svnicp_align_begin(c);
  if (rc) return rc;
  if ((rc = svnicp_stage_candidates(c, 0, c->B))) return rc;
  if ((rc = svnicp_build_candidate_table(c))) return rc;
  c->st.small_launched = false;
  const DrivePlan drive = plan_drive(registration_facts(c, c->pl.on, c->gi.on, c->pr.on), c->tune, c->sb.plan, c->st.step, follow_stop);
  c->st.drive = drive;
  c->st.drive.defer_fin = false;   // holds inside the loop below only: not in the persistent kernel, not in a caller's own split-phase loop
  if (drive.persistent_try) {
    // all iterations in ONE cooperative launch (small_registration.hip: k_small_registration); anything the runtime refuses
    // (no cooperative launch, grid not resident) falls back to the four launches per iteration
    const AccumArgs a = accum_args(c, 0);   // defer_fin is off here: fin_iteration = -1, the search body decides nothing
    if ((rc = ensure_dbg_upd(c))) return rc;
    if (c->tune.debug) HIPCHK(c, hipMemsetAsync(c->dbg.upd.p, 0, 8 * sizeof(unsigned long long), c->stream));
    UpdateArgs u = update_args(c, 0);
    u.sums_out = c->sb.sums.p;
    const hipError_t e = launch_small_registration(c->sb.plan, a, u, c->prm.iterations, c->st.small_bar.p, c->num_cus, c->stream);
    if (e == hipSuccess && c->tune.debug)
      if ((rc = print_update_phases(c, true))) return rc;
    if (e == hipSuccess) { c->st.small_launched = true; return svnicp_finish(c); }
    (void)hipGetLastError();
  }
  c->st.drive.defer_fin = drive.defer_fin;
  struct Reset { bool& f; ~Reset() { f = false; } } reset_defer{c->st.drive.defer_fin};   // a caller's own split-phase loop keeps k_upd_finish
  if (drive.follow && !c->st.h_flags.p) {
    HIPCHK(c, c->st.h_flags.alloc(3));
    for (auto& e : c->st.ev_chunk) HIPCHK(c, e.create(hipEventDisableTiming));
  }
  for (int it = 0; it < c->prm.iterations; ++it) {
    if ((rc = svnicp_iter_accumulate(c, it))) return rc;
    if ((rc = svnicp_iter_update(c, it))) return rc;
    if (drive.follow && (it + 1) % kChunk == 0) {
      const int chunk = it / kChunk, slot = chunk % 3;
      HIPCHK(c, hipMemcpyAsync(&c->st.h_flags.p[slot], c->st.ctl.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipEventRecord(c->st.ev_chunk[slot], c->stream));
      if (chunk >= 1) {
        const int prev = (chunk - 1) % 3;
        HIPCHK(c, hipEventSynchronize(c->st.ev_chunk[prev]));
        if (c->st.h_flags.p[prev]) break;   // stopped: what is already enqueued returns at once, nothing more is needed
      }
    }
  }
  return svnicp_finish(c);
}
int svnicp_align_async(svnicp_ctx* c) { return align_enqueue(c, false); }

// the persistent kernel's barrier gives up after a bounded wait and says so in its error word
static int check_small_kernel(svnicp_ctx* c) {
  if (!c->st.small_launched) return SVNICP_OK;
  c->st.small_launched = false;
  unsigned int w[2] = {0u, 0u};
  HIPCHK(c, hipMemcpyAsync(w, c->st.small_bar.p, sizeof w, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (w[1] != 0u) { c->run.have_result = false; return fail(c, SVNICP_ERR_HIP, "svnicp_align: the small-registration kernel's grid barrier timed out (chain=persistent is an option; the default launches do not wait on each other)"); }
  return SVNICP_OK;
}

// an explicit mini-batch table in DEVICE memory is validated by the draw kernel: its flag is read once the stream has drained
static int check_minibatch_table(svnicp_ctx* c) {
  if (!c->mb.check) return SVNICP_OK;
  c->mb.check = false;
  int w[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(w, c->mb.ctl.p, sizeof w, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (w[0]) {
    c->run.have_result = false; c->st.finish_seen = true;   // nothing ran behind the flag: no result, no finish_iter to fold in
    return fail(c, SVNICP_ERR_INVALID, "svnicp_align: the mini-batch index table holds a value outside [0, B); the registration did not run");
  }
  return SVNICP_OK;
}

int svnicp_align(svnicp_ctx* c) {
  CTX_CHECK(c);
  if (c->shard.set && (c->shard.p_lo != 0 || c->shard.p_hi != c->P))
    return fail(c, SVNICP_ERR_INVALID, "svnicp_align: a particle shard is set; drive the split-phase calls instead");
  if (c->shard.row_world > 1)
    return fail(c, SVNICP_ERR_INVALID, "svnicp_align: a source-row shard is set (this context holds a partial record); drive the split-phase calls instead");
  int rc = align_enqueue(c, true);
  if (rc) return rc;  // negative status, or SVNICP_NO_OPTIMIZER
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((rc = check_small_kernel(c))) return rc;
  if ((rc = check_minibatch_table(c))) return rc;
  c->st.host_stats_valid = c->st.h_stats.p != nullptr;
  return SVNICP_ALIGN_SUCCESS;
}

static int fetch(svnicp_ctx* c, void* dst, const void* src, size_t bytes) {
  if (bind(c)) return SVNICP_ERR_HIP;
  HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SVNICP_OK;
}
#define NEED_RESULT(c)                                                                   \
  do {                                                                                   \
    CTX_CHECK(c);                                                                        \
    if (!(c)->run.have_result) return fail((c), SVNICP_ERR_INVALID, "no registration result yet"); \
  } while (0)

// mean[6] var[6] cov[36] weights[P]: from the pinned copy svnicp_finish queued when it has landed, else from the device
static int fetch_stats(svnicp_ctx* c, void* dst, size_t off_doubles, size_t n_doubles) {
  if (c->st.host_stats_valid) { std::memcpy(dst, c->st.h_stats.p + off_doubles, n_doubles * 8); return SVNICP_OK; }
  return fetch(c, dst, c->st.stats.p + off_doubles, n_doubles * 8);
}
int svnicp_get_transformation(svnicp_ctx* c, double out6[6]) { NEED_RESULT(c); return fetch_stats(c, out6, 0, 6); }
int svnicp_get_distribution(svnicp_ctx* c, double out6[6]) { NEED_RESULT(c); return fetch_stats(c, out6, 6, 6); }
int svnicp_get_cov_matrix(svnicp_ctx* c, double out36[36]) { NEED_RESULT(c); return fetch_stats(c, out36, 12, 36); }
int svnicp_get_particle_weight(svnicp_ctx* c, double* outP) {
  NEED_RESULT(c);
  return fetch_stats(c, outP, 48, (size_t)c->P);
}
int svnicp_get_particles(svnicp_ctx* c, double* out6P) {
  CTX_CHECK(c);
  if (!c->run.particles_set) return fail(c, SVNICP_ERR_INVALID, "no particles set");
  return fetch(c, out6P, c->st.pose_out.p, (size_t)c->P * 48);
}
int svnicp_get_particle_history(svnicp_ctx* c, float* out) {
  NEED_RESULT(c);
  return fetch(c, out, c->st.history.p, (size_t)c->st.hist_I * 6 * c->st.hist_P * sizeof(float));
}

int svnicp_get_gpu_ms(svnicp_ctx* c, double out3[3]) {
  NEED_RESULT(c);
  if (bind(c)) return SVNICP_ERR_HIP;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float a = 0, b = 0;
  HIPCHK(c, hipEventElapsedTime(&a, c->prof.ev[0], c->prof.ev[1]));
  HIPCHK(c, hipEventElapsedTime(&b, c->prof.ev[1], c->prof.ev[2]));
  out3[0] = a; out3[1] = b; out3[2] = (double)a + b;
  return SVNICP_OK;
}

int svnicp_get_runtime(svnicp_ctx* c, double out3[3]) {
  NEED_RESULT(c);
  double ms[3];
  int rc = svnicp_get_gpu_ms(c, ms);   // synchronises the stream
  if (rc) return rc;
  if (c->prm.mode == SVNICP_MODE_SVGD && c->prm.check_early_stop && !c->st.finish_seen) {
    // finish_iter_ = epoch + 1 on an SVGD-mode early stop (SVGDICP.cpp:128).  Read here rather than in svnicp_align so that
    // svnicp_align_async + svnicp_synchronize and the split-phase sequence (svnicp_iter_update … svnicp_finish) report it too
    int v[2] = {0, 0};
    HIPCHK(c, hipMemcpy(v, c->st.ctl.p, sizeof v, hipMemcpyDeviceToHost));
    if (v[0]) c->st.finish_iter = v[1];
    c->st.finish_seen = true;
  }
  // finish_iter_: SVNICP::stein_align never touches it (SVNICP.cpp:95-101 only breaks), SVGDICP::stein_align sets it on
  // an early stop and nothing resets it (SVGDICP.cpp:42,128)
  out3[0] = ms[0] * 1e-3; out3[1] = ms[1] * 1e-3; out3[2] = (double)c->st.finish_iter;
  return SVNICP_OK;
}

int svnicp_get_iterations_run(svnicp_ctx* c, int* out) {
  NEED_RESULT(c);
  if (!out) return SVNICP_ERR_INVALID;
  int v[2];
  const int rc = fetch(c, v, c->st.ctl.p, sizeof v);
  if (rc) return rc;
  *out = v[1];
  return SVNICP_OK;
}

int svnicp_get_knn_fallbacks(svnicp_ctx* c, int* out) {
  CTX_CHECK(c);
  if (!c->run.have_candidates) return fail(c, SVNICP_ERR_INVALID, "no candidates yet");
  const int* count = c->sa.fallback_count();
  if (!count) { *out = -1; return SVNICP_OK; }
  return fetch(c, out, count, sizeof(int));
}

int svnicp_get_knn_fallback_rows(svnicp_ctx* c, int32_t* out, int cap, int* n_out) {
  CTX_CHECK(c);
  if (!c->run.have_candidates || !n_out) return fail(c, SVNICP_ERR_INVALID, "no candidates yet");
  *n_out = 0;
  const int* count = c->sa.fallback_count();
  if (!count) return SVNICP_OK;
  int n = 0;
  int rc = fetch(c, &n, count, sizeof(int));
  if (rc) return rc;
  *n_out = n;
  if (n > cap) n = cap;
  if (n > 0 && out) return fetch(c, out, c->sa.fallback_rows(), (size_t)n * 4);
  return SVNICP_OK;
}

int svnicp_get_knn_survivors(svnicp_ctx* c, int32_t* outB) {
  CTX_CHECK(c);
  const int32_t* n = c->run.have_candidates ? c->sa.survivors(c->prm.record_trace != 0) : nullptr;
  if (!n) return fail(c, SVNICP_ERR_INVALID, "svnicp_get_knn_survivors: needs record_trace and the pruned stage-A kernel");
  return fetch(c, outB, n, (size_t)c->B * 4);
}

int svnicp_get_ambiguous_steps(svnicp_ctx* c, int* out) {
  NEED_RESULT(c);
  if (c->sb.plan.f32 == 0) { *out = -1; return SVNICP_OK; }
  return fetch(c, out, c->sb.ambig.p, sizeof(int));
}

int svnicp_get_ambiguous_pairs(svnicp_ctx* c, int64_t* out) {
  CTX_CHECK(c);
  if (!c->run.have_result || !out) return fail(c, SVNICP_ERR_INVALID, "no registration result yet");
  if (c->sb.plan.f32 != 3) { *out = -1; return SVNICP_OK; }   // counted by the bf16 search kernel only
  int v[2] = {0, 0};
  const int rc = fetch(c, v, c->sb.ambig.p, sizeof v);
  *out = v[1];
  return rc;
}

int svnicp_set_profile(svnicp_ctx* c, int on) {
  CTX_CHECK(c);
  c->prof.on = on != 0;
  c->prof.mask = on == 1 ? ~0u : ((unsigned)on >> 1);  // 1 = every class, else bit (class + 1) selects a class
  return SVNICP_OK;
}

int svnicp_get_kernel_ms(svnicp_ctx* c, double* ms5, int32_t* launches5) {  // SVNICP_KERNEL_CLASSES entries each
  NEED_RESULT(c);
  if (!c->prof.on) return fail(c, SVNICP_ERR_INVALID, "svnicp_get_kernel_ms: profiling is off (svnicp_set_profile)");
  if (bind(c)) return SVNICP_ERR_HIP;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < KC_COUNT; ++i) { ms5[i] = 0.0; launches5[i] = 0; }
  for (size_t i = 0; i < c->prof.pused; ++i) {
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->prof.pev[2 * i], c->prof.pev[2 * i + 1]));
    ms5[c->prof.pcls[i]] += ms;
    launches5[c->prof.pcls[i]] += 1;
  }
  return SVNICP_OK;
}

static const char* const kMbCandMsg = "mini-batch mode: stage A ran on the drawn rows only, use svnicp_get_minibatch_candidates";
int svnicp_get_candidates(svnicp_ctx* c, int32_t* out) {
  CTX_CHECK(c);
  if (!c->run.have_candidates) return fail(c, SVNICP_ERR_INVALID, "no candidates yet");
  if (c->mb.on) return fail(c, SVNICP_ERR_INVALID, std::string("svnicp_get_candidates: ") + kMbCandMsg);
  return fetch(c, out, c->sa.cand_idx.p, (size_t)c->B * c->K * 4);
}
int svnicp_get_candidate_dist2(svnicp_ctx* c, double* out) {
  CTX_CHECK(c);
  if (!c->run.have_candidates) return fail(c, SVNICP_ERR_INVALID, "no candidates yet");
  if (c->mb.on) return fail(c, SVNICP_ERR_INVALID, std::string("svnicp_get_candidate_dist2: ") + kMbCandMsg);
  if (c->run.d2_due) {   // the select kernel stored none: the same distances again from cand_idx (rows of the fallback kernels included)
    if (bind(c)) return SVNICP_ERR_HIP;
    HIPCHK(c, launch_candidate_dist2(c->cloud.src.p, c->pose0, c->cloud.tgt.p, c->M, c->sa.cand_idx.p, c->B, c->K, c->sa.cand_d2.p, c->stream));
    c->run.d2_due = false;
  }
  return fetch(c, out, c->sa.cand_d2.p, (size_t)c->B * c->K * 8);
}

// ---- SteinICPParam::use_minibatch / batch_size ----
int svnicp_set_minibatch(svnicp_ctx* c, int batch_size, uint64_t seed) {
  CTX_CHECK(c);
  c->mb.batch = batch_size;   // a negative value is refused by svnicp_align_begin
  c->mb.seed = seed; c->mb.n = 0;
  c->mb.explicit_tab = false; c->mb.tab_I = 0; c->mb.tab_h.clear(); c->mb.tab_checked_B = -1;
  c->run.have_candidates = false;
  return SVNICP_OK;
}

int svnicp_set_minibatch_indices(svnicp_ctx* c, const int32_t* idx, int iterations, int batch_size, int mem_kind) {
  CTX_CHECK(c);
  if (!idx || iterations < 1 || batch_size < 1)
    return fail(c, SVNICP_ERR_INVALID, "svnicp_set_minibatch_indices: need a table of iterations >= 1 rows of batch_size >= 1 indices");
  const int64_t n = (int64_t)iterations * batch_size;
  if (n > kMinibatchMaxRows) return fail(c, SVNICP_ERR_INVALID, "svnicp_set_minibatch_indices: iterations * batch_size exceeds 2^22 table rows");
  if (bind(c)) return SVNICP_ERR_HIP;
  HIPCHK(c, hipStreamSynchronize(c->stream));   // a registration in flight may still read the previous table
  HIPCHK(c, c->mb.tab.ensure((size_t)n));
  c->mb.tab_h.clear();
  if (mem_kind == SVNICP_MEM_DEVICE) {
    HIPCHK(c, hipMemcpyAsync(c->mb.tab.p, idx, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));
  } else {
    c->mb.tab_h.assign(idx, idx + n);
    HIPCHK(c, hipMemcpyAsync(c->mb.tab.p, c->mb.tab_h.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  c->mb.batch = batch_size; c->mb.explicit_tab = true; c->mb.tab_I = iterations; c->mb.tab_checked_B = -1;
  c->run.have_candidates = false;
  return SVNICP_OK;
}

#define NEED_MINIBATCH(c, what)                                                                                          \
  do {                                                                                                                   \
    CTX_CHECK(c);                                                                                                        \
    if (!(c)->mb.on || !(c)->mb.have) return fail((c), SVNICP_ERR_INVALID, what ": no registration in mini-batch mode yet"); \
  } while (0)
int svnicp_get_minibatch_indices(svnicp_ctx* c, int32_t* out) {
  NEED_MINIBATCH(c, "svnicp_get_minibatch_indices");
  return fetch(c, out, c->mb.idx.p, (size_t)c->mb.rows * 4);
}
int svnicp_get_minibatch_candidates(svnicp_ctx* c, int32_t* out) {
  NEED_MINIBATCH(c, "svnicp_get_minibatch_candidates");
  return fetch(c, out, c->mb.cand.p, (size_t)c->mb.rows * c->K * 4);
}
int svnicp_get_minibatch_rows(svnicp_ctx* c, int64_t out2[2]) {
  NEED_MINIBATCH(c, "svnicp_get_minibatch_rows");
  if (!out2) return SVNICP_ERR_INVALID;
  int w[2] = {0, 0};
  const int rc = fetch(c, w, c->mb.ctl.p, sizeof w);
  if (rc) return rc;
  out2[0] = w[1]; out2[1] = c->mb.nq;
  return SVNICP_OK;
}

// ---- Gaussian pose prior on the correction ----
int svnicp_set_pose_prior(svnicp_ctx* c, const double mean6[6], const double info36[36]) {
  CTX_CHECK(c);
  if (!info36) { c->pr.set = false; return SVNICP_OK; }
  if (!mean6) return fail(c, SVNICP_ERR_INVALID, "svnicp_set_pose_prior: null mean");
  PosePrior next;
  const char* why = nullptr;
  if (pose_prior::validate(mean6, info36, &next, &why)) return fail(c, SVNICP_ERR_INVALID, std::string("svnicp_set_pose_prior: ") + why);
  c->pr.next = next; c->pr.set = true;
  std::memcpy(c->pr.mean6, mean6, sizeof c->pr.mean6);
  std::memcpy(c->pr.info36, next.L, sizeof c->pr.info36);
  c->run.have_candidates = false;   // the step chain follows the prior: svnicp_iter_accumulate refuses until the next svnicp_align_begin
  return SVNICP_OK;
}
int svnicp_get_pose_prior(svnicp_ctx* c, int* on, double mean6[6], double info36[36]) {
  CTX_CHECK(c);
  if (on) *on = c->pr.set ? 1 : 0;
  if (c->pr.set && mean6) std::memcpy(mean6, c->pr.mean6, sizeof c->pr.mean6);
  if (c->pr.set && info36) std::memcpy(info36, c->pr.info36, sizeof c->pr.info36);
  return SVNICP_OK;
}

// ---- point-to-plane residual ----
int svnicp_set_residual(svnicp_ctx* c, int residual, double huber_delta, int normal_k) {
  CTX_CHECK(c);
  if (residual != SVNICP_RESIDUAL_POINT && residual != SVNICP_RESIDUAL_PLANE) return fail(c, SVNICP_ERR_INVALID, "svnicp_set_residual: unknown residual");
  if (!(huber_delta > 0.0)) return fail(c, SVNICP_ERR_INVALID, "svnicp_set_residual: huber_delta must be positive (+inf: no down-weighting)");
  if (normal_k != 0 && (normal_k < 4 || normal_k > 64)) return fail(c, SVNICP_ERR_INVALID, "svnicp_set_residual: normal_k must be 0 (= 16) or in 4..64");
  c->pl.residual = residual; c->pl.delta = huber_delta; c->pl.normal_k = normal_k ? normal_k : 16;
  c->run.have_candidates = false;   // the stage-B plan follows the residual: svnicp_iter_accumulate refuses until the next svnicp_align_begin
  return SVNICP_OK;
}

int svnicp_set_target_normals(svnicp_ctx* c, const double* n_xyz, int64_t M, int mem_kind) {
  CTX_CHECK(c);
  if (!n_xyz) return fail(c, SVNICP_ERR_INVALID, "svnicp_set_target_normals: null argument");
  if (!c->cloud.tgt_set || M != c->M)
    return fail(c, SVNICP_ERR_INVALID, "svnicp_set_target_normals: must follow the svnicp_set_target it belongs to, with the same point count");
  if (bind(c)) return SVNICP_ERR_HIP;
  HIPCHK(c, c->pl.nsup.ensure((size_t)M * 3));
  HIPCHK(c, c->pl.rec.ensure((size_t)M * 6));
  HIPCHK(c, hipMemcpyAsync(c->pl.nsup.p, n_xyz, (size_t)M * 24, mem_kind == SVNICP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, launch_pack_normals(c->cloud.tgt.p, c->pl.nsup.p, M, c->pl.rec.p, c->stream));
  if (mem_kind != SVNICP_MEM_DEVICE) HIPCHK(c, hipStreamSynchronize(c->stream));  // caller may reuse its host buffer
  c->pl.supplied = true; c->pl.estimated = false;
  c->ev.mark_stale("the target normals changed since the last svnicp_evaluate");
  return SVNICP_OK;
}

int svnicp_get_target_normals(svnicp_ctx* c, double* outMx3) {
  CTX_CHECK(c);
  if (!outMx3) return fail(c, SVNICP_ERR_INVALID, "svnicp_get_target_normals: null argument");
  if (!c->pl.supplied && !c->pl.estimated) return fail(c, SVNICP_ERR_INVALID, "svnicp_get_target_normals: no normals supplied or estimated for this target yet");
  std::vector<double> rec((size_t)c->M * 6);
  if (const int rc = fetch(c, rec.data(), c->pl.rec.p, rec.size() * 8)) return rc;
  for (int64_t i = 0; i < c->M; ++i)
    for (int d = 0; d < 3; ++d) outMx3[3 * i + d] = rec[6 * i + 3 + d];
  return SVNICP_OK;
}

int svnicp_get_plane_stats(svnicp_ctx* c, double* outPx2, int64_t* normal_passes) {
  CTX_CHECK(c);
  if (normal_passes) *normal_passes = c->pl.passes;
  if (!outPx2) return SVNICP_OK;
  if (!c->run.have_result || !c->pl.on) return fail(c, SVNICP_ERR_INVALID, "svnicp_get_plane_stats: no registration with the point-to-plane residual yet");
  return fetch(c, outPx2, c->pl.stats.p, (size_t)c->P * 16);
}

// ---- generalized-ICP residual ----
int svnicp_set_residual_gicp(svnicp_ctx* c, double huber_delta, int normal_k, double epsilon) {
  CTX_CHECK(c);
  if (!(huber_delta > 0.0)) return fail(c, SVNICP_ERR_INVALID, "svnicp_set_residual_gicp: huber_delta must be positive (+inf: no down-weighting)");
  if (normal_k != 0 && (normal_k < 4 || normal_k > 64)) return fail(c, SVNICP_ERR_INVALID, "svnicp_set_residual_gicp: normal_k must be 0 (= 16) or in 4..64");
  if (epsilon != 0.0 && !(epsilon >= kGicpEpsilonMin && epsilon <= 1.0))
    return fail(c, SVNICP_ERR_INVALID, "svnicp_set_residual_gicp: epsilon must be 0 (= 1e-3) or in [1e-6, 1]");
  c->pl.residual = SVNICP_RESIDUAL_GICP; c->pl.delta = huber_delta; c->pl.normal_k = normal_k ? normal_k : 16;
  c->gi.eps = epsilon != 0.0 ? epsilon : kGicpEpsilonDefault;
  c->run.have_candidates = false;   // the stage-B plan follows the residual: svnicp_iter_accumulate refuses until the next svnicp_align_begin
  return SVNICP_OK;
}

int svnicp_set_source_normals(svnicp_ctx* c, const double* n_xyz, int64_t B, int mem_kind) {
  CTX_CHECK(c);
  if (!n_xyz) return fail(c, SVNICP_ERR_INVALID, "svnicp_set_source_normals: null argument");
  if (!c->cloud.src_set || B != c->B)
    return fail(c, SVNICP_ERR_INVALID, "svnicp_set_source_normals: must follow the svnicp_set_source it belongs to, with the same point count");
  if (bind(c)) return SVNICP_ERR_HIP;
  HIPCHK(c, c->gi.nsup.ensure((size_t)B * 3));
  HIPCHK(c, c->gi.rec.ensure((size_t)B * 6));
  HIPCHK(c, hipMemcpyAsync(c->gi.nsup.p, n_xyz, (size_t)B * 24, mem_kind == SVNICP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, launch_pack_normals(c->cloud.src.p, c->gi.nsup.p, B, c->gi.rec.p, c->stream));
  if (mem_kind != SVNICP_MEM_DEVICE) HIPCHK(c, hipStreamSynchronize(c->stream));  // caller may reuse its host buffer
  c->gi.supplied = true; c->gi.estimated = false;
  return SVNICP_OK;
}

int svnicp_get_source_normals(svnicp_ctx* c, double* outBx3) {
  CTX_CHECK(c);
  if (!outBx3) return fail(c, SVNICP_ERR_INVALID, "svnicp_get_source_normals: null argument");
  if (!c->gi.supplied && !c->gi.estimated) return fail(c, SVNICP_ERR_INVALID, "svnicp_get_source_normals: no normals supplied or estimated for this source yet");
  std::vector<double> rec((size_t)c->B * 6);
  if (const int rc = fetch(c, rec.data(), c->gi.rec.p, rec.size() * 8)) return rc;
  for (int64_t i = 0; i < c->B; ++i)
    for (int d = 0; d < 3; ++d) outBx3[3 * i + d] = rec[6 * i + 3 + d];
  return SVNICP_OK;
}

int svnicp_get_gicp_stats(svnicp_ctx* c, double* outPx2, int64_t passes2[2]) {
  CTX_CHECK(c);
  if (passes2) { passes2[0] = c->pl.passes; passes2[1] = c->gi.passes; }
  if (!outPx2) return SVNICP_OK;
  if (!c->run.have_result || !c->gi.on) return fail(c, SVNICP_ERR_INVALID, "svnicp_get_gicp_stats: no registration with the generalized-ICP residual yet");
  return fetch(c, outPx2, c->pl.stats.p, (size_t)c->P * 16);
}

// ---- evaluate a registration ----
// Rot3::Expmap as both pipelines' correction_to_pose states it (pipeline.py / registration_pipeline.hpp: so3_exp)
static void host_so3_exp(const double w[3], double R[9]) {
  const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  double K2[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) K2[3 * i + j] = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
  const double a = th < 1e-10 ? 1.0 : std::sin(th) / th, b = th < 1e-10 ? 0.5 : (1.0 - std::cos(th)) / (th * th);
  for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * K[i] + b * K2[i];
}

// T0 * Pose3(Rot3::Expmap(x[3:6]), x[0:3]): the total pose of a correction 6-vector -- the global mean (svnicp_evaluate with
// a NULL pose) or a mode's mean (svnicp_particle_modes)
static void correction_total_pose(const Pose0& pose0, const double x[6], EvalPose& T) {
  double Rc[9];
  host_so3_exp(x + 3, Rc);
  const double* R0 = pose0.R0;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T.R[3 * i + j] = R0[3 * i] * Rc[j] + R0[3 * i + 1] * Rc[3 + j] + R0[3 * i + 2] * Rc[6 + j];
    T.t[i] = (R0[3 * i] * x[0] + R0[3 * i + 1] * x[1] + R0[3 * i + 2] * x[2]) + pose0.t0[i];
  }
}

int svnicp_evaluate(svnicp_ctx* c, const double* R, const double* t, double max_corr_dist, svnicp_eval* out) {
  CTX_CHECK(c);
  if (!out) return fail(c, SVNICP_ERR_INVALID, "svnicp_evaluate: null result struct");
  if (out->struct_size != (int32_t)sizeof(svnicp_eval)) return fail(c, SVNICP_ERR_INVALID, "svnicp_evaluate: svnicp_eval.struct_size mismatch");
  if (!(max_corr_dist > 0.0)) return fail(c, SVNICP_ERR_INVALID, "svnicp_evaluate: max_corr_dist must be positive and not NaN (+inf: every evaluated row with a finite distance is an inlier)");
  if ((R == nullptr) != (t == nullptr)) return fail(c, SVNICP_ERR_INVALID, "svnicp_evaluate: R and t must both be given, or both be NULL (the last registration's result)");
  if (R) {
    bool finite = true;
    for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(R[i]);
    for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(t[i]);
    if (!finite) return fail(c, SVNICP_ERR_INVALID, "svnicp_evaluate: the pose holds a non-finite entry");
  }
  if (!c->run.have_result)
    return fail(c, SVNICP_ERR_INVALID, "svnicp_evaluate: no finished registration yet (stage A's target layout and scratch belong to one)");
  if (!c->run.have_candidates)
    return fail(c, SVNICP_ERR_INVALID, "svnicp_evaluate: the source, the target, the initial mean, K or an option changed since the last registration: "
                                       "register again first (stage A's target layout and scratch belong to that registration)");
  if (!c->sa.plan.can_search(1))
    return fail(c, SVNICP_ERR_INVALID, "svnicp_evaluate: the seeded-scan stage A (option knn=v2, or a target beyond the tile kernel's range) is built "
                                       "for knn_count neighbours and cannot search with K = 1");
  if (const int rc = svnicp_synchronize(c)) return rc;   // an asynchronous registration has finished and its checks have run
  EvalPose T{};
  if (R) {
    std::memcpy(T.R, R, sizeof T.R); std::memcpy(T.t, t, sizeof T.t);
  } else {   // T0 * Pose3(Rot3::Expmap(mean[3:6]), mean[0:3])
    double mean[6];
    if (const int rc = fetch_stats(c, mean, 0, 6)) return rc;
    correction_total_pose(c->pose0, mean, T);
    for (int i = 0; i < 12; ++i)
      if (!std::isfinite(i < 9 ? T.R[i] : T.t[i - 9])) return fail(c, SVNICP_ERR_INVALID, "svnicp_evaluate: the last registration's result pose is not finite");
  }
  const int64_t B = c->B, M = c->M, nblk = evaluate_blocks(B);
  EvalState& ev = c->ev;
  ev.have = false; ev.fresh = false; ev.stale = "the last svnicp_evaluate did not finish";
  HIPCHK(c, ev.q.ensure((size_t)B * 3)); HIPCHK(c, ev.idx.ensure((size_t)B)); HIPCHK(c, ev.d2.ensure((size_t)B));
  HIPCHK(c, ev.partial.ensure((size_t)nblk * kEvalRecord)); HIPCHK(c, ev.result.ensure(kEvalResult));
  if (!ev.h_result.p) HIPCHK(c, ev.h_result.alloc(kEvalResult));
  HIPCHK(c, launch_evaluate_transform(c->cloud.src.p, B, T, ev.q.p, c->stream));
  // stage A's own search, K = 1, identity pose, in blocks of the rows its scratch is sized for (a mini-batch registration
  // sizes it for fewer than B); no survivor counts: svnicp_get_knn_survivors keeps the registration's
  const StageAEnv env{c->stream, c->tune, c->num_cus, false, c->cloud.tgt.p, c->B, c->M, c->pose0};
  if (!c->sa.stage_kept)
    if (const int rc = c->sa.keep_stage_fallbacks(c, env)) return rc;
  if (const int rc = c->sa.search_blocks(c, env, ev.q.p, B, 1, ev.idx.p, ev.d2.p, 1)) return rc;
  const bool normals = c->pl.supplied || c->pl.estimated;
  EvalArgs a{};
  a.q = ev.q.p; a.tgt = c->cloud.tgt.p; a.rec = normals ? c->pl.rec.p : nullptr; a.B = B; a.M = M;
  a.thr2 = max_corr_dist * max_corr_dist; a.idx = ev.idx.p; a.d2 = ev.d2.p; a.partial = ev.partial.p;
  HIPCHK(c, launch_evaluate_pairs(a, ev.result.p, c->stream));
  HIPCHK(c, hipMemcpyAsync(ev.h_result.p, ev.result.p, kEvalResult * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const double* r = ev.h_result.p;
  out->has_normals = normals ? 1 : 0;
  out->rows = B;
  out->evaluated = (int64_t)r[0]; out->inliers = (int64_t)r[1]; out->plane_inliers = (int64_t)r[2];
  out->sum_d2 = r[3]; out->sum_r2 = r[4]; out->fitness = r[5]; out->inlier_rmse = r[6]; out->plane_rmse = r[7];
  std::memcpy(out->R, T.R, sizeof T.R); std::memcpy(out->t, T.t, sizeof T.t);
  ev.have = true; ev.rows = B;
  ev.fresh = true; ev.normals = normals; ev.max_corr_dist = max_corr_dist; ev.T = T;
  return SVNICP_OK;
}

const int32_t* svnicp_eval_index_devptr(svnicp_ctx* c) { return (c && c->ev.have) ? c->ev.idx.p : nullptr; }
const double* svnicp_eval_dist2_devptr(svnicp_ctx* c) { return (c && c->ev.have) ? c->ev.d2.p : nullptr; }

int svnicp_get_eval_pairs(svnicp_ctx* c, int32_t* idxB, double* d2B) {
  CTX_CHECK(c);
  if (!c->ev.have) return fail(c, SVNICP_ERR_INVALID, "svnicp_get_eval_pairs: no svnicp_evaluate yet");
  if (idxB)
    if (const int rc = fetch(c, idxB, c->ev.idx.p, (size_t)c->ev.rows * 4)) return rc;
  if (d2B)
    if (const int rc = fetch(c, d2B, c->ev.d2.p, (size_t)c->ev.rows * 8)) return rc;
  return SVNICP_OK;
}

// ---- information matrix of a registration ----
int svnicp_information_solve(svnicp_information* io) { return svnicp_info::solve(io, nullptr); }

// What the two entry points share once the form is known: the remaining argument checks, the freshness of the last evaluate,
// the two launches, the copy and the host solve.  fn names the entry point in every refusal; eps is read by the GICP form only.
static int information_of_last_evaluate(svnicp_ctx* c, const char* fn, int form, double huber_delta, double eps, double eig_floor_ratio,
                                        svnicp_information* out) {
  const std::string who = std::string(fn) + ": ";
  if (!(huber_delta > 0.0)) return fail(c, SVNICP_ERR_INVALID, who + "huber_delta must be positive and not NaN (+inf: unweighted)");
  if (!(eig_floor_ratio >= 0.0 && eig_floor_ratio < 1.0)) return fail(c, SVNICP_ERR_INVALID, who + "eig_floor_ratio must lie in [0, 1) (0: the default, 1e-12)");
  EvalState& ev = c->ev;
  if (!ev.fresh || !ev.have || ev.rows != c->B)
    return fail(c, SVNICP_ERR_INVALID, who + ev.stale + ": call svnicp_evaluate first (the sums run over its rows; it "
                                       "must have succeeded since the source, the target or the target normals last changed and since the last registration began)");
  if (form == SVNICP_INFO_PLANE && !ev.normals)
    return fail(c, SVNICP_ERR_INVALID, who + "the plane form needs target normals, and the last svnicp_evaluate had has_normals = 0");
  const bool gicp = form == SVNICP_INFO_GICP;
  if (gicp && !ev.normals)
    return fail(c, SVNICP_ERR_INVALID, who + "the GICP form needs target normals, and the last svnicp_evaluate had has_normals = 0");
  if (gicp && !c->gi.supplied && !c->gi.estimated)
    return fail(c, SVNICP_ERR_INVALID, who + "the context holds no normals of the current source (svnicp_set_source_normals, or a registration in "
                                             "generalized-ICP mode that estimated them)");
  if (bind(c)) return SVNICP_ERR_HIP;
  const int64_t B = c->B, nblk = evaluate_blocks(B);
  HIPCHK(c, ev.info_partial.ensure((size_t)nblk * kInfoPlaneRecord)); HIPCHK(c, ev.info_result.ensure(kInfoResult));
  if (!ev.h_info.p) HIPCHK(c, ev.h_info.alloc(kInfoResult));
  InfoArgs a{};
  a.src = c->cloud.src.p; a.q = ev.q.p; a.tgt = c->cloud.tgt.p; a.rec = ev.normals ? c->pl.rec.p : nullptr; a.idx = ev.idx.p; a.d2 = ev.d2.p;
  a.B = B; a.M = c->M; a.thr2 = ev.max_corr_dist * ev.max_corr_dist; a.delta = huber_delta; a.T = ev.T; a.partial = ev.info_partial.p;
  a.srec = gicp ? c->gi.rec.p : nullptr; a.eps = eps;
  HIPCHK(c, launch_information(gicp ? 2 : form, a, ev.info_result.p, c->stream));
  HIPCHK(c, hipMemcpyAsync(ev.h_info.p, ev.info_result.p, kInfoResult * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const double* r = ev.h_info.p;
  svnicp_information o{};
  o.struct_size = (int32_t)sizeof o; o.form = form;
  o.huber_delta = huber_delta; o.eig_floor_ratio = eig_floor_ratio; o.max_corr_dist = ev.max_corr_dist;
  std::memcpy(o.H, r, sizeof o.H); std::memcpy(o.b, r + 36, sizeof o.b);
  o.pairs = (int64_t)r[42]; o.sum_w = r[43]; o.sum_wr2 = r[44];
  std::memcpy(o.R, ev.T.R, sizeof o.R); std::memcpy(o.t, ev.T.t, sizeof o.t);
  const char* why = nullptr;
  if (const int rc = svnicp_info::solve(&o, &why)) return fail(c, rc, who + (why ? why : "svnicp_information_solve failed"));
  *out = o;
  return SVNICP_OK;
}

int svnicp_eval_information(svnicp_ctx* c, int form, double huber_delta, double eig_floor_ratio, svnicp_information* out) {
  CTX_CHECK(c);
  if (!out) return fail(c, SVNICP_ERR_INVALID, "svnicp_eval_information: null result struct");
  if (out->struct_size != (int32_t)sizeof(svnicp_information)) return fail(c, SVNICP_ERR_INVALID, "svnicp_eval_information: svnicp_information.struct_size mismatch");
  if (form != SVNICP_INFO_POINT && form != SVNICP_INFO_PLANE)
    return fail(c, SVNICP_ERR_INVALID, "svnicp_eval_information: unknown form (SVNICP_INFO_POINT or SVNICP_INFO_PLANE; the GICP form is svnicp_eval_information_gicp)");
  return information_of_last_evaluate(c, "svnicp_eval_information", form, huber_delta, 0.0, eig_floor_ratio, out);
}

int svnicp_eval_information_gicp(svnicp_ctx* c, double huber_delta, double epsilon, double eig_floor_ratio, svnicp_information* out) {
  CTX_CHECK(c);
  if (!out) return fail(c, SVNICP_ERR_INVALID, "svnicp_eval_information_gicp: null result struct");
  if (out->struct_size != (int32_t)sizeof(svnicp_information)) return fail(c, SVNICP_ERR_INVALID, "svnicp_eval_information_gicp: svnicp_information.struct_size mismatch");
  if (epsilon != 0.0 && !(epsilon >= kGicpEpsilonMin && epsilon <= 1.0))   // svnicp_set_residual_gicp's rule
    return fail(c, SVNICP_ERR_INVALID, "svnicp_eval_information_gicp: epsilon must be 0 (= 1e-3) or in [1e-6, 1]");
  return information_of_last_evaluate(c, "svnicp_eval_information_gicp", SVNICP_INFO_GICP, huber_delta, epsilon != 0.0 ? epsilon : kGicpEpsilonDefault,
                                      eig_floor_ratio, out);
}

// ---- score and weight the particles ----
int svnicp_get_particle_scores(svnicp_ctx* c, double* outPx6, double* posesPx12) {
  CTX_CHECK(c);
  if (!c->sc.have) return fail(c, SVNICP_ERR_INVALID, "svnicp_get_particle_scores: no scoring yet (svnicp_score_particles, or a registration with svnicp_set_particle_weighting)");
  if (outPx6)
    if (const int rc = fetch(c, outPx6, c->sc.scores.p, (size_t)c->sc.P * kScoreFields * sizeof(double))) return rc;
  if (posesPx12)
    if (const int rc = fetch(c, posesPx12, c->sc.poses.p, (size_t)c->sc.P * 12 * sizeof(double))) return rc;
  return SVNICP_OK;
}

int svnicp_score_particles(svnicp_ctx* c, double max_corr_dist, double* outPx6, double* posesPx12) {
  CTX_CHECK(c);
  if (!(max_corr_dist > 0.0) || !std::isfinite(max_corr_dist))
    return fail(c, SVNICP_ERR_INVALID, "svnicp_score_particles: max_corr_dist must be finite and positive");
  if (!c->run.have_result)
    return fail(c, SVNICP_ERR_INVALID, "svnicp_score_particles: no finished registration yet (the candidate table belongs to one)");
  if (!c->run.have_candidates)
    return fail(c, SVNICP_ERR_INVALID, "svnicp_score_particles: the source, the target, the initial mean, K or an option changed since the last registration: "
                                       "register again first (the candidate table belongs to that registration)");
  if (c->sc.reg_refusal) return fail(c, SVNICP_ERR_INVALID, std::string(kScoringRefusal) + c->sc.reg_refusal);
  if (const int rc = svnicp_synchronize(c)) return rc;   // an asynchronous registration has finished and its checks have run
  if (bind(c)) return SVNICP_ERR_HIP;
  ScoreObjective point;
  point.gate = max_corr_dist;
  if (const int rc = enqueue_scoring(c, point)) return rc;
  if (!outPx6 && !posesPx12) { HIPCHK(c, hipStreamSynchronize(c->stream)); return SVNICP_OK; }
  return svnicp_get_particle_scores(c, outPx6, posesPx12);
}

int svnicp_set_particle_weighting(svnicp_ctx* c, int kind, double max_corr_dist, double temperature) {
  CTX_CHECK(c);
  if (kind != SVNICP_WEIGHT_UNIFORM) {
    if (!(max_corr_dist > 0.0) || !std::isfinite(max_corr_dist))
      return fail(c, SVNICP_ERR_INVALID, "svnicp_set_particle_weighting: max_corr_dist must be finite and positive");
    if (!(temperature > 0.0) || !std::isfinite(temperature))
      return fail(c, SVNICP_ERR_INVALID, "svnicp_set_particle_weighting: temperature must be finite and positive");
  }
  c->sc.kind = kind;   // an unknown kind is refused by svnicp_align_begin
  c->sc.cfg = ScoreObjective{}; c->sc.cfg.gate = max_corr_dist;   // the point cost (back, after svnicp_set_particle_weighting_objective)
  c->sc.temperature = temperature;
  return SVNICP_OK;
}

// ---- … in the objective the solver minimised ----
// the caller's struct as the rules of registration_plan.hpp take it; nullptr: nothing was refused
static const char* read_score_objective(const svnicp_score_objective* obj, ScoreObjective& o) {
  if (!obj) return "null svnicp_score_objective";
  if (obj->struct_size != sizeof(svnicp_score_objective)) return "svnicp_score_objective.struct_size mismatch";
  o.form = obj->form; o.gate = obj->max_corr_dist; o.delta = obj->huber_delta; o.eps = obj->epsilon;
  return score_objective_refusal(o, kGicpEpsilonMin);
}

int svnicp_score_particles_objective(svnicp_ctx* c, const svnicp_score_objective* obj, double* outPx6, double* posesPx12) {
  CTX_CHECK(c);
  ScoreObjective o;
  if (const char* why = read_score_objective(obj, o)) return fail(c, SVNICP_ERR_INVALID, std::string("svnicp_score_particles_objective: ") + why);
  if (!c->run.have_result)
    return fail(c, SVNICP_ERR_INVALID, "svnicp_score_particles_objective: no finished registration yet (the candidate table belongs to one)");
  if (!c->run.have_candidates)
    return fail(c, SVNICP_ERR_INVALID, "svnicp_score_particles_objective: the source, the target, the initial mean, K or an option changed since the last registration: "
                                       "register again first (the candidate table belongs to that registration)");
  if (c->sc.reg_refusal) return fail(c, SVNICP_ERR_INVALID, std::string(kScoringRefusal) + c->sc.reg_refusal);
  o = resolve_score_objective(o, c->pl.on, c->gi.on, c->pl.delta, c->gi.eps);
  if (const int rc = svnicp_synchronize(c)) return rc;   // an asynchronous registration has finished and its checks have run
  if (bind(c)) return SVNICP_ERR_HIP;
  if (const int rc = enqueue_scoring(c, o)) return rc;
  if (!outPx6 && !posesPx12) { HIPCHK(c, hipStreamSynchronize(c->stream)); return SVNICP_OK; }
  return svnicp_get_particle_scores(c, outPx6, posesPx12);
}

int svnicp_set_particle_weighting_objective(svnicp_ctx* c, int kind, const svnicp_score_objective* obj, double temperature) {
  CTX_CHECK(c);
  ScoreObjective o;
  if (kind != SVNICP_WEIGHT_UNIFORM) {
    if (const char* why = read_score_objective(obj, o)) return fail(c, SVNICP_ERR_INVALID, std::string("svnicp_set_particle_weighting_objective: ") + why);
    if (!(temperature > 0.0) || !std::isfinite(temperature))
      return fail(c, SVNICP_ERR_INVALID, "svnicp_set_particle_weighting_objective: temperature must be finite and positive");
  }
  c->sc.kind = kind;   // an unknown kind is refused by svnicp_align_begin
  c->sc.cfg = o; c->sc.temperature = temperature;
  return SVNICP_OK;
}

int svnicp_get_score_objective(svnicp_ctx* c, svnicp_score_objective* out) {
  CTX_CHECK(c);
  if (!out) return fail(c, SVNICP_ERR_INVALID, "svnicp_get_score_objective: null result struct");
  if (!c->sc.have) return fail(c, SVNICP_ERR_INVALID, "svnicp_get_score_objective: no scoring yet (svnicp_score_particles, svnicp_score_particles_objective, or a weighted registration)");
  const ScoreObjective& o = c->sc.last;
  out->struct_size = sizeof(svnicp_score_objective);
  out->form = o.form; out->max_corr_dist = o.gate; out->huber_delta = o.delta; out->epsilon = o.eps;
  return SVNICP_OK;
}

// ---- particle modes ----
int svnicp_particle_modes(svnicp_ctx* c, const svnicp_modes_opt* opt, svnicp_modes* out) {
  CTX_CHECK(c);
  if (!opt || !out) return fail(c, SVNICP_ERR_INVALID, "svnicp_particle_modes: null options or result struct");
  if (opt->struct_size != (int32_t)sizeof(svnicp_modes_opt)) return fail(c, SVNICP_ERR_INVALID, "svnicp_particle_modes: svnicp_modes_opt.struct_size mismatch");
  if (out->struct_size != (int32_t)sizeof(svnicp_modes)) return fail(c, SVNICP_ERR_INVALID, "svnicp_particle_modes: svnicp_modes.struct_size mismatch");
  if (opt->max_modes < 1 || opt->max_modes > SVNICP_MODES_MAX) return fail(c, SVNICP_ERR_INVALID, "svnicp_particle_modes: max_modes must lie in 1..SVNICP_MODES_MAX");
  if (!(opt->link_trans >= 0.0) || !std::isfinite(opt->link_trans) || !(opt->link_rot >= 0.0) || !std::isfinite(opt->link_rot))
    return fail(c, SVNICP_ERR_INVALID, "svnicp_particle_modes: link_trans and link_rot must be finite and not negative");
  const bool own = opt->particles6xP != nullptr;
  if (!own && opt->weightsP) return fail(c, SVNICP_ERR_INVALID, "svnicp_particle_modes: weightsP without particles6xP (the registration's set carries its own weights)");
  if (own && opt->P < 1) return fail(c, SVNICP_ERR_INVALID, "svnicp_particle_modes: need P >= 1");
  if (!own && !c->run.have_result)
    return fail(c, SVNICP_ERR_INVALID, "svnicp_particle_modes: no finished registration yet (pass particles6xP to cluster a set of your own)");
  const int P = own ? opt->P : c->P;
  if (P > kModesMaxP) return fail(c, SVNICP_ERR_INVALID, "svnicp_particle_modes: more than 2048 particles (one workgroup stages the set in LDS)");
  if (own && opt->weightsP)
    for (int p = 0; p < P; ++p)
      if (!(opt->weightsP[p] >= 0.0) || !std::isfinite(opt->weightsP[p]))
        return fail(c, SVNICP_ERR_INVALID, "svnicp_particle_modes: a supplied weight is negative or not finite");
  if (const int rc = svnicp_synchronize(c)) return rc;   // an asynchronous registration has finished and its checks have run
  ModesState& md = c->md;
  md.have = false;
  const size_t res_doubles = (modes_result_bytes(P) + 7) / 8;
  HIPCHK(c, md.result.ensure(res_doubles));
  if (md.h_result.cap < res_doubles) HIPCHK(c, md.h_result.alloc(res_doubles));
  ModesArgs a{};
  a.P = P; a.max_modes = opt->max_modes;
  a.lt2 = opt->link_trans * opt->link_trans; a.lr2 = opt->link_rot * opt->link_rot;
  a.result = md.result.p;
  bool scores = false;
  if (own) {   // the stream is idle and stays so until this call returns: one pinned block carries the set up
    const size_t n_in = (size_t)P * (opt->weightsP ? 7 : 6);
    HIPCHK(c, md.in_pose.ensure((size_t)P * 6));
    if (md.h_in.cap < n_in) HIPCHK(c, md.h_in.alloc(n_in));
    std::memcpy(md.h_in.p, opt->particles6xP, (size_t)P * 48);
    HIPCHK(c, hipMemcpyAsync(md.in_pose.p, md.h_in.p, (size_t)P * 48, hipMemcpyHostToDevice, c->stream));
    a.pose = md.in_pose.p;
    if (opt->weightsP) {
      HIPCHK(c, md.in_w.ensure((size_t)P));
      std::memcpy(md.h_in.p + (size_t)P * 6, opt->weightsP, (size_t)P * 8);
      HIPCHK(c, hipMemcpyAsync(md.in_w.p, md.h_in.p + (size_t)P * 6, (size_t)P * 8, hipMemcpyHostToDevice, c->stream));
      a.w = md.in_w.p;
    }
  } else {
    a.pose = c->st.pose_out.p;
    a.w = c->st.stats.p + 48;   // what svnicp_get_particle_weight returns
    scores = c->sc.have && c->sc.of_result && c->sc.P == P;
    if (scores) a.scores = c->sc.scores.p;
  }
  HIPCHK(c, launch_particle_modes(a, c->stream));
  HIPCHK(c, hipMemcpyAsync(md.h_result.p, md.result.p, modes_result_bytes(P), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const double* r = md.h_result.p;
  svnicp_modes o{};
  o.struct_size = (int32_t)sizeof o;
  o.particles = (int32_t)r[0]; o.nonfinite = (int32_t)r[1]; o.n_modes = (int32_t)r[2]; o.n_reported = (int32_t)r[3];
  o.has_scores = scores ? 1 : 0;
  for (int k = 0; k < SVNICP_MODES_MAX; ++k) {
    const double* rec = r + kModesHeader + (size_t)k * kModesRecord;
    o.label[k] = (int32_t)rec[0]; o.count[k] = (int32_t)rec[1]; o.best[k] = (int32_t)rec[2];
    o.mass[k] = rec[3]; o.cost_min[k] = rec[4]; o.cost_mean[k] = rec[5];
    std::memcpy(o.mean[k], rec + 6, sizeof o.mean[k]); std::memcpy(o.cov[k], rec + 12, sizeof o.cov[k]);
    if (k < o.n_reported) {
      EvalPose T{};
      correction_total_pose(c->pose0, o.mean[k], T);
      std::memcpy(o.R[k], T.R, sizeof T.R); std::memcpy(o.t[k], T.t, sizeof T.t);
    }
  }
  *out = o;
  md.have = true; md.P = P;
  return SVNICP_OK;
}

int svnicp_get_mode_labels(svnicp_ctx* c, int32_t* outP) {
  CTX_CHECK(c);
  if (!outP) return fail(c, SVNICP_ERR_INVALID, "svnicp_get_mode_labels: null output");
  if (!c->md.have) return fail(c, SVNICP_ERR_INVALID, "svnicp_get_mode_labels: no svnicp_particle_modes yet");
  std::memcpy(outP, c->md.h_result.p + kModesResult, (size_t)c->md.P * sizeof(int32_t));
  return SVNICP_OK;
}

int svnicp_get_trace(svnicp_ctx* c, int32_t* corr, double* H, double* b, double* N, double* phi, double* h) {
  NEED_RESULT(c);
  if (!c->prm.record_trace) return fail(c, SVNICP_ERR_INVALID, "svnicp_get_trace: params.record_trace was 0");
  const size_t I = (size_t)c->prm.iterations, P = (size_t)c->P;
  int rc = 0;
  if (corr && (rc = fetch(c, corr, c->tr.corr.p, I * P * (size_t)(c->mb.on ? c->mb.batch : c->B) * 4))) return rc;
  if (H && (rc = fetch(c, H, c->tr.H.p, I * P * 36 * 8))) return rc;
  if (b && (rc = fetch(c, b, c->tr.b.p, I * P * 6 * 8))) return rc;
  if (N && (rc = fetch(c, N, c->tr.N.p, I * P * 6 * 8))) return rc;
  if (phi && (rc = fetch(c, phi, c->tr.phi.p, I * P * 6 * 8))) return rc;
  if (h && (rc = fetch(c, h, c->tr.h.p, I * 8))) return rc;
  return SVNICP_OK;
}

}  // extern "C"
