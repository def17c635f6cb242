/*
 * svnicp_hip.h — C ABI of libsvnicp_hip.so: MI355X (gfx950) Stein-variational ICP registration.
 *
 * This is the drop-in boundary for the reference's solver classes svnicp::SVGDICP (virtual) /
 * svnicp::SVNICP (final).  The reference has no FFI: its only caller hands libtorch tensors on
 * kCUDA and one gtsam::Pose3 to those classes (svn-icp/src/core/OdometryPipeline.cpp:282-288,
 * 573-607, 1021).  Every entry point below names the reference interface it replaces
 * (file:line relative to /root/reference/svn-icp/).  Plain pointers and sizes only; no torch,
 * no C++ types.  All floating point is float64 (reference: include/core/SVGDICP.h:207), row-major.
 *
 * Threading: like the reference (one steinicp_thread_, OdometryPipeline.cpp:106-110) a context
 * is used by one host thread at a time; calls are sequential per scan.  Ownership: the context
 * owns all device memory; the caller owns every host buffer it passes in or out.
 *
 * Return convention: 0 (or a SteinICPState for svnicp_align) on success, a negative
 * svnicp_status on failure; nothing throws across this ABI.  svnicp_last_error() gives text.
 */
#ifndef SVNICP_HIP_H
#define SVNICP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVNICP_ABI_VERSION 1

typedef struct svnicp_ctx svnicp_ctx;

/* enum SteinICPState — include/core/SVGDICP.h:59-62 */
#define SVNICP_ALIGN_SUCCESS 1
#define SVNICP_NO_OPTIMIZER 2

typedef enum {
  SVNICP_OK = 0,
  SVNICP_ERR_INVALID = -1,   /* bad argument / call order            */
  SVNICP_ERR_HIP = -2,       /* a HIP runtime call failed             */
  SVNICP_ERR_NO_DEVICE = -3, /* no gfx950 device / code object        */
  SVNICP_ERR_NOMEM = -4
} svnicp_status;

/* class_type — OdometryPipeline.cpp:282-288 ("SVNICP" | "SVGDICP") */
#define SVNICP_MODE_SVN 0
#define SVNICP_MODE_SVGD 1

/* optimizer names of SVGDICP::set_optimizer — src/core/SVGDICP.cpp:142-170 */
#define SVNICP_OPT_ADAM 0
#define SVNICP_OPT_RMSPROP 1
#define SVNICP_OPT_SGD 2
#define SVNICP_OPT_ADAGRAD 3
#define SVNICP_OPT_NONE (-1)

#define SVNICP_MEM_HOST 0
#define SVNICP_MEM_DEVICE 1

/* svnicp::SteinICPParam — include/core/SVGDICP.h:41-57 (solver-relevant fields; normalize_cloud,
 * convergence_steps, cov_filter_type are ignored by the reference solver; use_minibatch / batch_size
 * are set through svnicp_set_minibatch, see "mini-batch" below) */
typedef struct svnicp_params {
  int32_t struct_size;           /* = sizeof(svnicp_params)                                   */
  int32_t mode;                  /* SVNICP_MODE_*                                              */
  int32_t iterations;            /* SteinICPParam::iterations                                  */
  int32_t knn_count;             /* SteinICPParam::KNN_count  (K_source_).  K <= 128: matrix-pipe
                                  * search and Morton-tile stage A (the tuned path); larger K runs
                                  * the LDS-tile kernels and is refused with SVNICP_ERR_INVALID in
                                  * svnicp_align / svnicp_align_begin once the smallest tile no longer
                                  * fits one CU's 160 KB of LDS (about K >= 330 for shards of <= 8
                                  * particles, K >= 620 otherwise) */
  double lr;                     /* SteinICPParam::lr                                          */
  double max_dist;               /* SteinICPParam::max_dist                                    */
  double convergence_threshold;  /* SteinICPParam::convergence_threshold                       */
  int32_t check_early_stop;      /* SteinICPParam::check_early_stop                            */
  int32_t svn_full_grad;         /* SteinICPParam::SVN_full_grad                               */
  int32_t optimizer;             /* SteinICPParam::optimizer as SVNICP_OPT_*                   */
  int32_t record_trace;          /* test hook: keep per-iteration H,b,N,phi,h,correspondences  */
} svnicp_params;

/* ctor svnicp::SVNICP(param, init_pose[6,P,1], opt) / svnicp::SVGDICP(param, init_pose)
 * — src/core/SVNICP.cpp:20-38, src/core/SVGDICP.cpp:22-44.  init_pose6xP may be NULL (then
 * svnicp_set_particles must be called before svnicp_align).  `device` is the HIP ordinal. */
int svnicp_create(const svnicp_params *params, int device, const double *init_pose6xP, int P,
                  svnicp_ctx **out);
void svnicp_destroy(svnicp_ctx *ctx);
const char *svnicp_last_error(const svnicp_ctx *ctx); /* ctx may be NULL: last create() error */
int svnicp_abi_version(void);

/* run on this hipStream_t instead of the context's private stream: lets a host that owns streams
 * (torch, a ROS executor) keep kernels, copies and collectives in ONE queue.  NULL is a valid
 * handle — HIP's default (null) stream, which is what torch.cuda.current_stream() usually is;
 * pass SVNICP_OWN_STREAM to return to the private stream. */
#define SVNICP_OWN_STREAM ((void *)(intptr_t)-1)
int svnicp_set_stream(svnicp_ctx *ctx, void *hip_stream);
int svnicp_synchronize(svnicp_ctx *ctx);

/* SVGDICP::add_cloud(source[B,3], target[M,3], init_pose[6,P,1]) — src/core/SVGDICP.cpp:46-62.
 * Split in two because the clouds and the particles are independent buffers; both are copied.  SVNICP_MEM_HOST: the
 * caller's buffer is free when the call returns.  SVNICP_MEM_DEVICE: the copy is QUEUED on the context's stream — the
 * device buffer must stay unchanged until svnicp_align has returned (or svnicp_synchronize).  svnicp_set_particles stages
 * the poses through pinned memory and does not wait for the stream either.
 *
 * Non-finite and huge points.  Clouds are taken as given (svnicp_set_clouds, svnicp_set_source, svnicp_set_target): a row
 * may hold NaN, +-inf or a finite junk coordinate such as 1e20 or 1e160 (the scan-prep, segmentation, deskew and map entry
 * points drop such rows; these three do not).  What they do, for every stage-A kernel and every launch chain:
 *   stage A      per query q = R0 s + t0 and target j: d2 = ((dx*dx) + dy*dy) + dz*dz in float64, unfused.  A target whose d2
 *                is NaN is never a neighbour; any other d2, +inf included, is a number; the neighbours are the K smallest by
 *                (d2, index); positions past the number of eligible targets hold index 0 and d2 = 0.0 (a NaN query: the
 *                whole row).  A row's result depends on that row and the target only.  This is the reference's
 *                knn_cpu.cpp except where a NaN distance is inserted while its heap is not yet full.
 *   search       per iteration, strict '<' from candidate 0: a NaN first distance is never replaced, an all-NaN row keeps
 *                candidate 0.
 *   point        the mask is a multiplication of the rows, as in the reference (SVGDICP.cpp:331-333): a pair whose source
 *   residual     row, transformed row or winner has a NaN or an infinite coordinate is 0 * that value = NaN, and the 22 sums
 *                of every particle it enters are NaN (the early-stop test then never fires: all `iterations` run).  A
 *                FINITE row whose d2 is huge or overflows to +inf is masked to exact zeros and still adds the identity
 *                block, like any rejected row.
 *   plane        a source row with a non-finite coordinate, a pair beyond max_dist and a winner without a normal are
 *   residual     rejected pairs and contribute exact zeros.  Estimated normals: a target point has no normal when the
 *                offset to one of its normal_k neighbours is NaN, infinite or too large for float32 to hold its square
 *                (|d| >= 2^64) -- a non-finite or huge point itself never has one.
 * A bad target row costs time, not correctness: its float32 image disables the pre-filters of the pruned kernels, and
 * more queries take their exact fallback. */
int svnicp_set_clouds(svnicp_ctx *ctx, const double *src_xyz, int64_t B, const double *tgt_xyz,
                      int64_t M, int mem_kind);
int svnicp_set_particles(svnicp_ctx *ctx, const double *init_pose6xP, int P);
/* the two halves of svnicp_set_clouds, for callers whose clouds live on different sides (host source scan, device
 * target from svnicp_map_query): each copies its cloud; both must have been given before svnicp_align */
int svnicp_set_source(svnicp_ctx *ctx, const double *src_xyz, int64_t B, int mem_kind);
int svnicp_set_target(svnicp_ctx *ctx, const double *tgt_xyz, int64_t M, int mem_kind);

/* SVGDICP::set_initial_mean(gtsam::Pose3) — include/core/SVGDICP.h:102-110.
 * R0 is the rotation matrix row-major (the reference's R0_ after its transpose), t0 the translation. */
int svnicp_set_initial_mean(svnicp_ctx *ctx, const double R0_rowmajor[9], const double t0[3]);
/* SVGDICP::set_k / set_threshold — include/core/SVGDICP.h:98,100 */
int svnicp_set_k(svnicp_ctx *ctx, int k);
int svnicp_set_max_dist(svnicp_ctx *ctx, double max_dist);

/* SVNICP::stein_align() / SVGDICP::stein_align() — src/core/SVNICP.cpp:41-114,
 * src/core/SVGDICP.cpp:66-140.  Synchronous.  Returns SVNICP_ALIGN_SUCCESS / SVNICP_NO_OPTIMIZER
 * or a negative svnicp_status. */
int svnicp_align(svnicp_ctx *ctx);
/* same work, enqueued only (no host sync): for benchmarking / pipelining; results are valid after
 * svnicp_synchronize().  With check_early_stop every iteration is enqueued (those behind the stop return at once on the
 * device); the blocking svnicp_align instead follows the device's stop flag and stops enqueuing a few iterations after it
 * (the reference breaks out of its loop, SVNICP.cpp:95-101) — same result, less idle launching when the run stops early. */
int svnicp_align_async(svnicp_ctx *ctx);

/* results — caller-allocated outputs, copied device -> host */
int svnicp_get_transformation(svnicp_ctx *ctx, double out6[6]);      /* SVNICP.cpp:286-290 / SVGDICP.cpp:497-499 */
int svnicp_get_distribution(svnicp_ctx *ctx, double out6[6]);        /* SVNICP.cpp:292-297 / SVGDICP.cpp:501-503 */
int svnicp_get_cov_matrix(svnicp_ctx *ctx, double out36[36]);        /* SVNICP.cpp:299-308 / SVGDICP.cpp:505-513 */
int svnicp_get_particles(svnicp_ctx *ctx, double *out6P);            /* SVGDICP.cpp:515-520: x..,y..,z..,rx..,ry..,rz.. */
int svnicp_get_particle_weight(svnicp_ctx *ctx, double *outP);       /* SVNICP.cpp:281-284 / SVGDICP.cpp:522-524 */
int svnicp_get_particle_history(svnicp_ctx *ctx, float *outIx6P);    /* SVGDICP.cpp:526-534: I rows of 6P float32 */
int svnicp_get_runtime(svnicp_ctx *ctx, double out3[3]);             /* SVGDICP.h:94-96 {knn_s, update_s, finish_iter} */

/* test / profiling knobs of a context, by name (the product configuration is the default of every one):
 *   knn = auto|v1|v2|brute|tiles   brute_qb = 0..6   fallback_sliced_max = <n>      accum = split|valu|f64
 *   update = auto|fused     fused_update_max_p = <P>       wgpcu = <search>,<accumulate>     tp = <points>    debug = 0|1
 *   single = fused|split    chain = auto|general|persistent   median = auto|stream|inline          correspondence = fast|full
 * The environment variable SVNICP_OPTIONS ("name=value;name=value") is read once, in svnicp_create. */
int svnicp_set_option(svnicp_ctx *ctx, const char *name, const char *value);

/* ---- mini-batch: SteinICPParam::use_minibatch / batch_size — SVGDICP::mini_batch_pair_generator (SVGDICP.cpp:176-199) -----
 * With a batch, iteration i of both solvers works on the source rows idx[i][0..batch_size) of a table int32
 * [iterations][batch_size] drawn with replacement (values in [0, B); batch_size may exceed B; a row drawn twice counts
 * twice) instead of the whole scan: correspondences, point_filter, the H / b sums, the SVGD non-zero count and its
 * (count + 1) normalisation are "over the batch"; gradient_scaling_factor_ stays the WHOLE cloud's size (:58, :454).  Stage A
 * is unchanged but runs only on the rows that were drawn.  Early stop, history, particle update and outputs are unchanged.
 * batch_size 0 = off (the default: full batch, exactly the launches of a context that never called this).
 * Generated tables: the table of the n-th registration after this call (n = 0, 1, ...; svnicp_align_begin advances n) is, at
 * flat position j of [0, iterations * batch_size), with splitmix64 as in svn-icp_amd/scans.py (arithmetic mod 2^64):
 *   base = splitmix64(seed * 1000003 + n);  bits = splitmix64(base + j);  idx = floor(bits * B / 2^64)
 * written on the device (no host pass); the Python mirror minibatch_indices() gives the same table bit for bit.  The
 * reference draws with libtorch's CUDA generator, which is not reproduced: what is pinned is the arithmetic GIVEN the table.
 * Refused by svnicp_align / svnicp_align_begin with SVNICP_ERR_INVALID: batch_size < 0, a partial particle shard
 * (svnicp_set_shard), a source-row shard (row_world > 1), the options correspondence=full and chain=persistent, and
 * iterations * batch_size > 2^22 rows (about 2.5 KB of candidate tables per row: 10 GB).  In this mode
 * svnicp_stage_candidates accepts only the whole range (0, B), svnicp_get_trace's corr is [I][P][batch_size], and
 * svnicp_get_candidates / svnicp_get_candidate_dist2 return SVNICP_ERR_INVALID (see svnicp_get_minibatch_candidates). */
int svnicp_set_minibatch(svnicp_ctx *ctx, int batch_size, uint64_t seed);
/* an explicit table int32 [iterations][batch_size] (host or device memory; copied), used by EVERY following registration
 * until svnicp_set_minibatch is called again: tests, replay of a recorded run.  A shape that does not match
 * params.iterations, or a value outside [0, B), makes the registration fail with SVNICP_ERR_INVALID: a host table is checked
 * in svnicp_align_begin; a device table is checked by the kernel that reads it (the value is never used as an address and
 * no iteration runs), which svnicp_align reports when it returns and svnicp_align_async at svnicp_synchronize. */
int svnicp_set_minibatch_indices(svnicp_ctx *ctx, const int32_t *idx, int iterations, int batch_size, int mem_kind);
/* taps, valid after a registration in mini-batch mode */
int svnicp_get_minibatch_indices(svnicp_ctx *ctx, int32_t *outIxb);      /* the table the last registration used */
int svnicp_get_minibatch_candidates(svnicp_ctx *ctx, int32_t *outIxbxK); /* candidate target indices per drawn position */
int svnicp_get_minibatch_rows(svnicp_ctx *ctx, int64_t out2[2]);         /* {unique rows drawn U, queries stage A ran} */

/* ---- point-to-plane residual (an extension: the reference computes point-to-point only) ----------
 * svnicp_set_residual(SVNICP_RESIDUAL_PLANE, huber_delta, normal_k): from the next registration on, SVN mode minimises
 * sum rho(r) over the accepted pairs with r = n . (T s - q), q the winner of the unchanged nearest-of-K search, n its unit
 * normal and rho the Huber function: weight w = 1 for |r| <= huber_delta, huber_delta / |r| beyond (huber_delta > 0; +inf =
 * unweighted).  A pair is accepted iff its squared distance is below max_dist (the gate of point mode, quirk included) and
 * q has a normal; a rejected pair contributes nothing.  Per particle, with Rt | tt its total pose, m = Rt^T n, j = [m ; s x m]:
 * H = sum w j j^T + 1e-6 I, b = sum w r j; the Stein step, early stop, history, outputs and trace taps are unchanged.
 * Normals: those of svnicp_set_target_normals, else estimated on the device when the registration begins — per target point
 * from its normal_k nearest target points, itself included (4..64; 0 = 16; stage A's exact search with the target as the
 * query cloud): covariance of the offsets, eigenvector of the smallest eigenvalue, sign unspecified (the residual does not
 * depend on it).  A point has NO normal when the offset to a neighbour is non-finite or has |d| >= 2^64 (see
 * svnicp_set_clouds, "non-finite and huge points"), when the largest eigenvalue l2 is 0 or when the middle one
 * l1 < 0.01 * l2 (collinear neighbourhoods: the same-ring neighbours of a sparse scan).  Estimated normals are
 * kept until the target or normal_k changes: a second registration against the same target pays nothing.
 * SVNICP_RESIDUAL_POINT (the default) runs exactly the launches of a context that never called this.
 * Refused by svnicp_align / svnicp_align_begin with SVNICP_ERR_INVALID in plane mode: SVGD mode, a partial particle shard, a
 * source-row shard, mini-batch mode, the options correspondence=full, chain=persistent and accum=f64|valu, knn_count > 128,
 * and a target of fewer than normal_k points without supplied normals. */
#define SVNICP_RESIDUAL_POINT 0   /* today's behaviour, the default */
#define SVNICP_RESIDUAL_PLANE 1
int svnicp_set_residual(svnicp_ctx *ctx, int residual, double huber_delta, int normal_k);
/* optional: normals of the current target, double [M][3], host or device (copied).  Must follow the svnicp_set_target /
 * svnicp_set_clouds it belongs to, with the same M; rows are normalised on upload (n / |n| in float64: a row that is already
 * unit comes back from svnicp_get_target_normals within 2 ulp, not necessarily bit for bit), a zero or non-finite row means "no
 * normal here" and stays zero, and so does a finite row whose squared norm overflows or underflows to 0 in float64 (entries
 * of 1e160, of 1e-170, subnormal entries: the norm is taken as sqrt(x x + y y + z z), unscaled; tests/test_plane_alone_gpu.py
 * pins it); a later svnicp_set_target drops them.  SVNICP_MEM_HOST: copied when the call returns.
 * SVNICP_MEM_DEVICE: the device-to-device copy is QUEUED on the context's stream, as svnicp_set_target's is: the rows must stay
 * unchanged until a call that synchronises that stream (svnicp_align, svnicp_synchronize) has returned. */
int svnicp_set_target_normals(svnicp_ctx *ctx, const double *n_xyz, int64_t M, int mem_kind);
/* taps: the supplied or estimated unit normals, rows without a normal are 0 (SVNICP_ERR_INVALID before there are any);
 * per particle {accepted pairs, sum w r^2} of the last iteration run, and the count of normal passes run so far
 * (either pointer may be NULL; outPx2 needs a finished registration in plane mode) */
int svnicp_get_target_normals(svnicp_ctx *ctx, double *outMx3);
int svnicp_get_plane_stats(svnicp_ctx *ctx, double *outPx2, int64_t *normal_passes);

/* ---- generalized-ICP residual (an extension) ---------------------------------------------------------
 * svnicp_set_residual_gicp(huber_delta, normal_k, epsilon): from the next registration on, SVN mode weighs every pair by the
 * combined covariance of BOTH local surfaces.  Notation of the plane residual: Rt | tt the particle's total pose, s the source
 * point, q the search kernel's winner, e = Ts - q, n_q the winner's unit normal, n_s the source point's unit normal.
 *   C(n) = I - (1 - epsilon) n n^T           regularised surface covariance: epsilon along the normal, 1 in the plane
 *   m = Rt^T n_q,  u = Rt^T e,  S = C(m) + C(n_s),  W = 2 epsilon S^-1     (closed-form inverse in float64; cond(S) <= 1/epsilon)
 *   rho = sqrt(u^T W u),  w = 1 for rho <= huber_delta else huber_delta / rho,  G = [I3 | -[s]x]
 *   H = sum w G^T W G + 1e-6 I,  b = sum w G^T W u         over the accepted pairs; W is frozen at the linearisation pose, so b
 *                                                          is the exact gradient of sum Huber(rho) with W held fixed
 * The factor 2 epsilon gives the cost the plane residual's units: parallel normals weigh 1 along the normal and epsilon across
 * it, W = (1 - epsilon) m m^T + epsilon I; epsilon = 1 gives W = I, the unweighted point-to-point cost.  huber_delta and the
 * pose prior's prior_point_sigma keep their meaning.  epsilon: 0 = 1e-3, else in [1e-6, 1]; huber_delta > 0 (+inf = unweighted);
 * normal_k 0 = 16, else 4..64, for BOTH clouds.
 * Accepted pairs: d2 < max_dist (the project's gate), the winner has a normal AND the source row has one; a rejected pair
 * contributes exact zeros.  Target normals: exactly as in plane mode (svnicp_set_target_normals, svnicp_get_target_normals,
 * svnicp_map_query_normals, or the target's own pass).  Source normals: those of svnicp_set_source_normals, else estimated when
 * the registration begins from each source point's normal_k nearest SOURCE points (the same kernel and validity rule as the
 * target's pass, neighbours from a stage A whose target is the source cloud); kept until the source or normal_k changes.
 * The mode is entered only here (svnicp_set_residual(2, ...) stays SVNICP_ERR_INVALID) and left by svnicp_set_residual(POINT |
 * PLANE, ...).  It runs the plane residual's launches with its own accumulate kernel, so the Stein step, the pose prior, early
 * stop, history, traces, svnicp_evaluate, svnicp_eval_information (forms point and plane), svnicp_score_particles and
 * svnicp_particle_modes behave as on a plane-mode context (the information matrix of THIS objective is
 * svnicp_eval_information_gicp); svnicp_plane_record_devptr / svnicp_plane_stats_devptr tap its
 * records ([P][2] = {accepted pairs, sum w rho^2}).
 * Refused by svnicp_align / svnicp_align_begin with SVNICP_ERR_INVALID: everything plane mode refuses, and a source of fewer
 * than normal_k points without supplied source normals. */
#define SVNICP_RESIDUAL_GICP 2
int svnicp_set_residual_gicp(svnicp_ctx *ctx, double huber_delta, int normal_k, double epsilon);
/* optional: normals of the current source, double [B][3], host or device (copied): the rules of svnicp_set_target_normals.
 * Must follow the svnicp_set_source / svnicp_set_clouds it belongs to, with the same B; dropped by the next one. */
int svnicp_set_source_normals(svnicp_ctx *ctx, const double *n_xyz, int64_t B, int mem_kind);
/* taps: the supplied or estimated unit normals of the source (SVNICP_ERR_INVALID before there are any); per particle
 * {accepted pairs, sum w rho^2} of the last iteration run and the normal passes run so far, {target, source} (either pointer
 * may be NULL; outPx2 needs a finished registration in generalized-ICP mode) */
int svnicp_get_source_normals(svnicp_ctx *ctx, double *outBx3);
int svnicp_get_gicp_stats(svnicp_ctx *ctx, double *outPx2, int64_t passes2[2]);

/* ---- Gaussian pose prior on the correction (an extension: the reference's posterior has no prior) --
 * svnicp_set_pose_prior(ctx, mean6, info36): from the next svnicp_align_begin on, SVN mode minimises, per particle,
 * 1/2 sum w |e|^2 + 1/2 e^T Lambda e with e = [t_p - mu_t ; Log(R_mu^T R_p)], (R_p, t_p) the particle's CORRECTION pose (not
 * the total pose R0 R_p), mean6 = [mu_t ; mu_r] in the coordinates of svnicp_get_transformation, R_mu = Exp(mu_r), and info36
 * = Lambda, 6x6 row-major in the order (t, r) of svnicp_get_cov_matrix.  In front of every Stein step one kernel adds
 * J^T Lambda e to b and J^T Lambda J to H of every particle, J = blkdiag(R_p, Jr^-1(e_r)), at the pose the iteration's
 * search used; the 1e-6 I of the data term stays, H stays exactly symmetric, and the trace taps H, b include the prior.
 * Domain |e_r| < pi.  A particle with a non-finite pose gets a non-finite record; the others are unaffected.
 * UNITS: Lambda is in the units of the cost, which has NO point noise in it (the data term is sum w |e|^2 in m^2).  For a
 * metric prior covariance Sigma and a point noise sigma_pt pass Lambda = sigma_pt^2 Sigma^-1.
 * info36 NULL: the prior is off (the default): exactly the launches of a context that never called this.
 * SVNICP_ERR_INVALID for a non-finite entry, |Lambda_ij - Lambda_ji| > 1e-12 max|Lambda|, a negative diagonal entry, a
 * smallest eigenvalue below -1e-12 max|Lambda|, or |mu_r| >= pi; the stored matrix is (Lambda + Lambda^T) / 2.
 * Refused by svnicp_align / svnicp_align_begin with SVNICP_ERR_INVALID while a prior is set: SVGD mode, a partial particle
 * shard, a source-row shard and the option chain=persistent.  Allowed: mini-batch mode, the plane residual,
 * correspondence=full, update=fused, particle weighting, any particle count.  With a prior the small chain and the fused
 * one-particle iteration are not chosen (neither has a place for the launch between the sums and the step).
 * svnicp_get_pose_prior: *on = a prior is set; mean6 / info36 (the symmetrised matrix) are written only then; any pointer
 * may be NULL. */
int svnicp_set_pose_prior(svnicp_ctx *ctx, const double mean6[6], const double info36[36]);
int svnicp_get_pose_prior(svnicp_ctx *ctx, int *on, double mean6[6], double info36[36]);

/* ---- evaluate a registration: fitness, inlier RMSE, nearest pairs (an extension: the reference returns a pose and a
 * covariance and nothing that says whether the registration worked) -------------------------------
 * svnicp_evaluate(ctx, R, t, max_corr_dist, out): one pose against the WHOLE target, on the device, blocking.
 *   pose         the total pose, map <- sensor.  R and t both NULL: the last registration's result, T0 * Pose3(Rot3::Expmap(
 *                mean[3:6]), mean[0:3]) with T0 of svnicp_set_initial_mean and mean of svnicp_get_transformation -- the
 *                composition both pipelines apply (correction_to_pose), in both solver modes.  Only one of the two NULL, or
 *                a non-finite entry: SVNICP_ERR_INVALID.
 *   transformed  q = R s + t in float64, unfused: (s0*R[3i] + s1*R[3i+1] + s2*R[3i+2]) + t[i].
 *   point
 *   nearest      exact over the whole target, stage A's contract (svnicp_set_clouds) with K = 1: smallest (d2, index), a NaN
 *   target       distance is never a neighbour.  The search is stage A's own, with the kernel the registration chose.
 *   evaluated    d2 is recomputed from q and the returned target row; a row is evaluated iff q is finite and that d2 is not
 *   rows         NaN (which also covers the contract's "index 0, d2 = 0.0" filler of a row with no eligible target).  A d2 of
 *                +inf is evaluated and never an inlier.
 *   inliers      evaluated rows with d2 < thr2, thr2 = max_corr_dist * max_corr_dist computed once in float64;
 *                max_corr_dist must be > 0 and not NaN, +inf is allowed.
 *   plane        has_normals = 1 iff the context holds normals of the current target: supplied by svnicp_set_target_normals,
 *   figures      or estimated by an earlier plane-mode registration and not dropped since; evaluate never runs a normal pass
 *                of its own.  A plane inlier is an inlier whose target normal n is non-zero; its residual is
 *                r = (n0 e0 + n1 e1) + n2 e2 with e = q - p.  Independent of the residual mode the solver ran.
 *   determinism  the same context state and arguments give bit-identical results on every call: each workgroup owns a fixed
 *                range of rows and the records are added in an order that depends on B alone (no atomics).
 *   when         there must be a finished registration since the source, the target, the initial mean, K, an option, the
 *                mini-batch or the residual setting last changed (stage A's target layout and scratch belong to that
 *                registration); otherwise SVNICP_ERR_INVALID, and svnicp_last_error names the reason.  A stage A that cannot
 *                search with K = 1 is refused too: the seeded scan (option knn=v2) unless knn_count is 1.  Returns with the
 *                stream synchronised and *out filled.
 *   side         none: nothing an existing getter returns changes (svnicp_get_knn_fallbacks, _fallback_rows and _survivors
 *   effects      keep describing the registration), and the next registration is bit for bit that of a context that never
 *                evaluated.
 *   sharded      a row-sharded context evaluates its own rows; the counts and the two sums add across ranks.
 * The per-row results stay in device memory until the next svnicp_evaluate. */
typedef struct svnicp_eval {
  int32_t struct_size;    /* in: sizeof(svnicp_eval) */
  int32_t has_normals;    /* 1: the context holds normals of the current target, plane figures are filled */
  int64_t rows;           /* B, the context's source rows */
  int64_t evaluated;      /* rows with a finite transformed point and a nearest target whose d2 is not NaN */
  int64_t inliers;        /* evaluated rows with d2 < max_corr_dist * max_corr_dist */
  int64_t plane_inliers;  /* inliers whose nearest target has a normal (0 without normals) */
  double sum_d2, sum_r2;  /* over inliers; over plane_inliers */
  double fitness;         /* inliers / rows */
  double inlier_rmse;     /* sqrt(sum_d2 / inliers), 0 when there are none */
  double plane_rmse;      /* sqrt(sum_r2 / plane_inliers), 0 when there are none */
  double R[9], t[3];      /* the pose that was evaluated (row-major), also when NULL was passed */
} svnicp_eval;
int svnicp_evaluate(svnicp_ctx *ctx, const double R_rowmajor[9], const double t[3], double max_corr_dist, svnicp_eval *out);
const int32_t *svnicp_eval_index_devptr(svnicp_ctx *ctx);   /* int32 [B]: nearest target row, -1 = not evaluated */
const double *svnicp_eval_dist2_devptr(svnicp_ctx *ctx);    /* double [B]: its d2, NaN = not evaluated */
int svnicp_get_eval_pairs(svnicp_ctx *ctx, int32_t *idxB, double *d2B);   /* host copy of the two; either may be NULL */

/* ---- information matrix of a registration: the Gauss-Newton normal equations at an evaluated pose, their eigen-structure
 * and what follows from it (an extension: the reference meant to hand a "Hessian_for_KF" to its filter, include/core/SVNICP.h:45,
 * and left it commented out) ---------------------------------------------------------------------
 * svnicp_eval_information(ctx, form, huber_delta, eig_floor_ratio, out): the sums on the device, then
 * svnicp_information_solve on the host; blocking.
 *   rows         those of the LAST svnicp_evaluate: its pose T = (R, t) (returned in out->R, out->t), its gate
 *                (out->max_corr_dist), its per-row nearest target index and d2, and the q = R s + t it left on the device.  No
 *                second search.
 *   tangent      right perturbation T * Exp([v ; omega]), translation first: the solver's order (svnicp_get_trace H).  GTSAM's
 *                Pose3 orders [omega ; v]: swap the two 3-blocks of H, b, step and cov before handing them to GTSAM.
 *   terms        s = the source row, p = its nearest target row, e = q - p.
 *   point form   rows: evaluate's inliers.  d = sqrt(d2), w = 1 if d <= delta else delta / d; c = R^T e;
 *   (form 0)     H += w [[I, -hat(s)], [hat(s), |s|^2 I - s s^T]];  b += w [c ; s x c];  sum_wr2 += w d2.
 *                H[0:3,0:3] is sum_w * I whatever the scene: this form can never show a translational degeneracy.
 *   plane form   rows: evaluate's plane inliers (inlier, and the target's normal n != 0).  r = (n0 e0 + n1 e1) + n2 e2,
 *   (form 1)     w = 1 if |r| <= delta else delta / |r|;  m = R^T n, j = [m ; s x m];
 *                H += w j j^T;  b += w r j;  sum_wr2 += w r^2.
 *                The form is the caller's choice, independent of the residual the solver ran (as evaluate's plane figures).
 *   both         huber_delta = +inf: unweighted.  pairs = the exact count of contributing rows, sum_w = sum of w.  H is the
 *                CLEAN normal matrix: no + 1e-6 I and no terms for rejected pairs -- not the solver's quirk-compatible H that
 *                svnicp_get_trace returns.  Operands of rows that do not contribute are selected to zero, never multiplied:
 *                a NaN or inf row reaches no sum.
 *   determinism  the same context state and arguments give bit-identical structs: each workgroup owns a fixed range of rows
 *                and every addition happens in an order that depends on B alone (no atomics).
 *   when         SVNICP_ERR_INVALID, with the reason in svnicp_last_error, unless a svnicp_evaluate has succeeded since the
 *                source, the target or the target normals were last set and since the last registration began
 *                (svnicp_align_begin, so also svnicp_align and svnicp_align_async).  Also refused: an unknown form;
 *                huber_delta not > 0 (NaN included); eig_floor_ratio outside [0, 1); a wrong struct_size; the plane form when
 *                that evaluate had has_normals = 0.
 *   side         none: no existing getter changes -- svnicp_get_eval_pairs and the two eval device pointers included -- and the
 *   effects      next registration is bit for bit that of a context that never asked.
 *   sharded      a row-sharded context returns the sums of its own rows.  H, b, pairs, sum_w and sum_wr2 ADD across ranks;
 *                svnicp_information_solve on the added struct finishes it (every derived field of a rank's own struct
 *                describes that rank's rows only).  No collective is run here.
 * svnicp_information_solve(io): host only -- no context, no device.  From form, pairs, sum_wr2, eig_floor_ratio, H and b it
 * fills rank, sigma2, eigval, eigvec, eig_t, vec_t, eig_r, vec_r, step and cov; every other field is left as it is.
 *   eigen        cyclic Jacobi in float64 with a fixed sweep count on (H + H^T) / 2 and on its two diagonal 3x3 blocks.
 *                Eigenvalues ascending; row i of eigvec is the unit eigenvector of eigval[i], its largest-magnitude component
 *                positive (the lowest index decides a tie).
 *   floor        f = eig_floor_ratio in [0, 1); 0 means 1e-12.  Jacobi's eigenvalues carry an ABSOLUTE error of about
 *                6 u |H| (u = 2^-53, |H| the largest eigenvalue), i.e. 7e-16 |H|: a true zero comes back as +-1e-15 |H|.  The
 *                default sits three orders above that, so rounding never counts as rank, and far below any direction a scan
 *                does constrain (lambda_min / lambda_max of a real scene: 1e-4 .. 1e-2).
 *   rank         the number of eigval[i] > f * eigval[5].
 *   H+, step     H+ = sum over the `rank` largest of v v^T / lambda;  step = -H+ b (the Gauss-Newton step in the tangent
 *                above: a stationary result has |step| near 0);  no component along a direction below the floor.
 *   sigma2, cov  dof = dim * pairs - rank with dim = 3 (point, GICP) or 1 (plane);  sigma2 = sum_wr2 / dof if dof > 0 else 0;
 *                cov = sigma2 * H+: the Gauss-Newton covariance of the pose AT this one pose, in the tangent above -- not
 *                svnicp_get_cov_matrix, which is the particle spread in correction coordinates.
 *   edge cases   a zero H gives rank 0, zero eigenvalues, step, sigma2 and cov (the eigenvectors are the unit axes) and no
 *                NaN.  A non-finite entry of H or b (or sum_wr2), a form, floor or struct_size as above: SVNICP_ERR_INVALID.
 *                Forms 0, 1 and 3 are known (2 is not a form).
 *
 * svnicp_eval_information_gicp(ctx, huber_delta, epsilon, eig_floor_ratio, out): the same in the generalized-ICP objective of
 * svnicp_set_residual_gicp, sum Huber(sqrt(u^T W u)) -- what a filter or a degeneracy gate must be handed after a registration
 * in that mode.  A function of its own because the form has one more argument;
 * svnicp_eval_information(ctx, 3, ...) stays refused as an unknown form.  Everything said above holds (tangent, both,
 * determinism, side effects, sharded, the solve), and:
 *   rows         those of the LAST svnicp_evaluate, as above: its pose, gate, nearest target index, d2 and q.  No second
 *                search and no normal pass.  A row contributes iff it is one of evaluate's plane inliers (an inlier whose
 *                target normal n_q is non-zero) and the context holds a normal n_s for the source row: a row of the packed
 *                source record that is not all zero, the rule of the mode's accumulate kernel.
 *   GICP form    e = q - p, u = R^T e, m = R^T n_q, G = [I3 | -hat(s)], C(x) = I - (1 - epsilon) x x^T;
 *   (form 3)     W = 2 epsilon (C(m) + C(n_s))^-1   (closed-form inverse in float64, cond <= 1 / epsilon);
 *                rho = sqrt(max(u^T W u, 0)),  w = 1 if rho <= delta else delta / rho;
 *                H += w G^T W G;  b += w G^T W u;  sum_w += w;  sum_wr2 += w rho^2;  pairs += 1.
 *                W is frozen at the evaluated pose, as in the solver, so b is the exact gradient of sum Huber(rho) with W
 *                held fixed, and step is near 0 at a converged registration of that mode.  H is the clean normal matrix.
 *                epsilon = 1 gives the point form's H and b on these rows; parallel normals (n_s = m) and delta = +inf give
 *                (1 - epsilon) of the plane form's H plus epsilon of the point form's.
 *   epsilon      0 = 1e-3, else in [1e-6, 1] (svnicp_set_residual_gicp's rule).  The caller's choice, independent of the
 *                residual the solver ran and of its epsilon, as the form is.
 *   when         as svnicp_eval_information, and also refused with SVNICP_ERR_INVALID: epsilon out of range; a last
 *                svnicp_evaluate with has_normals = 0; a context without normals of the current source (they come from
 *                svnicp_set_source_normals, or from a registration in generalized-ICP mode that estimated them, and are
 *                dropped with the source).
 *   result       form = SVNICP_INFO_GICP; the struct and every other field as above, dim = 3 in the solve. */
#define SVNICP_INFO_POINT 0
#define SVNICP_INFO_PLANE 1
#define SVNICP_INFO_GICP 3
typedef struct svnicp_information {
  int32_t struct_size;     /* in: sizeof(svnicp_information) */
  int32_t form;            /* SVNICP_INFO_POINT | SVNICP_INFO_PLANE | SVNICP_INFO_GICP */
  int64_t pairs;           /* contributing rows, exact */
  int32_t rank;            /* eigenvalues above the floor */
  int32_t reserved;
  double huber_delta, eig_floor_ratio;   /* as passed */
  double max_corr_dist;    /* the gate of the evaluate the rows came from */
  double sum_w, sum_wr2;   /* sum of the weights; of w d2 (point) or w r^2 (plane) */
  double sigma2;           /* sum_wr2 / dof, 0 when dof <= 0 */
  double H[36], b[6];      /* row-major, order [v ; omega] */
  double eigval[6], eigvec[36];   /* ascending; row i = unit eigenvector i */
  double eig_t[3], vec_t[9], eig_r[3], vec_r[9];   /* of the blocks H[0:3,0:3] and H[3:6,3:6] */
  double step[6], cov[36]; /* -H+ b; sigma2 * H+ */
  double R[9], t[3];       /* the evaluated pose (row-major) */
} svnicp_information;
int svnicp_eval_information(svnicp_ctx *ctx, int form, double huber_delta, double eig_floor_ratio, svnicp_information *out);
int svnicp_eval_information_gicp(svnicp_ctx *ctx, double huber_delta, double epsilon, double eig_floor_ratio, svnicp_information *out);
int svnicp_information_solve(svnicp_information *io);   /* host only: no context, no device */

/* ---- score and weight the particles (an extension: the reference declares ParticleWeightOpt::use_weight_mean,
 * include/core/SVNICP.h:25-27, and writes its getters for arbitrary weights, SVNICP.cpp:286-308, but particle_weight_ never
 * becomes anything but ones / P) --------------------------------------------------------------------
 * svnicp_score_particles(ctx, max_corr_dist, outPx6, posesPx12): every particle's final pose scored through the candidate
 * table the registration built -- the nearest-of-K rule of the iterations, not svnicp_evaluate's search of the whole target.
 *   poses        particle p is scored at the total pose the device holds after the last executed update, [R0 R_p | t0 + R0 t_p]:
 *                the pose the next iteration's search would have used, also after an early stop.  posesPx12 (may be NULL)
 *                returns exactly those 12 doubles per particle, R row-major, then t.  The kernels ignore the stop flag.
 *   transformed  for source row b: T_i = (s0*R[3i] + s1*R[3i+1] + s2*R[3i+2]) + t[i], float64, unfused (the search's).
 *   point
 *   winner       among the knn_count candidates cand[b][0..K) of the registration (svnicp_candidates_devptr): e = T - q_k,
 *                d2 = ((e0*e0) + e1*e1) + e2*e2, strict '<' from candidate 0, exactly the "search" rule under
 *                svnicp_set_clouds: a NaN first distance is never replaced.  Candidate indices are clamped to [0, M) before
 *                they become addresses.
 *   classes      a row is evaluated iff T is finite and the winner's d2 is not NaN; an inlier iff evaluated and d2 < thr2,
 *                thr2 = max_corr_dist * max_corr_dist computed once in float64; a plane inlier iff an inlier, the context holds
 *                normals of the current target (svnicp_evaluate's has_normals; no normal pass is ever run here) and the
 *                winner's normal n is non-zero, with r = (n0*e0 + n1*e1) + n2*e2.  sum_d2 runs over the inliers, sum_r2 =
 *                sum r*r over the plane inliers; operands of rejected pairs are selected to zero, never multiplied.
 *   cost         cost_p = (sum_d2_p + (B - inliers_p) * thr2) / B, the mean truncated squared distance: a row that is not an
 *                inlier costs the gate.  max_corr_dist must be finite and > 0, so the cost is always finite.
 *   out          outPx6, per particle: {evaluated, inliers, plane_inliers, sum_d2, sum_r2, cost}; the counts are exact
 *                integers held in doubles.
 *   determinism  no atomics: each workgroup owns a fixed range of rows and the records are added in an order that depends on
 *                B and P alone; the same context state gives the same bits on every call.
 *   when         as svnicp_evaluate: a finished registration since the source, the target, the initial mean, K, an option,
 *                the mini-batch or the residual setting last changed; otherwise SVNICP_ERR_INVALID with the reason in
 *                svnicp_last_error.  Refused after a registration that ran with a partial particle shard, a source-row shard,
 *                mini-batch mode or the option correspondence=full; allowed in SVGD mode, in plane mode, for every stage-B
 *                variant and chain and any K the registration accepted.  Synchronises first and returns with the results on
 *                the host.
 * svnicp_set_particle_weighting(ctx, kind, max_corr_dist, temperature): SVNICP_WEIGHT_UNIFORM (the reference, the default)
 * runs exactly the launches of a context that never called this.  With SVNICP_WEIGHT_SOFTMIN every following registration
 * ends (svnicp_finish, so also svnicp_align and svnicp_align_async) with one scoring at max_corr_dist, the weights
 *   w_p = exp(-(cost_p - cost_min) / temperature) / Z      (Z added in particle order; temperature in m^2, finite and > 0)
 * and the reference's own weighted expressions in float64, every sum in particle order: mean_i = sum_p x_ip w_p,
 * var_i = sum_p (x_ip - mean_i)^2 w_p, cov_rc = sum_p w_p (x_rp - mean_r)(x_cp - mean_c).  svnicp_get_transformation,
 * svnicp_get_distribution, svnicp_get_cov_matrix and svnicp_get_particle_weight (w) return them, and what builds on the mean
 * follows: svnicp_evaluate(NULL, NULL), the pipelines' correction_to_pose.  For any kind but UNIFORM the setter itself refuses
 * a max_corr_dist or temperature that is not finite and > 0 (SVNICP_ERR_INVALID).  Refused by svnicp_align /
 * svnicp_align_begin with SVNICP_ERR_INVALID while weighting is on: an unknown kind, SVGD mode (the option belongs to SVNICP's
 * constructor only), a partial particle shard, a source-row shard, mini-batch mode (its candidate tables are per drawn
 * position) and the option correspondence=full.
 * svnicp_get_particle_scores: the last scoring, whoever ran it -- a weighted registration supplies it at no extra GPU work;
 * SVNICP_ERR_INVALID before there is one.
 * Side effects: none.  No existing getter changes in UNIFORM mode, and the next registration of a context that scored or
 * weighted is bit for bit that of one that never did. */
#define SVNICP_SCORE_FIELDS 6
/* per particle p: {evaluated, inliers, plane_inliers, sum_d2, sum_r2, cost}; the counts are exact integers held in doubles */
int svnicp_score_particles(svnicp_ctx *ctx, double max_corr_dist, double *outPx6, double *posesPx12);
#define SVNICP_WEIGHT_UNIFORM 0   /* the reference, the default */
#define SVNICP_WEIGHT_SOFTMIN 1
int svnicp_set_particle_weighting(svnicp_ctx *ctx, int kind, double max_corr_dist, double temperature);
int svnicp_get_particle_scores(svnicp_ctx *ctx, double *outPx6, double *posesPx12);  /* of the last scoring, whoever ran it */

/* ---- score and weight the particles in the objective the solver minimised ----------------------
 * svnicp_score_particles knows one cost, the mean truncated squared point distance.  After a registration with the plane
 * residual (svnicp_set_residual) or the generalized-ICP residual (svnicp_set_residual_gicp) that is not what the iterations
 * minimised: sliding along a wall costs nothing there and a lot in the point cost.  These three score and weight in either
 * residual's own terms.  Purely additive: svnicp_score_particles, svnicp_set_particle_weighting and every getter are unchanged.
 * svnicp_score_particles_objective(ctx, obj, outPx6, posesPx12):
 *   shared       poses, transformed point, winner, the classes `evaluated` and `inlier`, index clamping, determinism, `when`
 *                and the four refusals are those of svnicp_score_particles, word for word.  The output is the same [P][6]
 *                device block: svnicp_get_particle_scores, the weights, the weighted statistics and svnicp_particle_modes'
 *                best / cost_min / cost_mean read its field 5 whatever form wrote it.
 *   form         SVNICP_SCORE_POINT: exactly svnicp_score_particles(max_corr_dist) -- the same launches, the same bits;
 *                huber_delta and epsilon are checked and not used.  SVNICP_SCORE_PLANE, SVNICP_SCORE_GICP: below.
 *                SVNICP_SCORE_AS_SOLVED resolves at the call from the registration begun last: point residual -> POINT;
 *                plane -> PLANE with the solver's huber_delta; GICP -> GICP with the solver's huber_delta and epsilon (a
 *                huber_delta or epsilon passed with AS_SOLVED is checked and then replaced by the solver's).
 *                An explicit form is the caller's choice, independent of the residual that ran, as with
 *                svnicp_eval_information: a point-mode registration followed by svnicp_set_target_normals and form PLANE is fine.
 *   out          forms PLANE and GICP, per particle: {evaluated, inliers, accepted, sum_d2, sum_h, cost}.
 *   robust term  for x >= 0: h(x) = x*x if x <= delta else delta*(2*x - delta): twice Huber's rho, so delta = +inf gives x*x
 *                and the unit stays m^2, as for the point cost and the temperature.  The branch is a select.  h is continuous.
 *   PLANE        accepted: a plane inlier exactly as in svnicp_score_particles (an inlier, the context holds target normals,
 *                the winner's normal n is non-zero).  r = (n0*e0 + n1*e1) + n2*e2, sum_h = sum h(|r|) with x*x = r*r.  With
 *                delta = +inf the fields 0..4 equal svnicp_score_particles' fields 0..4 bit for bit.
 *   GICP         accepted: a plane inlier whose source row has a non-zero normal in the context's packed source record (the
 *                rule of the mode's accumulate kernel).  u = R^T e, m = R^T n, W = 2 eps (C(m) + C(n_s))^-1 (the closed form
 *                of svnicp_eval_information_gicp), rho2 = max(u^T W u, 0), sum_h = sum h(sqrt(rho2)); inside delta the term is
 *                rho2 itself, no square root.
 *   cost         cap = h(max_corr_dist); cost = (sum_h + (B - accepted) * cap) / B.  The cap is derived, not chosen: |n| = 1
 *                and W's eigenvalues lie in [epsilon, 1], so x <= |e| < max_corr_dist and every accepted pair costs at most
 *                cap: a particle cannot lower its cost by shedding pairs.  Rows without a normal (target or, for GICP, source)
 *                cost cap for every particle alike.  The cost is finite.
 *   refused      SVNICP_ERR_INVALID with the reason in svnicp_last_error: a struct_size mismatch; an unknown form; a
 *                max_corr_dist that is not finite and > 0; huber_delta negative or NaN; epsilon neither 0 nor in [1e-6, 1];
 *                PLANE without normals of the current target in the context (no normal pass is ever run by a scoring); GICP
 *                without them, or without normals of the current source (svnicp_set_source_normals, or a registration in
 *                generalized-ICP mode that estimated them); knn_count too large for one row's candidates to fit the kernel's
 *                LDS tile; and everything svnicp_score_particles refuses.
 * svnicp_set_particle_weighting_objective(ctx, kind, obj, temperature): SVNICP_WEIGHT_SOFTMIN makes every following
 * registration end with one scoring in obj in place of the point cost; with AS_SOLVED the form is resolved at each
 * svnicp_align_begin (a form that then lacks its normals refuses the registration).  The weights and the weighted statistics
 * are computed as under svnicp_set_particle_weighting, with its refusals (SVGD mode, the two shards, mini-batch,
 * correspondence=full); a later svnicp_set_particle_weighting puts the point cost back.  SVNICP_WEIGHT_UNIFORM (obj may be
 * NULL) runs exactly the launches of a context that never called either setter.
 * svnicp_get_score_objective(ctx, out): the RESOLVED objective of the last scoring, whoever ran it (form never AS_SOLVED;
 * huber_delta and epsilon as used, 0 where the form has none); SVNICP_ERR_INVALID before there is one.
 * Not in the cost: the pose prior's chi^2.  Not available: shards, mini-batch, weighting in SVGD mode. */
#define SVNICP_SCORE_AS_SOLVED (-1)  /* the residual of the registration begun last */
#define SVNICP_SCORE_POINT 0         /* svnicp_score_particles' cost, unchanged */
#define SVNICP_SCORE_PLANE 1
#define SVNICP_SCORE_GICP  2
typedef struct svnicp_score_objective {
  size_t struct_size;     /* in: sizeof(svnicp_score_objective) */
  int    form;            /* one of the four above */
  double max_corr_dist;   /* finite, > 0: the gate, as today */
  double huber_delta;     /* > 0, +inf = no robust weight; 0 = the solver's own (svnicp_set_residual / _gicp) */
  double epsilon;         /* GICP only: 0 = the solver's own, else [1e-6, 1]: svnicp_set_residual_gicp's rule and constants */
} svnicp_score_objective;
int svnicp_score_particles_objective(svnicp_ctx *ctx, const svnicp_score_objective *obj, double *outPx6, double *posesPx12);
int svnicp_set_particle_weighting_objective(svnicp_ctx *ctx, int kind, const svnicp_score_objective *obj, double temperature);
int svnicp_get_score_objective(svnicp_ctx *ctx, svnicp_score_objective *out);  /* the RESOLVED objective of the last scoring */

/* ---- particle modes: the particle set clustered on the device (an extension: the reference publishes particles and weights
 * and stops there; every getter above collapses the set into one mean, which lies between the peaks of a posterior that has
 * more than one) -----------------------------------------------------------------------------------
 * svnicp_particle_modes(ctx, opt, out): blocking; one kernel launch, one copy of about 16 KB.
 *   input        the particle 6-vectors x_p = (t, omega) that svnicp_get_particles returns (the device's [6][P] block) with the
 *                weights svnicp_get_particle_weight returns (uniform, or soft-min when weighting is on); or, with
 *                opt->particles6xP, a caller's host [6][P] block with opt->weightsP (NULL: every weight is 1.0).
 *   link         p and q are linked iff dt2 <= link_trans * link_trans AND dr2 <= link_rot * link_rot, both squares computed
 *                once, with d = x_p - x_q per component, dt2 = ((d0*d0) + d1*d1) + d2*d2 and dr2 = ((d3*d3) + d4*d4) + d5*d5:
 *                float64, unfused.  dr2 is on the COMPONENT DIFFERENCES of the rotation vectors, not a geodesic angle: the
 *                particles are small corrections about the initial mean, where the two agree to second order.  A particle with
 *                a non-finite component links to nothing, belongs to no mode and is counted in `nonfinite`.
 *   modes        the connected components of the link graph over the finite particles; a mode's label is its lowest particle
 *                index.  (Device: each particle takes the lowest label among its links, pointers are jumped, and the sweep is
 *                repeated until nothing changes; the pair distances are recomputed every sweep.  The result does not depend on
 *                the schedule.)
 *   per mode     count;  W = sum of the members' weights;  mass = W / W_all, W_all the same sum over all finite particles;
 *                mean_i = (sum w_p * x_ip) / W;  cov_rc = (sum w_p * ((x_rp - mean_r) * (x_cp - mean_c))) / W.  Every sum runs
 *                over the members in ascending particle order from 0.0, in float64, unfused; no atomics.  The division by W
 *                is deliberate: the global getters above do not normalise (the reference's float32(1 / P) * P != 1 shows in
 *                them); a mode's statistics do not depend on the scale of the weights.  A mode of zero weight has NaN
 *                statistics (0 / 0).
 *   order        descending W, ties to the lower label.  n_modes counts all modes; the first n_reported = min(n_modes,
 *                max_modes) are reported in full, the arrays beyond are zero (best: -1).
 *   total pose   R, t of a mode: T0 * Pose3(Rot3::Expmap(mean[3:6]), mean[0:3]) -- the composition svnicp_evaluate(ctx, NULL,
 *                NULL, ...) applies to the global mean (the same function), row-major, map <- sensor; hand it to
 *                svnicp_evaluate to judge a mode instead of the mean.
 *   scores       has_scores = 1 iff the context holds a scoring of exactly the particles that were clustered: the set of the
 *                last registration, scored by svnicp_score_particles or by a weighted registration since that registration began
 *                and since svnicp_set_particles.  Then per mode: best = the member with the lowest cost (strict '<' in particle
 *                order: ties to the lowest index), cost_min its cost, cost_mean = (sum of the members' costs in particle
 *                order) / count, unweighted.  Otherwise (always for a caller's set) best = -1 and the costs are 0.
 *   when         with opt->particles6xP == NULL: after a finished registration of any kind -- SVN or SVGD mode, plane residual,
 *                mini-batch, particle shards and row shards (the Stein step is replicated: every rank holds all P poses),
 *                correspondence=full; otherwise SVNICP_ERR_INVALID.  A caller's set needs no registration, no clouds and no
 *                svnicp_set_particles (clustering an earlier iteration out of svnicp_get_particle_history is the use).
 *                Synchronises first.
 *   refused      SVNICP_ERR_INVALID with the reason in svnicp_last_error: a struct_size mismatch of either struct; max_modes
 *                outside 1..SVNICP_MODES_MAX; a link that is negative or not finite; P < 1 with a caller's set; weightsP without
 *                particles6xP; a supplied weight that is negative or not finite; more than 2048 particles (one workgroup
 *                stages the set in LDS; there is no global-memory fallback).
 *   determinism  the same particles, weights and options give bit-identical structs and labels on every call.
 *   side         none: every existing getter returns what it returned before, and the next registration is bit for bit that
 *   effects      of a context that never asked.  The kernel ignores the stop flag.
 * svnicp_get_mode_labels(ctx, outP): per particle of the last svnicp_particle_modes the rank of its mode in the order above
 * (0 = the heaviest; ranks beyond n_reported included), -1 for a non-finite particle.  outP holds that call's `particles`
 * entries.  SVNICP_ERR_INVALID before the first successful call. */
#define SVNICP_MODES_MAX 32
typedef struct svnicp_modes_opt {
  int32_t struct_size;          /* = sizeof(svnicp_modes_opt) */
  int32_t max_modes;            /* 1..SVNICP_MODES_MAX */
  double link_trans, link_rot;  /* metres, radians; finite, >= 0 */
  const double *particles6xP;   /* host [6][P]; NULL: the last registration's set */
  int32_t P;                    /* with particles6xP only */
  int32_t reserved;
  const double *weightsP;       /* host [P], with particles6xP only; NULL: equal weights */
} svnicp_modes_opt;
typedef struct svnicp_modes {
  int32_t struct_size;   /* in: sizeof(svnicp_modes) */
  int32_t particles;     /* P of the set that was clustered */
  int32_t nonfinite;     /* particles with a non-finite component: in no mode */
  int32_t n_modes;       /* all modes */
  int32_t n_reported;    /* min(n_modes, max_modes): the entries filled below */
  int32_t has_scores;    /* 1: best, cost_min, cost_mean are filled */
  int32_t label[SVNICP_MODES_MAX];   /* lowest particle index of the mode */
  int32_t count[SVNICP_MODES_MAX];   /* members */
  int32_t best[SVNICP_MODES_MAX];    /* member with the lowest cost, -1 without scores */
  double mass[SVNICP_MODES_MAX];     /* W / W_all */
  double cost_min[SVNICP_MODES_MAX], cost_mean[SVNICP_MODES_MAX];
  double mean[SVNICP_MODES_MAX][6], cov[SVNICP_MODES_MAX][36];   /* in correction coordinates, as svnicp_get_transformation */
  double R[SVNICP_MODES_MAX][9], t[SVNICP_MODES_MAX][3];         /* the mode's total pose, row-major */
} svnicp_modes;
int svnicp_particle_modes(svnicp_ctx *ctx, const svnicp_modes_opt *opt, svnicp_modes *out);
int svnicp_get_mode_labels(svnicp_ctx *ctx, int32_t *outP);

/* ---- split-phase entry points: one process per GPU, particles sharded across ranks ----------
 * (new functionality; the reference is single-GPU).  Sequence per registration:
 *   svnicp_set_shard -> svnicp_stage_candidates(b_lo,b_hi) -> [host all-gathers rows of
 *   svnicp_candidates_devptr] -> svnicp_build_candidate_table -> per iteration:
 *   svnicp_iter_accumulate -> [host all-gathers svnicp_sums_devptr, 22 doubles per particle] ->
 *   svnicp_iter_update ; finally svnicp_finish.  svnicp_align == all of it with one shard. */
int svnicp_set_shard(svnicp_ctx *ctx, int p_lo, int p_hi);
/* ---- the other split: SOURCE ROWS sharded across ranks (the one bench.py --gpus N uses) ---------------------------
 * Rank r is given only ITS rows of the source scan (svnicp_set_source / svnicp_set_clouds with the row slice) and the
 * whole target; it runs stage A, the candidate table and the per-iteration search + accumulation on those rows for ALL
 * particles, so nothing of size [B] is replicated or gathered.  Its 22 sums per particle are a partial record; the ranks
 * exchange them (all-gather of row_world x P x 22 doubles into svnicp_rank_sums_devptr, slot = row_rank) and
 * svnicp_iter_update adds the records in rank order before the Stein step — every rank the same values in the same
 * order, so the replicas stay bit-identical.  total_source_points = the whole scan's B (SVGD mode scales by it,
 * SVGDICP.cpp:58).  row_world = 1 returns to the unsharded behaviour.  May be combined with svnicp_set_shard
 * (2-D split): the record slot [row_rank][p_lo, p_hi) is then this rank's contribution.
 * Sequence: svnicp_set_row_shard -> svnicp_align_begin -> svnicp_stage_candidates(0, rows) ->
 * svnicp_build_candidate_table -> per iteration { svnicp_iter_accumulate -> [all-gather] -> svnicp_iter_update } ->
 * svnicp_finish. */
int svnicp_set_row_shard(svnicp_ctx *ctx, int row_rank, int row_world, int64_t total_source_points);
void *svnicp_rank_sums_devptr(svnicp_ctx *ctx);  /* double [row_world][P][SVNICP_NSUMS]; NULL unless row_world > 1 */
int svnicp_align_begin(svnicp_ctx *ctx);
int svnicp_stage_candidates(svnicp_ctx *ctx, int64_t b_lo, int64_t b_hi);
int svnicp_build_candidate_table(svnicp_ctx *ctx);
int svnicp_iter_accumulate(svnicp_ctx *ctx, int iteration);
int svnicp_iter_update(svnicp_ctx *ctx, int iteration);
int svnicp_finish(svnicp_ctx *ctx);
int svnicp_stopped(svnicp_ctx *ctx);     /* 1 once the early-stop flag is set (syncs the stream) */
void *svnicp_candidates_devptr(svnicp_ctx *ctx); /* int32 [B][K] */
void *svnicp_sums_devptr(svnicp_ctx *ctx);       /* double [P][SVNICP_NSUMS] */
/* the total poses stage B reads (test tap, no device work): double [P][12], R_total row-major then t_total
 * (SVNICP.cpp:58-59).  Valid after svnicp_align_begin; a test may overwrite it before svnicp_iter_accumulate, and the
 * next svnicp_iter_update or svnicp_set_particles rewrites it.  NULL before svnicp_set_particles. */
void *svnicp_total_pose_devptr(svnicp_ctx *ctx);
#define SVNICP_NSUMS 22

/* ---- local map in HBM: svnicp::VoxelHashMap — src/core/VoxelHashMap.cpp:22-101, include/core/VoxelHashMap.h ----------
 * voxel -> at most max_points points (float32, insertion order); the query result is float64 rows in device memory that
 * svnicp_set_target(..., SVNICP_MEM_DEVICE) copies device-to-device, so the target never crosses PCIe. */
typedef struct svnicp_map svnicp_map;
/* VoxelHashMap(voxel_size, max_range, max_pointscount) — VoxelHashMap.h:39-42; capacity_voxels 0 = default (2^20, grows) */
int svnicp_map_create(int device, double voxel_size, double max_range, int max_points, int64_t capacity_voxels,
                      svnicp_map **out);
void svnicp_map_destroy(svnicp_map *map);
const char *svnicp_map_last_error(const svnicp_map *map);
int svnicp_map_clear(svnicp_map *map);                        /* VoxelHashMap::Clear — VoxelHashMap.h:55 */
int svnicp_map_size(svnicp_map *map, int64_t *voxels);        /* VoxelHashMap::Size / Empty — VoxelHashMap.h:56-57 */
/* VoxelHashMap::AddPointCloud(cloud, pose) incl. RemoveFarPointCloud — VoxelHashMap.cpp:22-42, 89-97.
 * xyz: n x 3 float32 (pcl::PointXYZ) in the sensor frame, host or device; pose = rotation (row-major) + translation */
int svnicp_map_add_cloud(svnicp_map *map, const float *xyz, int64_t n, int mem_kind, const double R_rowmajor[9],
                         const double t[3]);
/* points svnicp_map_add_cloud has not stored since creation / clear because they lie outside +-2^20 voxels or are NaN
 * (the reference would index a voxel for them; here they are counted and the call still succeeds) */
int svnicp_map_skipped_points(svnicp_map *map, int64_t *out);
/* the hash table as the host knows it (test tap, no device work): slots of the table, tombstones counted by the statistics the
 * last modifying call read back, and table rebuilds (growth or tombstone clearing) since creation — svnicp_map_clear keeps
 * the capacity and the rebuild count.  Any out pointer may be NULL. */
int svnicp_map_table_info(svnicp_map *map, int64_t *capacity_slots, int64_t *tombstones, int64_t *rebuilds);
/* VoxelHashMap::GetMap(pose, max_range) — VoxelHashMap.cpp:48-58; center NULL or max_range < 0: GetMap() (:44-46).
 * The points are written as float64 [count][3] rows into a device buffer owned by the map (valid until the next query),
 * voxels in ascending (x, y, z) index, points of a voxel in insertion order. */
int svnicp_map_query(svnicp_map *map, const double center[3], double max_range, int64_t *count_out);
void *svnicp_map_points_devptr(svnicp_map *map);              /* double [count][3] of the last query */
int svnicp_map_download(svnicp_map *map, double *out_xyz, int64_t cap_points, int64_t *n_out); /* test tap */
/* normals of the rows of the LAST svnicp_map_query, from the 27-voxel neighbourhoods of the map: the candidates of a row are
 * all points the map stores in the 3 x 3 x 3 block of voxels around the row's own voxel (selected by the query or not; voxel
 * indices outside +-2^20 do not exist), enumerated in ascending (x, y, z) voxel index and slot; its neighbours are the
 * normal_k candidates smallest by (d2, enumeration order), d2 = ((dx*dx)+dy*dy)+dz*dz in float64 of the widened float32
 * coordinates; normal and validity from them exactly as for svnicp_set_residual's own pass (two-pass scatter matrix of the
 * offsets to the point, 8 Jacobi sweeps, lambda1 >= 0.01 * lambda2).  Fewer than normal_k candidates: no normal (a zero row).
 * Nothing is stored in the map, and the same map gives bit-identical normals on every call.
 * normal_k 4..64, 0 = 16.  SVNICP_ERR_INVALID: no query yet, or the map changed (add_cloud / clear) since the last query,
 * or normal_k out of range.  Complete when the call returns, like the query.  with_normal_out may be NULL.  An empty
 * selection is not an error: nothing is written and *with_normal_out = 0. */
int svnicp_map_query_normals(svnicp_map *map, int normal_k, int64_t *with_normal_out);
void *svnicp_map_normals_devptr(svnicp_map *map);      /* double [count][3], rows as svnicp_map_points_devptr's; feeds
                                                          svnicp_set_target_normals(..., SVNICP_MEM_DEVICE), whose copy is
                                                          stream-ordered: synchronise the context (svnicp_align does) before the
                                                          next query / add_cloud / clear, which invalidate the rows (NULL then) */
int svnicp_map_download_normals(svnicp_map *map, double *out_xyz, int64_t cap_points, int64_t *n_out);   /* test tap */
/* ---- score candidate poses against the map (an extension: the reference starts every registration at the constant-velocity
 * prediction and has no way to look for a better start) ------------------------------------------
 * svnicp_map_score_poses(map, src_xyz, n, src_mem_kind, posesCx12, C, poses_mem_kind, max_corr_dist, outCx4): how well do the
 * n rows of a scan fit the map at each of C poses, straight from the hash table -- no target cloud, no candidate table.
 *   poses        posesCx12 holds 12 doubles per pose, R row-major then t, map <- sensor: the layout of svnicp_score_particles'
 *                posesPx12.  Host or device memory (poses_mem_kind); src_xyz is n x 3 float32 in the sensor frame, host or
 *                device (src_mem_kind).
 *   transformed  exactly svnicp_map_add_cloud's: c[d] = (float)(((R[3d]*(double)p0 + R[3d+1]*(double)p1) + R[3d+2]*(double)p2)
 *   point        + t[d]), formed in float64 from the widened float32 row, left to right, rounded ONCE to float32.
 *   voxel        truncf(c[d] / (float)voxel_size) per axis, valid in [-2^20, 2^20); otherwise the row is not located -- also for
 *                NaN and inf, hence for every row of a pose with a non-finite entry.  A non-finite pose is never an error: its
 *                record is {0, 0, 0, thr2}.
 *   candidates   all points the map stores in the 3 x 3 x 3 block of voxels around that voxel.  Voxel indices outside +-2^20 do
 *                not exist; per-voxel counts are clamped to [0, max_points]; the table is only read: probing is bounded, goes on
 *                past a removed voxel's slot and stops at an empty one.
 *   distance     d2 = ((dx*dx) + dy*dy) + dz*dz in float64, dx = (double)stored - (double)c; dmin2 the minimum over the
 *                candidates.
 *   classes      a row is located iff its voxel is valid and its block holds at least one stored point; an inlier iff located
 *                and dmin2 < thr2, thr2 = max_corr_dist * max_corr_dist computed once in float64, the comparison strict.
 *   sums         sum_d2 runs over the inliers; cost = (sum_d2 + (n - inliers) * thr2) / n, the mean truncated squared distance
 *                of svnicp_score_particles, so costs of the two calls read alike.
 *   gate         max_corr_dist must be finite, > 0 and <= voxel_size, otherwise SVNICP_ERR_INVALID.  Up to that size the nearest
 *                point of the block is the nearest point of the whole map -- except for a stored point whose float32 quotient
 *                coordinate / voxel_size rounded across a voxel boundary, which sits one voxel further than its coordinates say.
 *                The contract itself is the block; that is why the result is exact.
 *   out          outCx4 (host, may be NULL: read svnicp_map_scores_devptr), per pose {located, inliers, sum_d2, cost}; the
 *                counts are exact integers held in doubles.
 *   determinism  no atomics: each workgroup owns a fixed range of 256 rows of one pose and the partial records are added in an
 *                order that depends on n alone.  The record of a pose has the same bits whether it is scored alone or in a
 *                batch of any C, with rows and poses on the host or on the device, and the same bits on every call.
 *   limits       0 <= n <= 2^31-1, 1 <= C <= 2^20.  n == 0 gives {0, 0, 0, thr2} for every pose.  An empty map is not an error:
 *                nothing is located.
 *   side         none on the map: svnicp_map_size and svnicp_map_table_info are unchanged, the rows of an earlier
 *   effects      svnicp_map_query and its normals stay valid (the call has its own buffers, svnicp_map_query_normals is still
 *                accepted), and a following svnicp_map_add_cloud leaves the map bit for bit that of a map that never scored.
 *   completion   returns with the map's stream synchronised and outCx4 filled. */
#define SVNICP_MAP_SCORE_FIELDS 4   /* per pose: {located, inliers, sum_d2, cost}; counts are exact integers held in doubles */
int svnicp_map_score_poses(svnicp_map *map, const float *src_xyz, int64_t n, int src_mem_kind, const double *posesCx12, int64_t C,
                           int poses_mem_kind, double max_corr_dist, double *outCx4 /* host */);
void *svnicp_map_scores_devptr(svnicp_map *map);   /* double [C][4] of the last scoring, NULL before one */
/* ---- coarse-to-fine pose search against the map -------------------------------------------------
 * svnicp_map_search_poses(map, src_xyz, n, src_mem_kind, guess_R, guess_t, opt, out): levels of scored nodes around `guess`, each
 * level three times finer than the one before, only the `keep` best nodes of a level expanded.  Nodes are made, scored and
 * ranked on the device in one enqueue: no host synchronisation and no host-to-device copy between levels.
 *   lattice      every node is an integer vector k[6] on the finest lattice.  fine[a] = step[a] / (double)3^(levels-1), one
 *                division (0 on an axis whose step is not finite and > 0); the correction of a node is x[a] = (double)k[a] *
 *                fine[a], one multiplication, in the solver's parametrisation [x, y, z, rx, ry, rz].  m[a] = floor(extent[a] /
 *                step[a] + 1e-9), 0 for extent 0; axis a is active iff m[a] >= 1; A is the number of active axes.
 *   level 0      the nodes k[a] = j * 3^(levels-1), j = -m[a]..m[a], in lexicographic order with x slowest: prod(2m+1) nodes.
 *                With levels == 1 this is the flat grid of k * step, bit for bit.
 *   level l+1    for each kept node of level l in rank order and each offset o in {-1, 0, 1}^A (lexicographic over the active
 *                axes, x slowest) the child k_parent + o * 3^(levels-2-l), at index rank * 3^A + offset index:
 *                kept_l * 3^A nodes, kept_l = min(keep, count_l).  Children of distinct parents never coincide; children may
 *                leave +-extent by less than half a level-0 step.
 *   pose         guess * correction_to_pose(x), the total pose of a particle: R = G_R * Exp(x[3:6]) (Rodrigues), t[d] =
 *                ((G_R[3d]*x0 + G_R[3d+1]*x1) + G_R[3d+2]*x2) + G_t[d]; float64, unfused.
 *   record       per node {located, inliers, sum_d2, cost} with the bits svnicp_map_score_poses gives for that pose scored alone.
 *   rank         ascending (cost, k lexicographic with x first); costs compare as doubles and are never NaN.  At level 0
 *                lexicographic order is index order.
 *   limits       1 <= levels <= 8, 1 <= keep <= 1024, every level's count <= 2^20, m[a] * 3^(levels-1) + (3^(levels-1) - 1) / 2
 *                < 2^20 per axis, extents finite and >= 0, a finite step > 0 on an axis with an extent, max_corr_dist under the
 *                gate rule of svnicp_map_score_poses, a finite guess, 0 <= n <= 2^31-1, no NULL among guess, opt and out:
 *                otherwise SVNICP_ERR_INVALID and nothing is enqueued.  n == 0 and an empty map are not errors: all costs tie at
 *                the squared gate and the lexicographically smallest nodes are kept.
 *   out          levels, active_axes, nodes_scored (all levels), level_count / level_kept per level, fine_step, and of the best
 *                node of the last level its lattice vector, correction, pose (R row-major, then t) and record; zero_record is
 *                the level-0 record of the zero correction, i.e. of `guess` itself.
 *   determinism  the same bits on every call, and with rows on the host or on the device.
 *   side         none on the map, on svnicp_map_scores_devptr or on an earlier svnicp_map_query's rows and normals: the search
 *   effects      has its own buffers, which hold every level until the next search.  A following svnicp_map_add_cloud leaves
 *                the map bit for bit that of a map that never searched.
 *   completion   returns with the map's stream synchronised. */
#define SVNICP_MAP_SEARCH_MAX_LEVELS 8
#define SVNICP_MAP_SEARCH_MAX_KEEP 1024
typedef struct svnicp_map_search_opt { double extent[6], step[6]; int levels, keep; double max_corr_dist; } svnicp_map_search_opt;
typedef struct svnicp_map_search {
  int levels, active_axes; int64_t nodes_scored; int64_t level_count[8]; int32_t level_kept[8];
  double fine_step[6]; int32_t best_lattice[6]; double best_correction[6], best_pose[12], best_record[4], zero_record[4];
} svnicp_map_search;
int svnicp_map_search_poses(svnicp_map *map, const float *src_xyz, int64_t n, int src_mem_kind,
                            const double guess_R_rowmajor[9], const double guess_t[3],
                            const svnicp_map_search_opt *opt, svnicp_map_search *out);
/* the kept nodes of the last level of the last search in rank order, at most cap of them (host arrays; any output may be NULL;
 * *n_out = how many there are, whatever cap is).  No device work.  SVNICP_ERR_INVALID before a search, or for cap < 0. */
int svnicp_map_search_top(svnicp_map *map, int cap, int32_t *latticeNx6, double *correctionsNx6, double *posesNx12,
                          double *recordsNx4, int *n_out);
/* test tap: level `level` of the last search -- the first min(cap, count) nodes' lattice vectors, poses and records and the
 * level's kept list (indices into the level, rank order, level_kept entries: size kept_indices for 1024); any output may be NULL.
 * SVNICP_ERR_INVALID before a search, for a level outside [0, levels) or cap < 0. */
int svnicp_map_search_level(svnicp_map *map, int level, int64_t cap, int32_t *latticeCx6, double *posesCx12, double *recordsCx4,
                            int32_t *kept_indices, int64_t *count_out, int *kept_out);

/* ---- test-only taps (parity tests; not part of the reference interface) -------------------- */
int svnicp_get_candidates(svnicp_ctx *ctx, int32_t *outBK);          /* sourceKNN_idx_  SVGDICP.cpp:214 */
int svnicp_get_candidate_dist2(svnicp_ctx *ctx, double *outBK);
/* plane mode, valid after svnicp_align_begin (NULL otherwise): the record one svnicp_iter_accumulate leaves, before any
 * Stein step reads it (tests/test_plane_alone_gpu.py) */
void *svnicp_plane_record_devptr(svnicp_ctx *ctx); /* double [P][42]: H (36, mirrored, + 1e-6 on the diagonal) | b (6) */
void *svnicp_plane_stats_devptr(svnicp_ctx *ctx);  /* double [P][2]: {accepted pairs, sum w r^2} */
/* the particles' correction poses as the kernels hold them, valid after svnicp_set_particles (NULL otherwise):
 * which = 0: R double [P][9] row-major, which = 1: t double [P][3] (tests/test_pose_prior_gpu.py reads and crafts them) */
void *svnicp_particle_pose_devptr(svnicp_ctx *ctx, int which);
/* (both are allocated max(P, Ppad) rows long, Ppad from svnicp_get_stage_b_grid: the rows from P on belong to the padded
 * particles of the stage-B grid and are never written) */
/* stage B's launch grid of the registration svnicp_align_begin began: {grid_x, grid_y, pts_per_block, Ppad} — the accumulate
 * kernel runs grid_x x grid_y workgroups of pts_per_block source points each, and the finalize / reduce kernel adds grid_x
 * records per particle.  SVNICP_ERR_INVALID before svnicp_align_begin. */
int svnicp_get_stage_b_grid(svnicp_ctx *ctx, int out4[4]);
/* valid when params.record_trace != 0; any pointer may be NULL.
 * corr: [I][P][B] int32 (-1 where not run), H [I][P][36], b [I][P][6], newton [I][P][6],
 * phi [I][P][6], h [I] */
int svnicp_get_trace(svnicp_ctx *ctx, int32_t *corr, double *H, double *b, double *newton,
                     double *phi, double *h);
/* iterations the last align executed (= iterations unless the early stop fired); svnicp_get_runtime()[2] is the
 * reference's finish_iter_, which SVN mode never updates */
int svnicp_get_iterations_run(svnicp_ctx *ctx, int *out);
/* elapsed GPU milliseconds of the last align, by phase: {stage A (candidates + table),
 * iterations (accumulate + update), total} — measured with hipEvents on the context's stream */
int svnicp_get_gpu_ms(svnicp_ctx *ctx, double out3[3]);

/* number of queries of the last stage A that the pre-filtered kernel handed to the streaming
 * fallback (-1 when the streaming kernel ran alone) */
int svnicp_get_knn_fallbacks(svnicp_ctx *ctx, int *out);
/* the source rows behind that count (at most `cap` of them, unordered); *n_out = the count */
int svnicp_get_knn_fallback_rows(svnicp_ctx *ctx, int32_t *out, int cap, int *n_out);
/* per source point: how many targets survived the float32 pre-filter of the pruned stage-A kernel
 * (needs params.record_trace) */
int svnicp_get_knn_survivors(svnicp_ctx *ctx, int32_t *outB);
/* wave steps of the last align whose float32 nearest-candidate search was not decisive and were
 * redone in float64 (-1 when the float64 kernel ran alone) */
int svnicp_get_ambiguous_steps(svnicp_ctx *ctx, int *out);
/* (source point, particle) pairs of the last align that the bf16 matrix-pipe search could not certify and handed to its
 * exact float64 pass (-1 when another search kernel ran) */
int svnicp_get_ambiguous_pairs(svnicp_ctx *ctx, int64_t *out);
/* bench hook: when on, every kernel launch of an align is bracketed by hipEvents on the
 * context's stream; svnicp_get_kernel_ms then returns the summed milliseconds and launch counts
 * per kernel class of the LAST align, SVNICP_KERNEL_CLASSES entries in this order:
 *   0 stage A (ordering + k_knn_tiles/k_knn_scan + fallback)   1 k_build_table*
 *   2 k_stein_search_bf16 (split stage B only)                 3 k_stein_accumulate* (fused variants: whole stage B)
 *   4 k_reduce_partials                                        5 k_particle_update / k_upd_*
 * (plane residual: 3 = k_plane_accumulate, 4 = k_plane_finalize; generalized-ICP residual: 3 = k_gicp_accumulate, 4 = the same) */
#define SVNICP_KERNEL_CLASSES 6
/* on: 0 = off, 1 = every class, otherwise a mask with bit (class + 1) set for each class to bracket (the event
 * pairs cost ~5 us of stream time each, so a timed run brackets only what it reports) */
int svnicp_set_profile(svnicp_ctx *ctx, int on);
int svnicp_get_kernel_ms(svnicp_ctx *ctx, double *ms6, int32_t *launches6);

/* ---- per-scan pre-processing on the device ------------------------------------------------
 * What OdometryPipeline::ICP_processing does to a scan before the solver sees it (src/core/OdometryPipeline.cpp):
 * crop_pointcloud (:692-704), pcl::UniformSampling at 0.5 * voxel_size (:559, :684-690) and at 1.5 * voxel_size of that
 * cloud (:560).  Mind the reference's aliasing: downsample_uniform filters the cloud it is handed IN PLACE
 * (uniform_sampling_.filter(*cloud) on its own input, :684-690), so after :559 *cropped_cloud holds the 0.5-voxel sampling
 * and after :560 *voxelized_cloud_toMap holds the 1.5-voxel one: the map is SEEDED with the 0.5-voxel cloud (:585,
 * svnicp_prep_map_cloud_devptr) and UPDATED with the 1.5-voxel cloud (:630, svnicp_prep_source_f32_devptr) — the same
 * points the solver registers.  The raw float32 scan is uploaded once; the three clouds stay in
 * device memory for svnicp_map_add_cloud(..., SVNICP_MEM_DEVICE) and svnicp_set_source(..., SVNICP_MEM_DEVICE).
 * Leaves are emitted in ascending linear index, the point closest to a leaf centre survives, first in input order on
 * ties (svn-icp_amd/host/registration_pipeline.hpp: downsample_uniform).  scan_max_range: in/out, the largest SQUARED
 * norm seen so far (:699, kept as the reference keeps it).  The counts are valid until the next svnicp_prep_scan. */
typedef struct svnicp_prep svnicp_prep;
int svnicp_prep_create(int device, svnicp_prep **out);
void svnicp_prep_destroy(svnicp_prep *prep);
const char *svnicp_prep_last_error(const svnicp_prep *prep);
int svnicp_prep_scan(svnicp_prep *prep, const float *xyz, int64_t n, int mem_kind, double min_range, double max_range,
                     double voxel_size, double *scan_max_range, int64_t *n_cropped, int64_t *n_map, int64_t *n_source);
const float *svnicp_prep_cropped_devptr(svnicp_prep *prep);    /* float32 [n_cropped][3] */
const float *svnicp_prep_map_cloud_devptr(svnicp_prep *prep);  /* float32 [n_map][3]     */
const double *svnicp_prep_source_devptr(svnicp_prep *prep);    /* float64 [n_source][3]: the solver's source cloud */
const float *svnicp_prep_source_f32_devptr(svnicp_prep *prep); /* the same points as float32 rows: what the map is UPDATED with */
int svnicp_prep_download(svnicp_prep *prep, int which /* 0 cropped, 1 map cloud, 2 source */, float *out_xyz,
                         int64_t cap_points, int64_t *n_out);   /* test tap */

/* ---- deskew (motion compensation) ahead of the crop: OdometryPipeline::deskew_pointcloud (:357-447) ----------------------
 * The reference deskews when deskew_cloud_ is set (on in config/ICP_parameters.yaml:18) and its pose buffer holds two poses
 * (:551-554: from the third scan on), then crops the DESKEWED cloud (:556, scan_max_range included) and samples it as above.
 * stamps: the per-point field "t" / "timestamp" / "time" (:364-367) of type stamp_type, widened to double (:372-381, :403-413);
 * NULL = no such field: all zero, min == max, the raw scan goes on (:418) — "no stamps" means "no deskew", not an error.
 * flags SVNICP_DESKEW_KITTI (cloud_topic "/kitti/velo/pointcloud", :385-401): stamps are ignored; each point p is rotated by
 * 0.205 deg about (p x z).normalized() (a zero axis stays zero, Eigen) into a float32 copy and stamped 0.5 * (yaw / pi + 1),
 * yaw = -atan2(y, x) of the corrected float32 coordinates, as a float.  min / max over the stamps (:414-417); min == max
 * returns the UNMODIFIED scan (:418; KITTI: without the correction); otherwise s = (t - min) / (max - min) (:419-423) and
 * p' = float32(Pose3::Expmap((s - 0.5) * delta_xi).transformFrom(double(p))) (:436-445).  delta_xi = Pose3::Logmap of
 * start^-1 * finish of the last two buffered poses (:427-432), [omega, v] (the caller computes it; pipeline.py /
 * registration_pipeline.hpp: se3_log).  Deliberate deviation: non-finite stamps take no part in min / max (the reference's
 * std::minmax_element result depends on where a NaN sits) and their points come out as NaN, which the crop drops.
 * mem_kind applies to xyz AND stamps.  SVNICP_ERR_INVALID for an unknown stamp_type or flag, a NULL or non-finite delta_xi.
 * The outputs (cropped / map cloud / source / source_f32, the counts, scan_max_range) mean exactly what they mean after
 * svnicp_prep_scan.  Same host synchronisation as svnicp_prep_scan (one, after the crop), two kernels in place of its crop
 * kernel.  Float64 Expmap on the device with the expressions of registration_pipeline.hpp; GTSAM / Eigen / PCL are absent,
 * so parity with the reference is unpinned. */
#define SVNICP_STAMP_F64 0
#define SVNICP_STAMP_F32 1
#define SVNICP_STAMP_U32 2
#define SVNICP_DESKEW_KITTI 1
int svnicp_prep_scan_deskew(svnicp_prep *prep, const float *xyz, const void *stamps, int stamp_type, int64_t n, int mem_kind,
                            const double delta_xi[6], int flags, double min_range, double max_range, double voxel_size,
                            double *scan_max_range, int64_t *n_cropped, int64_t *n_map, int64_t *n_source);
const float *svnicp_prep_deskewed_devptr(svnicp_prep *prep);   /* float32 [n][3]: every point after the deskew, before the crop */
int svnicp_prep_download_deskewed(svnicp_prep *prep, float *out_xyz, int64_t cap_points, int64_t *n_out);   /* test tap; valid
                                                                 until the next svnicp_prep_scan_deskew */

/* ---- range-image segmentation of a raw scan: LeGO-LOAM ImageProjection::cloudHandler (include/segmentation/ImageProjection.h)
 * OdometryPipeline::lidar_msg_cb (:328-355) runs it on every raw scan when USE_Segmentation is set (declared true, :180; off
 * in the shipped yamls) and hands GetSegmentedCloudPure() on, which returns segmentedCloud_ (:533-534).  Steps:
 *   input       (:240)      points with a non-finite coordinate are dropped; input order and input indices are kept.
 *   projection  (:281-325)  va = float(double(atan2f(z, sqrtf(x*x+y*y)) * 180.0f) / M_PI), q = (va + ang_bottom) / ang_res_y
 *                           (float); q is converted to size_t as on x86-64: q in (-1, 0) is row 0, q <= -1 or trunc(q) >=
 *                           n_scan drops the point.  h = float(double(atan2f(x, y) * 180.0f) / M_PI), col = -round((double(h)
 *                           - 90) / double(ang_res_x)) + horizon_scan / 2 (double, C round); col >= H: col -= H; a negative
 *                           or still too large col drops the point.  r = sqrtf(x*x + y*y + z*z); r < min_range drops it.
 *                           Several points in one pixel: the LAST in input order wins (xyz and range).
 *   ground      (:329-374)  rows 0..ground_scan_ind; pair (r, r+1) of a column is valid when both are filled and flat when
 *                           fabsf(float(double(atan2f(dz, sqrtf(dx*dx+dy*dy)) * 180.0f) / M_PI) - mount_angle) <= 10.  The
 *                           loop's overwrites give: ground(r) = -1 if r < G and pair (r, r+1) is invalid, else 1 if pair
 *                           (r, r+1) or (r-1, r) is flat, else 0.
 *   components  (:379-383, :435-531)  4-neighbour graph on the pixels that are filled and not ground (label 0); columns wrap,
 *                           rows do not; an edge when atan2f(d2*sin(a), d1 - d2*cos(a)) > segment_theta (d1 / d2 the larger /
 *                           smaller range, a = ang_res / 180 * pi of that direction).  A component (BFS from its row-major
 *                           first pixel) is valid with >= 30 pixels, or with >= valid_point_num pixels on >= valid_line_num
 *                           rows counting every member but the seed (lineCountFlag is set on push, :501).  Valid components
 *                           are labelled 1, 2, ... in seed order, the others 999999.
 *   output      (:384-414)  pixels row-major; kept when (label > 0 or ground == 1) and label != 999999, ground pixels only
 *                           at j % 5 == 0, j <= 5 or j >= H - 5: the winning point's xyz and its input index.
 * Deliberate deviation: every atan2f / sinf / cosf above is the float64 function of the float32 operands rounded once to
 * float32 (sin / cos of the alphas on the host); everything else is IEEE + - * / sqrt with -ffp-contract=off.  Host libms'
 * atan2f are not correctly rounded and disagree with each other, so this fixes one rule that the device and both host
 * restatements (pipeline.py / registration_pipeline.hpp: segment_scan) follow bit for bit; a decision can differ from a
 * glibc build of the reference only where a value lies within one float ulp of a threshold.
 * Device form (csrc/range_segment.hip): owner image by atomicMax of the input index, per-pixel ground / label-init, union-
 * find with minimum-index roots (the root of a component is its BFS seed, independent of scheduling), per-root size and row
 * mask, validity and labels by an exclusive scan, a stable compaction.  One host synchronisation, at the end.
 * The segmented buffers are the prep object's own: they may be passed to svnicp_prep_scan / svnicp_prep_scan_deskew with
 * SVNICP_MEM_DEVICE (those calls never write them); valid until the next svnicp_prep_segment.  The per-point stamps of the
 * raw message do not survive: segmentedCloud_ is PointXYZI, and the deskew that follows finds no time field (:363-381). */
typedef struct svnicp_seg_params {
  int32_t struct_size;           /* = sizeof(svnicp_seg_params) */
  int32_t n_scan, horizon_scan, ground_scan_ind;   /* N_SCAN, Horizon_SCAN, groundScanInd (:63-68) */
  float ang_res_x, ang_res_y, ang_bottom;          /* degrees */
  float min_range, mount_angle, segment_theta;     /* sensorMinimumRange, sensorMountAngle (deg), segmentTheta (rad) (:112-114) */
  int32_t valid_point_num, valid_line_num;         /* segmentValidPointNum, segmentValidLineNum (:115-116) */
} svnicp_seg_params;
/* the sensor blocks of ImageProjection.h:46-110 */
#define SVNICP_SEG_VLP16 0
#define SVNICP_SEG_HDL32E 1
#define SVNICP_SEG_HDL64E 2     /* the one the header compiles in */
#define SVNICP_SEG_VLS128 3
#define SVNICP_SEG_RS32 4
#define SVNICP_SEG_OS1_16 5
#define SVNICP_SEG_OS1_64 6
#define SVNICP_SEG_OS0_128 7
int svnicp_seg_default_params(int sensor, svnicp_seg_params *out);   /* no device needed; SVNICP_ERR_INVALID for an unknown id */
/* SVNICP_ERR_INVALID (nothing enqueued) unless 1 <= ground_scan_ind < n_scan <= 128, horizon_scan >= 1, n_scan * horizon_scan
 * <= 2^19, finite positive ang_res_x / ang_res_y, finite ang_bottom / min_range / mount_angle / segment_theta and a matching
 * struct_size.  params NULL = HDL-64E. */
int svnicp_prep_segment(svnicp_prep *prep, const float *xyz, int64_t n, int mem_kind, const svnicp_seg_params *params,
                        int64_t *n_segmented);
const float *svnicp_prep_segmented_devptr(svnicp_prep *prep);          /* float32 [n_segmented][3] */
const int32_t *svnicp_prep_segmented_index_devptr(svnicp_prep *prep);  /* int32 [n_segmented]: input index of each point */
int svnicp_prep_download_segmented(svnicp_prep *prep, float *out_xyz, int32_t *out_index, int64_t cap_points, int64_t *n_out);
int svnicp_prep_download_seg_images(svnicp_prep *prep, int32_t *owner, float *range, int8_t *ground, int32_t *label,
                                    int64_t cap_pixels);   /* test taps: row-major [n_scan][horizon_scan] of the last call; owner
                                                              -1 / range -100000 = empty; label as labelMat_ (-1, 1.., 999999) */

/* ---- visibility-based clearing of the local map (not in the reference): drop the stored points the new scan sees through
 * A stored map point is deleted when the scan's beam in its direction returned from clearly BEHIND it.  Inputs: the scan (n x 3
 * float32, sensor frame, host or device), its pose R | t (double, map <- sensor), the sensor geometry (of svnicp_seg_params
 * only n_scan, horizon_scan, ang_res_x, ang_res_y, ang_bottom and min_range are read) and the options below.
 *   image       [n_scan][horizon_scan] float32, empty = +inf.  A scan point takes part iff it passes the projection of the
 *               segmentation block above unchanged (finite coordinates, the row rule, the column rule, r >= min_range), with
 *               that block's row, column and r = sqrtf((x*x+y*y)+z*z).  A pixel keeps the MINIMUM r of its points (not the
 *               last point: the conservative choice for a rule that deletes, and independent of the input order).
 *   map point   p (float32) of every live voxel: d = double(p) - t, s_c = float((R[0][c]*d0 + R[1][c]*d1) + R[2][c]*d2)
 *               (R^T d, unfused, rounded once), projected by the same function to (row, col, r_m).  The point is KEPT when it
 *               does not project (outside the vertical field of view, non-finite, r_m < min_range), when r_m > max_range, or
 *               when its own pixel is empty.  Otherwise r_min = the minimum of the filled pixels over rows row + dr,
 *               |dr| <= window_rows, inside [0, n_scan) (rows do not wrap) and columns (col + dc) mod horizon_scan,
 *               |dc| <= window_cols (columns wrap), and the point is REMOVED iff
 *                   r_m < r_min - fmaxf(margin_abs, margin_rel * r_min)      (float32, unfused; equality keeps the point).
 *               The window is part of the rule: at grazing incidence one pixel spans metres of range, and a single-pixel test
 *               eats the ground.
 *   voxel       survivors keep their order and are compacted to the front; the next survivor becomes the voxel's first point,
 *               which svnicp_map_add_cloud's range cull and svnicp_map_query(center, r) read as before.  A voxel left empty
 *               becomes a tombstone exactly as the range cull makes one, and svnicp_map_add_cloud's rebuild rule applies
 *               unchanged; a later svnicp_map_add_cloud refills freed room in input order.
 * The call invalidates the last query like svnicp_map_add_cloud (svnicp_map_query_normals refuses until the next query).  It
 * is complete when it returns (one host synchronisation, for the statistics).  Two calls with the same inputs on equal maps
 * give bit-identical maps, and the host restatements (pipeline.py / registration_pipeline.hpp: clear_seen_through) follow
 * the device point for point.
 * SVNICP_ERR_INVALID, nothing enqueued: a NULL map / R / t / sensor / opt / out, scan_xyz NULL with n > 0, a struct_size that
 * does not match, n_scan outside 1..128, horizon_scan < 1, n_scan * horizon_scan > 2^19, ang_res_x / ang_res_y not finite and
 * positive, ang_bottom / min_range not finite, window_rows outside 0..4, window_cols outside 0..8, a negative or non-finite
 * margin, a non-positive or non-finite max_range, n < 0 or n > 2^31 - 1.  n = 0 or an empty map: success, zero statistics. */
typedef struct svnicp_visibility_opt {
  int32_t struct_size;                    /* = sizeof(svnicp_visibility_opt) */
  int32_t window_rows, window_cols;       /* 0..4, 0..8 */
  float margin_abs, margin_rel, max_range;   /* m, ratio of r_min, m */
} svnicp_visibility_opt;
typedef struct svnicp_visibility_stats {
  int64_t pixels_filled;     /* pixels of the image that hold a finite range */
  int64_t points_tested;     /* stored points that reached the comparison */
  int64_t points_removed;
  int64_t voxels_emptied;    /* voxels that became tombstones */
} svnicp_visibility_stats;
int svnicp_map_clear_seen_through(svnicp_map *map, const float *scan_xyz, int64_t n, int mem_kind, const double R_rowmajor[9],
                                  const double t[3], const svnicp_seg_params *sensor, const svnicp_visibility_opt *opt,
                                  svnicp_visibility_stats *out);

#ifdef __cplusplus
}
#endif
#endif /* SVNICP_HIP_H */
