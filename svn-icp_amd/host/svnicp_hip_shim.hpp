// svnicp_hip_shim.hpp — header-only C++ mirror of the reference solver classes over the C ABI.
//
// Same class and method names, argument meaning and call order as svnicp::SVGDICP / svnicp::SVNICP
// (/root/reference/svn-icp/include/core/SVGDICP.h:64-110, SVNICP.h:29-43) as used by
// OdometryPipeline::ICP_processing (src/core/OdometryPipeline.cpp:573-607), with raw buffers in
// place of torch::Tensor and a row-major 3x3 + translation in place of gtsam::Pose3.  A ROS2 node
// keeps its call sequence and links libsvnicp_hip.so instead of libtorch.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "svnicp_hip.h"
#include "../csrc/information_solve.hpp"

namespace svnicp {

enum SteinICPState { ALIGN_SUCCESS = 1, NO_OPTIMIZER = 2 };  // SVGDICP.h:59-62

struct SteinICPParam {  // SVGDICP.h:41-57 (same names and defaults; solver-relevant fields)
  int iterations = 50;
  bool use_minibatch = false;   // SVGDICP::mini_batch_pair_generator (SVGDICP.cpp:176-199): batch_size rows per iteration
  int batch_size = 50;
  uint64_t minibatch_seed = 0;  // seed of the generated tables (not in the reference; svnicp_hip.h "mini-batch")
  double lr = 0.02;
  double max_dist = 1.0;
  std::string optimizer = "Adam";
  bool check_early_stop = false;
  double convergence_threshold = 1e-5;
  int KNN_count = 100;
  bool SVN_full_grad = true;
  std::string residual = "point";   // "point" (the reference) | "plane": Huber-weighted point-to-plane | "gicp": generalized ICP (svnicp_hip.h, neither in the reference)
  double huber_delta = 0.1;         // plane residual: weight 1 up to this |r|, huber_delta / |r| beyond
  int normal_k = 16;                // plane residual: neighbours a target normal is estimated from (4..64)
  double gicp_epsilon = 1e-3;       // gicp residual: a surface's covariance along its normal, in units of the in-plane one ([1e-6, 1])
};

// SVNICP.h:25-27.  use_weight_mean alone is as inert as in the reference (particle_weight_ stays ones / P); with weight_dist > 0
// as well (not in the reference) every registration ends with one scoring of the particles at that gate (metres) and soft-min
// weights of `temperature` (m^2, > 0) that the getters honour (svnicp_hip.h "score and weight the particles").  weight_cost:
// "point" (the mean truncated squared point distance) or "solved": the residual the registration ran with, plane or
// generalized-ICP, with the solver's own huber_delta and epsilon (svnicp_set_particle_weighting_objective)
struct ParticleWeightOpt { bool use_weight_mean = false; double weight_dist = 0.0; double temperature = 0.0; std::string weight_cost = "point"; };

class SVGDICP {
 public:
  // init_pose: [6][P] row-major (x.., y.., z.., rx.., ry.., rz..) — the reference's [6,P,1] tensor
  SVGDICP(const SteinICPParam& p, const std::vector<double>& init_pose, int device = 0, int mode = SVNICP_MODE_SVGD)
      : P_((int)(init_pose.size() / 6)), I_(p.iterations) {
    svnicp_params q{};
    q.struct_size = (int32_t)sizeof q;
    q.mode = mode;
    q.iterations = p.iterations; q.knn_count = p.KNN_count; q.lr = p.lr; q.max_dist = p.max_dist;
    q.convergence_threshold = p.convergence_threshold; q.check_early_stop = p.check_early_stop;
    q.svn_full_grad = p.SVN_full_grad;
    q.optimizer = p.optimizer == "Adam" ? SVNICP_OPT_ADAM : p.optimizer == "RMSprop" ? SVNICP_OPT_RMSPROP
                : p.optimizer == "SGD" ? SVNICP_OPT_SGD : p.optimizer == "Adagrad" ? SVNICP_OPT_ADAGRAD : SVNICP_OPT_NONE;
    if (svnicp_create(&q, device, init_pose.data(), P_, &h_) != 0) throw std::runtime_error(svnicp_last_error(nullptr));
    if (p.use_minibatch) { batch_ = p.batch_size; chk(svnicp_set_minibatch(h_, p.batch_size, p.minibatch_seed)); }
    if (p.residual != "point") set_residual(p.residual, p.huber_delta, p.normal_k, p.gicp_epsilon);
  }
  virtual ~SVGDICP() { svnicp_destroy(h_); }
  SVGDICP(const SVGDICP&) = delete;
  SVGDICP& operator=(const SVGDICP&) = delete;

  // add_cloud(source[B,3], target[M,3], init_pose[6,P,1]) — SVGDICP.cpp:46-62
  void add_cloud(const double* source_xyz, int64_t B, const double* target_xyz, int64_t M, const double* init_pose6xP, int P) {
    chk(svnicp_set_clouds(h_, source_xyz, B, target_xyz, M, SVNICP_MEM_HOST));
    chk(svnicp_set_particles(h_, init_pose6xP, P));
    P_ = P;
  }
  // add_cloud with a host source scan and a target already in HBM (svnicp_map_query): only the source crosses PCIe
  void add_cloud_device_target(const double* source_xyz, int64_t B, const double* target_dev_xyz, int64_t M, const double* init_pose6xP, int P) {
    chk(svnicp_set_source(h_, source_xyz, B, SVNICP_MEM_HOST));
    chk(svnicp_set_target(h_, target_dev_xyz, M, SVNICP_MEM_DEVICE));
    chk(svnicp_synchronize(h_));
    chk(svnicp_set_particles(h_, init_pose6xP, P));
    P_ = P;
  }
  // add_cloud with both clouds already in HBM (float64 rows): two device-to-device copies
  void add_cloud_device(const double* source_dev_xyz, int64_t B, const double* target_dev_xyz, int64_t M, const double* init_pose6xP, int P) {
    chk(svnicp_set_source(h_, source_dev_xyz, B, SVNICP_MEM_DEVICE));
    chk(svnicp_set_target(h_, target_dev_xyz, M, SVNICP_MEM_DEVICE));
    chk(svnicp_synchronize(h_));
    chk(svnicp_set_particles(h_, init_pose6xP, P));
    P_ = P;
  }
  // set_initial_mean(gtsam::Pose3) — SVGDICP.h:102-110
  void set_initial_mean(const double R_rowmajor[9], const double t[3]) { chk(svnicp_set_initial_mean(h_, R_rowmajor, t)); }
  virtual SteinICPState stein_align() {  // SVNICP.cpp:41-114 / SVGDICP.cpp:66-140
    const int r = svnicp_align(h_);
    if (r < 0) fail();
    return (SteinICPState)r;
  }
  std::array<double, 6> get_transformation() { std::array<double, 6> o{}; chk(svnicp_get_transformation(h_, o.data())); return o; }
  std::array<double, 6> get_distribution() { std::array<double, 6> o{}; chk(svnicp_get_distribution(h_, o.data())); return o; }
  std::vector<double> get_cov_matrix() { std::vector<double> o(36); chk(svnicp_get_cov_matrix(h_, o.data())); return o; }
  std::vector<double> get_particles() { std::vector<double> o((size_t)6 * P_); chk(svnicp_get_particles(h_, o.data())); return o; }
  std::vector<double> get_particle_weight() { std::vector<double> o((size_t)P_); chk(svnicp_get_particle_weight(h_, o.data())); return o; }
  std::vector<std::vector<float>> get_particle_history() {
    std::vector<float> flat((size_t)I_ * 6 * P_);
    chk(svnicp_get_particle_history(h_, flat.data()));
    std::vector<std::vector<float>> o;
    for (int i = 0; i < I_; ++i) o.emplace_back(flat.begin() + (size_t)i * 6 * P_, flat.begin() + (size_t)(i + 1) * 6 * P_);
    return o;
  }
  std::vector<double> get_runtime() { std::vector<double> o(3); chk(svnicp_get_runtime(h_, o.data())); return o; }
  void set_k(int k) { chk(svnicp_set_k(h_, k)); }
  void set_threshold(double max_dist) { chk(svnicp_set_max_dist(h_, max_dist)); }
  // mini-batch (svnicp_hip.h "mini-batch"): rows per iteration from now on (0 = full batch), or an explicit table
  void set_minibatch(int batch_size, uint64_t seed = 0) { chk(svnicp_set_minibatch(h_, batch_size, seed)); batch_ = batch_size; }
  void set_minibatch_indices(const std::vector<int32_t>& table, int iterations, int batch_size) {
    if (table.size() != (size_t)iterations * (size_t)batch_size) throw std::runtime_error("set_minibatch_indices: table size");
    chk(svnicp_set_minibatch_indices(h_, table.data(), iterations, batch_size, SVNICP_MEM_HOST));
    batch_ = batch_size;
  }
  std::vector<int32_t> get_minibatch_indices() {   // [iterations][batch_size] of the last registration
    std::vector<int32_t> o((size_t)I_ * (size_t)(batch_ > 0 ? batch_ : 0));
    chk(svnicp_get_minibatch_indices(h_, o.data()));
    return o;
  }
  std::array<int64_t, 2> get_minibatch_rows() { std::array<int64_t, 2> o{}; chk(svnicp_get_minibatch_rows(h_, o.data())); return o; }
  // point-to-plane residual (svnicp_hip.h "point-to-plane residual")
  void set_residual(const std::string& residual, double huber_delta = 0.1, int normal_k = 16, double gicp_epsilon = 1e-3) {
    if (residual == "gicp") { chk(svnicp_set_residual_gicp(h_, huber_delta, normal_k, gicp_epsilon)); return; }   // svnicp_hip.h "generalized-ICP residual"
    if (residual != "point" && residual != "plane") throw std::runtime_error("set_residual: \"point\", \"plane\" or \"gicp\"");
    chk(svnicp_set_residual(h_, residual == "plane" ? SVNICP_RESIDUAL_PLANE : SVNICP_RESIDUAL_POINT, huber_delta, normal_k));
  }
  // normals of the current target, [M][3] in host memory; call after add_cloud
  void set_target_normals(const double* n_xyz, int64_t M) { chk(svnicp_set_target_normals(h_, n_xyz, M, SVNICP_MEM_HOST)); }
  // ... [M][3] float64 rows already in HBM (svnicp_map_normals_devptr): one device-to-device copy
  void set_target_normals_device(const double* n_dev_xyz, int64_t M) { chk(svnicp_set_target_normals(h_, n_dev_xyz, M, SVNICP_MEM_DEVICE)); }
  std::vector<double> get_target_normals(int64_t M) { std::vector<double> o((size_t)M * 3); chk(svnicp_get_target_normals(h_, o.data())); return o; }
  // {accepted pairs, sum w r^2} per particle of the last iteration run; *normal_passes = normal passes run so far
  std::vector<double> get_plane_stats(int64_t* normal_passes = nullptr) {
    std::vector<double> o((size_t)2 * P_);
    chk(svnicp_get_plane_stats(h_, o.data(), normal_passes));
    return o;
  }
  // generalized-ICP residual: normals of the current source, [B][3] in host memory; call after add_cloud
  void set_source_normals(const double* n_xyz, int64_t B) { chk(svnicp_set_source_normals(h_, n_xyz, B, SVNICP_MEM_HOST)); }
  std::vector<double> get_source_normals(int64_t B) { std::vector<double> o((size_t)B * 3); chk(svnicp_get_source_normals(h_, o.data())); return o; }
  // {accepted pairs, sum w rho^2} per particle of the last iteration run; passes2 = {target, source} normal passes run so far
  std::vector<double> get_gicp_stats(int64_t* passes2 = nullptr) {
    std::vector<double> o((size_t)2 * P_);
    chk(svnicp_get_gicp_stats(h_, o.data(), passes2));
    return o;
  }
  // Gaussian pose prior on the correction (svnicp_hip.h "pose prior"): mean6 = [t ; rotation vector], info36 = Lambda row-major
  // in the cost's units (sigma_pt^2 Sigma^-1); info36 == nullptr turns it off.  From the next registration on.
  void set_pose_prior(const double* mean6, const double* info36) { chk(svnicp_set_pose_prior(h_, mean6, info36)); }
  // true and mean6 / info36 filled (either may be nullptr) when a prior is set
  bool pose_prior(double* mean6 = nullptr, double* info36 = nullptr) {
    int on = 0;
    chk(svnicp_get_pose_prior(h_, &on, mean6, info36));
    return on != 0;
  }
  // evaluate a registration (svnicp_hip.h "evaluate a registration"): fitness, inlier RMSE and, with normals, plane RMSE of
  // a pose (row-major R, t; map <- sensor) against the whole target; both NULL: the last registration's result
  svnicp_eval evaluate(double max_corr_dist, const double* R_rowmajor = nullptr, const double* t = nullptr) {
    svnicp_eval e{};
    e.struct_size = (int32_t)sizeof e;
    chk(svnicp_evaluate(h_, R_rowmajor, t, max_corr_dist, &e));
    return e;
  }
  // per source row of the last evaluate: nearest target row (-1 = not evaluated) and its d2 (NaN = not evaluated)
  void get_eval_pairs(std::vector<int32_t>* idx, std::vector<double>* d2, int64_t B) {
    if (idx) idx->assign((size_t)B, -1);
    if (d2) d2->assign((size_t)B, 0.0);
    chk(svnicp_get_eval_pairs(h_, idx ? idx->data() : nullptr, d2 ? d2->data() : nullptr));
  }
  // information matrix of a registration (svnicp_hip.h): the Gauss-Newton normal equations H, b over the pairs of the last
  // evaluate, tangent T * Exp([v ; omega]), with their eigen-structure, rank, step -H+ b and covariance; form = SVNICP_INFO_POINT
  // or SVNICP_INFO_PLANE, independent of the residual the solver ran; huber_delta = +inf: unweighted
  svnicp_information information(int form = SVNICP_INFO_PLANE, double huber_delta = HUGE_VAL, double eig_floor_ratio = 0.0) {
    svnicp_information o{};
    o.struct_size = (int32_t)sizeof o;
    chk(svnicp_eval_information(h_, form, huber_delta, eig_floor_ratio, &o));
    return o;
  }
  // the same in the generalized-ICP objective (svnicp_eval_information_gicp): needs normals of both clouds in the context;
  // gicp_epsilon = 0: 1e-3
  svnicp_information information_gicp(double huber_delta = HUGE_VAL, double gicp_epsilon = 0.0, double eig_floor_ratio = 0.0) {
    svnicp_information o{};
    o.struct_size = (int32_t)sizeof o;
    chk(svnicp_eval_information_gicp(h_, huber_delta, gicp_epsilon, eig_floor_ratio, &o));
    return o;
  }
  // svnicp_information_solve without the library: every derived field from io.form, pairs, sum_wr2, eig_floor_ratio, H and b
  // (for instance the sums of several row-sharded contexts added up)
  static void information_solve(svnicp_information& io) {
    const char* why = nullptr;
    io.struct_size = (int32_t)sizeof io;
    if (svnicp_info::solve(&io, &why) != 0) throw std::runtime_error(std::string("svnicp_information_solve: ") + (why ? why : "invalid input"));
  }
  // score and weight the particles (svnicp_hip.h): [P][SVNICP_SCORE_FIELDS] {evaluated, inliers, plane inliers, sum d2, sum r2,
  // cost} of every particle's final pose through the registration's candidate table; poses: [P][12] (R row-major, t), optional
  std::vector<double> score_particles(double max_corr_dist, std::vector<double>* poses = nullptr) {
    std::vector<double> o((size_t)P_ * SVNICP_SCORE_FIELDS);
    if (poses) poses->assign((size_t)P_ * 12, 0.0);
    chk(svnicp_score_particles(h_, max_corr_dist, o.data(), poses ? poses->data() : nullptr));
    return o;
  }
  std::vector<double> get_particle_scores(std::vector<double>* poses = nullptr) {   // the last scoring, whoever ran it
    std::vector<double> o((size_t)P_ * SVNICP_SCORE_FIELDS);
    if (poses) poses->assign((size_t)P_ * 12, 0.0);
    chk(svnicp_get_particle_scores(h_, o.data(), poses ? poses->data() : nullptr));
    return o;
  }
  void set_particle_weighting(int kind, double max_corr_dist = 0.0, double temperature = 0.0) {
    chk(svnicp_set_particle_weighting(h_, kind, max_corr_dist, temperature));
  }
  // … in the objective the solver minimised (svnicp_hip.h): form SVNICP_SCORE_*; huber_delta / epsilon 0: the solver's own.
  // The block is {evaluated, inliers, accepted, sum d2, sum h, cost} in the forms PLANE and GICP
  static svnicp_score_objective score_objective(int form, double max_corr_dist, double huber_delta = 0.0, double epsilon = 0.0) {
    svnicp_score_objective o{};
    o.struct_size = sizeof o; o.form = form; o.max_corr_dist = max_corr_dist; o.huber_delta = huber_delta; o.epsilon = epsilon;
    return o;
  }
  std::vector<double> score_particles_objective(const svnicp_score_objective& obj, std::vector<double>* poses = nullptr) {
    std::vector<double> o((size_t)P_ * SVNICP_SCORE_FIELDS);
    if (poses) poses->assign((size_t)P_ * 12, 0.0);
    chk(svnicp_score_particles_objective(h_, &obj, o.data(), poses ? poses->data() : nullptr));
    return o;
  }
  void set_particle_weighting_objective(int kind, const svnicp_score_objective& obj, double temperature) {
    chk(svnicp_set_particle_weighting_objective(h_, kind, &obj, temperature));
  }
  svnicp_score_objective get_score_objective() {   // the resolved objective of the last scoring
    svnicp_score_objective o{};
    o.struct_size = sizeof o;
    chk(svnicp_get_score_objective(h_, &o));
    return o;
  }
  // particle modes (svnicp_hip.h "particle modes"): the connected components of the particles' link graph, heaviest first, with
  // mass, mean, covariance, total pose and best-scored member.  particles6xP == nullptr: the last registration's set with its
  // weights; else a host [6][P] block of the caller's (no registration needed) with weightsP [P] or equal weights
  svnicp_modes particle_modes(double link_trans, double link_rot, int max_modes = 8, const double* particles6xP = nullptr, int P = 0,
                              const double* weightsP = nullptr) {
    svnicp_modes_opt opt{};
    opt.struct_size = (int32_t)sizeof opt; opt.max_modes = max_modes; opt.link_trans = link_trans; opt.link_rot = link_rot;
    opt.particles6xP = particles6xP; opt.P = P; opt.weightsP = weightsP;
    svnicp_modes o{};
    o.struct_size = (int32_t)sizeof o;
    chk(svnicp_particle_modes(h_, &opt, &o));
    modes_P_ = o.particles;
    return o;
  }
  // per particle of the last particle_modes: the rank of its mode (0 = the heaviest), -1 for a non-finite particle
  std::vector<int32_t> get_mode_labels() {
    std::vector<int32_t> o((size_t)(modes_P_ > 0 ? modes_P_ : 1), -1);
    chk(svnicp_get_mode_labels(h_, o.data()));
    o.resize((size_t)modes_P_);
    return o;
  }
  const int32_t* eval_index_ptr() { return svnicp_eval_index_devptr(h_); }
  const double* eval_dist2_ptr() { return svnicp_eval_dist2_devptr(h_); }
  svnicp_ctx* handle() { return h_; }

 protected:
  void chk(int rc) { if (rc != 0) fail(); }
  [[noreturn]] void fail() { throw std::runtime_error(svnicp_last_error(h_)); }
  svnicp_ctx* h_ = nullptr;
  int P_, I_;
  int batch_ = 0;
  int modes_P_ = 0;
};

class SVNICP final : public SVGDICP {
 public:
  SVNICP(const SteinICPParam& p, const std::vector<double>& init_pose, const ParticleWeightOpt& w = {}, int device = 0)
      : SVGDICP(p, init_pose, device, SVNICP_MODE_SVN) {
    if (!(w.use_weight_mean && w.weight_dist > 0)) return;
    if (w.weight_cost == "point") set_particle_weighting(SVNICP_WEIGHT_SOFTMIN, w.weight_dist, w.temperature);
    else if (w.weight_cost == "solved") set_particle_weighting_objective(SVNICP_WEIGHT_SOFTMIN, score_objective(SVNICP_SCORE_AS_SOLVED, w.weight_dist), w.temperature);
    else throw std::invalid_argument("ParticleWeightOpt: weight_cost must be \"point\" or \"solved\"");
  }
};

}  // namespace svnicp
