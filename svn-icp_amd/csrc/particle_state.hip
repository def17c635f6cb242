// particle_state.hip — the particle set outside the Stein step: its initial state at the start of a registration
// (k_init_particles) and the statistics read back at the end (k_stats).
#include "kernels.hpp"

namespace svnicp {

namespace {

// constructor / add_cloud: R = Exp(r), t, total pose (SVNICP.cpp:20-38, SVGDICP.cpp:46-62)
__global__ void k_init_particles(const double* __restrict__ init, int P, Pose0 pose, int mode, double* R, double* t,
                                 double* Rtot, double* pose_out, int refresh_pose, double* eul, BeginZero z) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  // start of a registration (svnicp_align_begin): the control words and the small areas that must start at zero, in this
  // launch instead of five fill / copy launches of their own (each one costs a small registration 5-8 us)
  for (int a = 0; a < z.n; ++a)
    for (unsigned int e = (unsigned int)p; e < z.dwords[a]; e += gridDim.x * blockDim.x) z.ptr[a][e] = 0u;
  for (unsigned int e = (unsigned int)p; e < z.ones_dwords; e += gridDim.x * blockDim.x) z.ones[e] = 0xffffffffu;
  if (z.ctl && p == 0) { z.ctl[0] = 0; z.ctl[1] = z.iterations; z.ctl[2] = 0; z.ctl[3] = 0; }   // stop flag, finish_iter (SVGDICP.cpp:42)
  if (p >= P) return;
  double r[3] = {0, 0, 0}, tv[3], Rm[9];
  if (mode == 2) {  // keep the current R_, t_: only the total pose is recomputed
    for (int i = 0; i < 9; ++i) Rm[i] = R[9 * p + i];
    for (int i = 0; i < 3; ++i) tv[i] = t[3 * p + i];
  } else {
    r[0] = init[3 * P + p]; r[1] = init[4 * P + p]; r[2] = init[5 * P + p];
    tv[0] = init[p]; tv[1] = init[P + p]; tv[2] = init[2 * P + p];
    if (mode == 0) so3_exp(r, Rm, nullptr); else euler_to_R(r[0], r[1], r[2], Rm);
    if (mode == 1 && eul) {  // SVGD: the optimizer parameters are the pose entries themselves (SVGDICP.cpp:46-53)
      for (int i = 0; i < 3; ++i) { eul[6 * p + i] = tv[i]; eul[6 * p + 3 + i] = r[i]; }
    }
  }
  double Rt[9], tt[3];
  mat3_mul(pose.R0, Rm, Rt);
  mat3_vec(pose.R0, tv, tt);
  for (int i = 0; i < 9; ++i) { R[9 * p + i] = Rm[i]; Rtot[12 * p + i] = Rt[i]; }
  for (int i = 0; i < 3; ++i) { t[3 * p + i] = tv[i]; Rtot[12 * p + 9 + i] = pose.t0[i] + tt[i]; }
  if (refresh_pose) {
    double lg[3];
    if (mode == 0) so3_log(Rm, lg); else { lg[0] = r[0]; lg[1] = r[1]; lg[2] = r[2]; }
    for (int i = 0; i < 3; ++i) { pose_out[i * P + p] = tv[i]; pose_out[(3 + i) * P + p] = lg[i]; }
  }
}

// get_transformation / get_distribution / get_cov_matrix / get_particle_weight
// (SVNICP.cpp:281-308; SVGDICP.cpp:497-524).  out = mean[6] var[6] cov[36] weights[P]
__global__ void k_stats(StatsArgs a) {
  const int tid = threadIdx.x;
  const int P = a.P;
  __shared__ double mean[6];
  // the sums below run over the particles in order, one thread per output: from LDS (a coalesced copy first) instead of
  // 3 x P dependent global loads (48 -> 9 us at 128 particles); same order of additions, same bits
  constexpr int kStage = 1024;
  __shared__ double sp[6 * kStage];
  const bool staged = P <= kStage;
  if (staged) for (int e = tid; e < 6 * P; e += blockDim.x) sp[e] = a.pose[e];
  __syncthreads();
  const double* pose = staged ? sp : a.pose;
  // SVNICP.cpp:46: torch::ones({P,1}) / P is float32, promoted to f64 in the products
  const double wsvn = (double)(1.0f / (float)P);
  if (tid < 6) {
    double s = 0.0;
    if (a.mode == 0) { for (int p = 0; p < P; ++p) s += pose[tid * P + p] * wsvn; }
    else { for (int p = 0; p < P; ++p) s += pose[tid * P + p]; s /= P; }
    mean[tid] = s;
    a.out[tid] = s;
  }
  __syncthreads();
  if (tid < 6) {
    double s = 0.0;
    if (a.mode == 0) { for (int p = 0; p < P; ++p) { const double d = pose[tid * P + p] - mean[tid]; s += d * d * wsvn; } }
    else { for (int p = 0; p < P; ++p) { const double d = pose[tid * P + p] - mean[tid]; s += d * d; } s /= (P - 1); }
    a.out[6 + tid] = s;
  }
  if (tid < 36) {
    const int r = tid / 6, c = tid % 6;
    double s = 0.0;
    const double wgt = a.mode == 0 ? wsvn : 1.0;
    for (int p = 0; p < P; ++p) s += wgt * ((pose[r * P + p] - mean[r]) * (pose[c * P + p] - mean[c]));
    a.out[12 + tid] = a.mode == 0 ? s : s / P;
  }
  for (int p = tid; p < P; p += blockDim.x) a.out[48 + p] = a.mode == 0 ? wsvn : 1.0;
}

// the same block with weights w[P] (svnicp_set_particle_weighting; SVN mode): the reference's getters as written for arbitrary
// weights (SVNICP.cpp:286-308) — mean_i = sum x_ip w_p, var_i = sum (x_ip - mean_i)^2 w_p, cov_rc = sum w_p (x_rp - mean_r)
// (x_cp - mean_c), every sum in particle order.  A kernel of its own: k_stats, the uniform path, stays as it is bit for bit.
__global__ void k_stats_weighted(StatsArgs a, const double* __restrict__ w) {
  const int tid = threadIdx.x;
  const int P = a.P;
  __shared__ double mean[6];
  constexpr int kStage = 896;   // 7 x 896 doubles: 49 KB of LDS
  __shared__ double sp[7 * kStage];
  const bool staged = P <= kStage;
  if (staged) {
    for (int e = tid; e < 6 * P; e += blockDim.x) sp[e] = a.pose[e];
    for (int e = tid; e < P; e += blockDim.x) sp[6 * P + e] = w[e];
  }
  __syncthreads();
  const double* pose = staged ? sp : a.pose;
  const double* wp = staged ? sp + 6 * P : w;
  if (tid < 6) {
    double s = 0.0;
    for (int p = 0; p < P; ++p) s += pose[tid * P + p] * wp[p];
    mean[tid] = s;
    a.out[tid] = s;
  }
  __syncthreads();
  if (tid < 6) {
    double s = 0.0;
    for (int p = 0; p < P; ++p) { const double d = pose[tid * P + p] - mean[tid]; s += d * d * wp[p]; }
    a.out[6 + tid] = s;
  }
  if (tid < 36) {
    const int r = tid / 6, c = tid % 6;
    double s = 0.0;
    for (int p = 0; p < P; ++p) s += wp[p] * ((pose[r * P + p] - mean[r]) * (pose[c * P + p] - mean[c]));
    a.out[12 + tid] = s;
  }
  for (int p = tid; p < P; p += blockDim.x) a.out[48 + p] = wp[p];
}

}  // namespace

hipError_t launch_init_particles(const double* init6xP, int P, const Pose0& pose, int mode, double* R, double* t,
                                 double* Rtot, double* pose_out, int refresh_pose, double* eul, hipStream_t st, const BeginZero* zero) {
  BeginZero z{};
  if (zero) z = *zero;
  unsigned int most = 0;
  for (int a = 0; a < z.n; ++a) most = z.dwords[a] > most ? z.dwords[a] : most;
  int blocks = (P + 127) / 128;
  const int for_zero = (int)((most + 128u * 32u - 1u) / (128u * 32u));   // about 32 words per thread
  if (for_zero > blocks) blocks = for_zero > 256 ? 256 : for_zero;
  hipLaunchKernelGGL(k_init_particles, dim3(blocks), dim3(128), 0, st, init6xP, P, pose, mode, R, t, Rtot,
                     pose_out, refresh_pose, eul, z);
  return hipGetLastError();
}

hipError_t launch_stats(const StatsArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_stats, dim3(1), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_stats_weighted(const StatsArgs& a, const double* w, hipStream_t st) {
  hipLaunchKernelGGL(k_stats_weighted, dim3(1), dim3(256), 0, st, a, w);
  return hipGetLastError();
}

}  // namespace svnicp
