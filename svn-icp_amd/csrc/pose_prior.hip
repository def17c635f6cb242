// pose_prior.hip — the Gaussian pose prior on the correction (svnicp_set_pose_prior): ONE launch in front of
// the Stein step of an iteration.  Per particle p, with (R_p, t_p) the correction pose this iteration's search used:
//   base record   particle_Hb of the chain's own UpdateArgs (stein_step_device.hpp): the plane record where plane mode left
//                 one, else load_sums + finalize_Hb — the 1e-6·I and every rounding of the step without a prior
//   e = [t_p − μ_t ; Log(R_μᵀ R_p)]        J = blkdiag(R_p, Jr⁻¹(e_r)),  Jr⁻¹(ω) = I + ½[ω]× + c(θ)[ω]×²
//   b ← b + Jᵀ(Λe)        H ← H + JᵀΛJ (computed for i ≤ j and mirrored)
// and the sum goes to a SEPARATE [P][42] record that UpdateArgs::plane_Hb of the Stein-step kernels then points at: the base
// record is never changed, so svnicp_iter_update may run again on it.  A particle whose R_p or t_p holds a non-finite entry
// gets a record of NaN; the others do not depend on it.  Every sum below runs over ascending index, left to right, no fma
// (-ffp-contract=off): tests/pose_prior_reference.py restates it operation by operation.
#include "kernels.hpp"
#include "pose_prior.hpp"
#include "stein_step_device.hpp"

namespace svnicp {
namespace {

constexpr int PT = 64;   // one particle per lane, one wave per workgroup

// c(θ) of Jr⁻¹ from θ² = |ω|²: 1/θ² − (1 + cos θ)/(2 θ sin θ); below kSeriesTheta the series 1/12 + θ²/720 + θ⁴/30240, whose
// first dropped term θ⁶/1209600 is under 1e-18 there, while the closed form's cancellation costs about 2⁻⁵³/θ² (1e-12 at the
// threshold, times the [ω]×² ~ θ² it multiplies: 1e-16 of an entry of Jr⁻¹)
constexpr double kSeriesTheta = 1e-2;
__device__ __forceinline__ double jr_inv_c(double th2) {
  const double th = sqrt(th2);
  if (th < kSeriesTheta) return (1.0 / 12.0 + th2 / 720.0) + (th2 * th2) / 30240.0;
  return 1.0 / th2 - (1.0 + cos(th)) / ((2.0 * th) * sin(th));
}

__global__ __launch_bounds__(PT) void k_pose_prior(UpdateArgs a, PosePrior pr, double* __restrict__ out) {
  const int p = blockIdx.x * PT + threadIdx.x;
  if (p >= a.P) return;
  double H[36], b[6];
  particle_Hb(a, p, H, b);
  double Rp[9], e[6];
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) { Rp[i] = a.R[9 * p + i]; finite = finite && isfinite(Rp[i]); }
#pragma unroll
  for (int i = 0; i < 3; ++i) { const double t = a.t[3 * p + i]; finite = finite && isfinite(t); e[i] = t - pr.mu_t[i]; }
  double* rec = out + (size_t)p * 42;
  if (!finite) {
#pragma unroll
    for (int i = 0; i < 42; ++i) rec[i] = __builtin_nan("");
    return;
  }
  // E = R_μᵀ R_p, e_r = Log E
  double E[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) E[3 * i + j] = pr.Rmu[i] * Rp[j] + pr.Rmu[3 + i] * Rp[3 + j] + pr.Rmu[6 + i] * Rp[6 + j];
  so3_log(E, e + 3);
  const double w0 = e[3], w1 = e[4], w2 = e[5];
  const double c = jr_inv_c((w0 * w0 + w1 * w1) + w2 * w2);
  const double W[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
  double W2[9], Jr[9];
  mat3_mul(W, W, W2);
#pragma unroll
  for (int i = 0; i < 9; ++i) Jr[i] = ((i % 4 == 0 ? 1.0 : 0.0) + 0.5 * W[i]) + c * W2[i];
  // J[m][j], m, j in 0..5: rows 0..2 hold R_p in columns 0..2, rows 3..5 hold Jr⁻¹ in columns 3..5
  // v = Λe, then b += Jᵀv
  double v[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double s = pr.L[6 * k] * e[0];
#pragma unroll
    for (int m = 1; m < 6; ++m) s += pr.L[6 * k + m] * e[m];
    v[k] = s;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    b[j] += (Rp[j] * v[0] + Rp[3 + j] * v[1]) + Rp[6 + j] * v[2];
    b[3 + j] += (Jr[j] * v[3] + Jr[3 + j] * v[4]) + Jr[6 + j] * v[5];
  }
  // A = ΛJ: A[k][j] = Σ_m Λ[k][m] J[m][j] over the three rows m of J's block that holds column j
  double A[36];
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      A[6 * k + j] = (pr.L[6 * k] * Rp[j] + pr.L[6 * k + 1] * Rp[3 + j]) + pr.L[6 * k + 2] * Rp[6 + j];
      A[6 * k + 3 + j] = (pr.L[6 * k + 3] * Jr[j] + pr.L[6 * k + 4] * Jr[3 + j]) + pr.L[6 * k + 5] * Jr[6 + j];
    }
  // G = JᵀA for i ≤ j: G[i][j] = Σ_k J[k][i] A[k][j] over the three rows k of the block that holds column i; mirrored
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) {
      const double* Jb = i < 3 ? Rp : Jr;
      const int ci = i < 3 ? i : i - 3, k0 = i < 3 ? 0 : 3;
      const double g = (Jb[ci] * A[6 * k0 + j] + Jb[3 + ci] * A[6 * (k0 + 1) + j]) + Jb[6 + ci] * A[6 * (k0 + 2) + j];
      H[6 * i + j] += g;
      if (j != i) H[6 * j + i] += g;
    }
#pragma unroll
  for (int i = 0; i < 36; ++i) rec[i] = H[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) rec[36 + i] = b[i];
}

}  // namespace

hipError_t launch_pose_prior(const UpdateArgs& a, const PosePrior& pr, double* record, hipStream_t st) {
  if (a.P <= 0 || !record) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pose_prior, dim3((unsigned)((a.P + PT - 1) / PT)), dim3(PT), 0, st, a, pr, record);
  return hipGetLastError();
}

}  // namespace svnicp
