// pose_prior.hpp — the host half of the Gaussian pose prior (include/svnicp_hip.h "pose prior"): what
// svnicp_set_pose_prior checks and stores, and the block the kernel of pose_prior.hip takes by value.  Plain C++17, no HIP:
// api.hip and the C++ shim's tests include it, and tests/pose_prior_driver.cpp compiles it alone.
//   mean6    [t ; rotation vector] of the CORRECTION pose, the coordinates of svnicp_get_transformation; |mu_r| < pi
//   info36   the information matrix Lambda, row-major, order (t, r) as in svnicp_get_cov_matrix; symmetric to
//            1e-12 max|Lambda|, no negative diagonal entry, smallest eigenvalue not below -1e-12 max|Lambda| (cyclic Jacobi of
//            information_solve.hpp).  Stored symmetrised, (Lambda + Lambda^T) / 2 with the halves taken first.
// Lambda is in the units of the registration's cost, 1/2 sum w |e|^2, which carries no point noise: for a metric prior
// covariance Sigma and a point noise sigma_pt the caller passes Lambda = sigma_pt^2 Sigma^-1.
#pragma once
#include <cmath>

#include "information_solve.hpp"

namespace svnicp {

// kernel argument of k_pose_prior: R_mu = Exp(mu_r) row-major, mu_t, Lambda (symmetric)
struct PosePrior { double Rmu[9]; double mu_t[3]; double L[36]; };

namespace pose_prior {

constexpr double kSymTol = 1e-12;   // asymmetry and negative eigenvalue allowed, times max|Lambda|
constexpr double kPi = 3.14159265358979323846;

// Rodrigues: R = I + sin(a)/a K + (1 - cos a)/a^2 K^2; below 1e-12 rad exactly I (the guard of the device's so3_exp)
inline void exp_so3(const double* r, double* R) {
  const double a = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (a < 1e-12) { for (int i = 0; i < 9; ++i) R[i] = I3[i]; return; }
  const double K[9] = {0, -r[2], r[1], r[2], 0, -r[0], -r[1], r[0], 0};
  const double s = std::sin(a) / a, h = std::sin(0.5 * a) / a, c = 2.0 * h * h;   // (1 - cos a) / a^2 without cancellation
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double kk = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
      R[3 * i + j] = (I3[3 * i + j] + s * K[3 * i + j]) + c * kk;
    }
}

// 0 and *out filled, or SVNICP_ERR_INVALID with *why naming the reason (out untouched)
inline int validate(const double* mean6, const double* info36, PosePrior* out, const char** why) {
  const char* dummy = nullptr;
  const char*& reason = why ? *why : dummy;
  reason = nullptr;
  if (!mean6 || !info36 || !out) { reason = "null argument"; return SVNICP_ERR_INVALID; }
  double big = 0.0;
  for (int i = 0; i < 6; ++i)
    if (!std::isfinite(mean6[i])) { reason = "the mean holds a non-finite entry"; return SVNICP_ERR_INVALID; }
  for (int i = 0; i < 36; ++i) {
    if (!std::isfinite(info36[i])) { reason = "the information matrix holds a non-finite entry"; return SVNICP_ERR_INVALID; }
    big = std::fabs(info36[i]) > big ? std::fabs(info36[i]) : big;
  }
  const double tol = kSymTol * big;
  for (int i = 0; i < 6; ++i)
    for (int j = i + 1; j < 6; ++j)
      if (std::fabs(info36[6 * i + j] - info36[6 * j + i]) > tol) { reason = "the information matrix is not symmetric"; return SVNICP_ERR_INVALID; }
  for (int i = 0; i < 6; ++i)
    if (info36[7 * i] < 0.0) { reason = "the information matrix has a negative diagonal entry"; return SVNICP_ERR_INVALID; }
  if (!(std::sqrt(mean6[3] * mean6[3] + mean6[4] * mean6[4] + mean6[5] * mean6[5]) < kPi)) {
    reason = "the mean's rotation vector is not shorter than pi"; return SVNICP_ERR_INVALID;
  }
  double S[36], A[36], val[6], vec[36];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) S[6 * i + j] = 0.5 * info36[6 * i + j] + 0.5 * info36[6 * j + i];   // halves first: no overflow
  for (int i = 0; i < 36; ++i) A[i] = S[i];
  svnicp_info::jacobi_eigen<6>(A, val, vec);
  if (val[0] < -tol) { reason = "the information matrix has a negative eigenvalue"; return SVNICP_ERR_INVALID; }
  exp_so3(mean6 + 3, out->Rmu);
  for (int i = 0; i < 3; ++i) out->mu_t[i] = mean6[i];
  for (int i = 0; i < 36; ++i) out->L[i] = S[i];
  return SVNICP_OK;
}

}  // namespace pose_prior
}  // namespace svnicp
