// information_solve.hpp — the host half of svnicp_eval_information (include/svnicp_hip.h "information matrix of a
// registration"): everything svnicp_information_solve derives from {form, pairs, sum_wr2, eig_floor_ratio,
// H, b}.  Plain C++17, no HIP: api.hip and the C++ shim (host/svnicp_hip_shim.hpp) both include it, and tests compile it alone.
//   eigen-structure   cyclic Jacobi in float64, kSweeps sweeps, on (H + H^T) / 2 and on its two diagonal 3x3 blocks; the
//                     matrix is first scaled by a power of two (exact) so that its largest entry lies in [1, 2): no product
//                     of two entries can overflow or underflow, whatever the units of H
//   order and sign    eigenvalues ascending (equal ones keep Jacobi's column order); every eigenvector has unit length and its
//                     largest-magnitude component positive, the lowest index deciding a tie
//   rank, H+          rank = #{lambda_i > f * lambda_max}; H+ = sum over those of v v^T / lambda
// plane_normal_device.hpp keeps its own 3x3 Jacobi: its results are pinned bit for bit by the plane tests.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/svnicp_hip.h"

namespace svnicp_info {

constexpr int kSweeps = 12;                  // a 6x6 matrix is diagonal to rounding after 6 to 7; the count is fixed so that
                                             // the same input always runs the same rotations
constexpr double kDefaultFloor = 1e-12;      // eig_floor_ratio = 0 (svnicp_hip.h states the reasoning)

// A [N][N] symmetric, row-major, destroyed.  val[N] ascending, vec[N][N]: row i = unit eigenvector i.
template <int N>
inline void jacobi_eigen(double* A, double* val, double* vec) {
  double V[N][N];
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  double big = 0.0;
  for (int i = 0; i < N * N; ++i) big = std::fabs(A[i]) > big ? std::fabs(A[i]) : big;
  int ex = 0;
  if (big > 0.0) {
    (void)std::frexp(big, &ex);
    ex -= 1;                                 // big * 2^-ex in [1, 2)
    for (int i = 0; i < N * N; ++i) A[i] = std::ldexp(A[i], -ex);
  }
  const double tiny = std::ldexp(1.0, -80);  // an off-diagonal entry below this (largest entry ~1) rotates nothing representable
  for (int sweep = 0; sweep < kSweeps; ++sweep)
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        const double apq = A[p * N + q];
        if (!(std::fabs(apq) > tiny)) { A[p * N + q] = A[q * N + p] = 0.0; continue; }
        const double theta = (A[q * N + q] - A[p * N + p]) / (2.0 * apq);
        // the smaller root of t^2 + 2 theta t - 1 = 0; |theta| beyond 2^500 rounds to t = 1 / (2 theta) without squaring
        const double at = std::fabs(theta);
        const double t = (at > 0x1p500 ? 0.5 / at : 1.0 / (at + std::sqrt(at * at + 1.0))) * (theta < 0.0 ? -1.0 : 1.0);
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        A[p * N + p] -= t * apq;
        A[q * N + q] += t * apq;
        A[p * N + q] = A[q * N + p] = 0.0;
        for (int k = 0; k < N; ++k) {
          if (k == p || k == q) continue;
          const double akp = A[k * N + p], akq = A[k * N + q];
          A[k * N + p] = A[p * N + k] = c * akp - s * akq;
          A[k * N + q] = A[q * N + k] = s * akp + c * akq;
        }
        for (int k = 0; k < N; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  int order[N];
  for (int i = 0; i < N; ++i) order[i] = i;
  for (int i = 1; i < N; ++i)                // insertion sort: stable, equal eigenvalues keep their column order
    for (int j = i; j > 0 && A[order[j] * N + order[j]] < A[order[j - 1] * N + order[j - 1]]; --j) {
      const int tmp = order[j]; order[j] = order[j - 1]; order[j - 1] = tmp;
    }
  for (int i = 0; i < N; ++i) {
    const int col = order[i];
    val[i] = big > 0.0 ? std::ldexp(A[col * N + col], ex) : 0.0;
    double nrm2 = 0.0;
    for (int k = 0; k < N; ++k) nrm2 += V[k][col] * V[k][col];
    const double inv = 1.0 / std::sqrt(nrm2);   // the product of rotations is orthogonal to a few ulp; make the length exact to one
    int lead = 0;
    for (int k = 1; k < N; ++k)
      if (std::fabs(V[k][col]) > std::fabs(V[lead][col])) lead = k;
    const double sign = V[lead][col] < 0.0 ? -inv : inv;
    for (int k = 0; k < N; ++k) vec[i * N + k] = V[k][col] * sign;
  }
}

// every field svnicp_information_solve derives; 0 or SVNICP_ERR_INVALID with *why naming the reason
inline int solve(svnicp_information* io, const char** why) {
  const char* dummy = nullptr;
  const char*& reason = why ? *why : dummy;
  reason = nullptr;
  if (!io) { reason = "null struct"; return SVNICP_ERR_INVALID; }
  if (io->struct_size != (int32_t)sizeof(svnicp_information)) { reason = "svnicp_information.struct_size mismatch"; return SVNICP_ERR_INVALID; }
  if (io->form != SVNICP_INFO_POINT && io->form != SVNICP_INFO_PLANE && io->form != SVNICP_INFO_GICP) {
    reason = "unknown form (SVNICP_INFO_POINT, SVNICP_INFO_PLANE or SVNICP_INFO_GICP)"; return SVNICP_ERR_INVALID;
  }
  if (!(io->eig_floor_ratio >= 0.0 && io->eig_floor_ratio < 1.0)) { reason = "eig_floor_ratio must lie in [0, 1)"; return SVNICP_ERR_INVALID; }
  if (io->pairs < 0) { reason = "pairs is negative"; return SVNICP_ERR_INVALID; }
  bool finite = std::isfinite(io->sum_wr2);
  for (int i = 0; i < 36; ++i) finite = finite && std::isfinite(io->H[i]);
  for (int i = 0; i < 6; ++i) finite = finite && std::isfinite(io->b[i]);
  if (!finite) { reason = "H, b or sum_wr2 holds a non-finite entry"; return SVNICP_ERR_INVALID; }

  double S[36], A6[36], A3[9];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) S[6 * i + j] = 0.5 * io->H[6 * i + j] + 0.5 * io->H[6 * j + i];   // halves first: no overflow
  for (int i = 0; i < 36; ++i) A6[i] = S[i];
  jacobi_eigen<6>(A6, io->eigval, io->eigvec);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A3[3 * i + j] = S[6 * i + j];
  jacobi_eigen<3>(A3, io->eig_t, io->vec_t);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A3[3 * i + j] = S[6 * (i + 3) + j + 3];
  jacobi_eigen<3>(A3, io->eig_r, io->vec_r);

  const double f = io->eig_floor_ratio == 0.0 ? kDefaultFloor : io->eig_floor_ratio;
  const double top = io->eigval[5], cut = f * top;
  int rank = 0;
  for (int i = 0; i < 6; ++i) rank += (top > 0.0 && io->eigval[i] > cut) ? 1 : 0;
  io->rank = rank;
  double pinv[36];
  for (int i = 0; i < 36; ++i) pinv[i] = 0.0;
  for (int i = 0; i < 6; ++i) io->step[i] = 0.0;
  for (int e = 6 - rank; e < 6; ++e) {       // ascending eigenvalues: the smallest retained term first
    const double* v = io->eigvec + 6 * e;
    const double inv = 1.0 / io->eigval[e];
    double vb = 0.0;
    for (int k = 0; k < 6; ++k) vb += v[k] * io->b[k];
    for (int i = 0; i < 6; ++i) {
      io->step[i] -= v[i] * (vb * inv);
      for (int j = 0; j < 6; ++j) pinv[6 * i + j] += (v[i] * v[j]) * inv;
    }
  }
  const int64_t dof = (io->form == SVNICP_INFO_PLANE ? 1 : 3) * io->pairs - rank;   // the GICP form's rho is a 3-vector's whitened norm
  io->sigma2 = dof > 0 ? io->sum_wr2 / (double)dof : 0.0;
  for (int i = 0; i < 36; ++i) io->cov[i] = io->sigma2 * pinv[i];
  return SVNICP_OK;
}

}  // namespace svnicp_info
