// plane_normal_device.hpp — from a neighbourhood's scatter matrix to its normal: cyclic Jacobi with a fixed
// number of sweeps, normal = unit eigenvector of the smallest eigenvalue, and the validity rule.  Stated once for
// k_target_normals (plane_icp.hip: neighbours from stage A) and k_map_normals (map_normals.hip: neighbours from the 27-voxel
// block of the map); the two kernels differ only in where the neighbours come from and in the order of their sums.
//
// The header stands alone and also compiles for the host (tests/plane_normal_driver.cpp runs normal_from_scatter under the
// address and undefined-behaviour sanitizers): device functions under hipcc, plain inline functions elsewhere.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define SVNICP_NORMAL_FN __device__ __forceinline__
#else
#define SVNICP_NORMAL_FN inline
#endif

namespace svnicp {

constexpr double kPlaneMinRatio = 0.01;   // a normal is valid iff λ1 >= kPlaneMinRatio · λ2 (collinear neighbourhoods have none)
constexpr int kJacobiSweeps = 8;   // cyclic Jacobi on a symmetric 3x3 converges quadratically: 4-5 sweeps reach f64 round-off

// one Jacobi rotation of the (P, Q) plane; R is the remaining index.  A = [a00 a11 a22 a01 a02 a12], V row-major.
template <int P, int Q, int R>
SVNICP_NORMAL_FN void jacobi_rot(double* d, double& apq, double& apr, double& aqr, double* V) {
  if (apq == 0.0) return;
  const double theta = (d[Q] - d[P]) / (2.0 * apq);
  const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));   // |theta| huge: t = 0
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  d[P] -= t * apq;
  d[Q] += t * apq;
  apq = 0.0;
  const double rp = apr, rq = aqr;
  apr = c * rp - s * rq;
  aqr = s * rp + c * rq;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 3; ++i) {
    const double vp = V[3 * i + P], vq = V[3 * i + Q];
    V[3 * i + P] = c * vp - s * vq;
    V[3 * i + Q] = s * vp + c * vq;
  }
}

// scatter matrix Σ (d − mean)(d − mean)ᵀ = [d0 d1 d2 | a01 a02 a12] -> unit normal n; returns false (n = 0) when there is none.
// finite: every neighbour offset was finite (a non-finite matrix is not rotated).
SVNICP_NORMAL_FN bool normal_from_scatter(double d0, double d1, double d2, double a01, double a02, double a12, bool finite,
                                         double& n0, double& n1, double& n2) {
  double d[3] = {d0, d1, d2};
  double V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  if (finite) {
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
      jacobi_rot<0, 1, 2>(d, a01, a02, a12, V);
      // in the (0, 2) plane the third index is 1: its couplings are a01 (with 0) and a12 (with 2)
      jacobi_rot<0, 2, 1>(d, a02, a01, a12, V);
      // in the (1, 2) plane the third index is 0: a01 (with 1) and a02 (with 2)
      jacobi_rot<1, 2, 0>(d, a12, a01, a02, V);
    }
  }
  // λ0 <= λ1 <= λ2 and the column of λ0
  int lo = 0;
  if (d[1] < d[lo]) lo = 1;
  if (d[2] < d[lo]) lo = 2;
  const double oa = lo == 0 ? d[1] : d[0], ob = lo == 2 ? d[1] : d[2];
  const double l1 = oa < ob ? oa : ob, l2 = oa < ob ? ob : oa;
  n0 = lo == 0 ? V[0] : (lo == 1 ? V[1] : V[2]);
  n1 = lo == 0 ? V[3] : (lo == 1 ? V[4] : V[5]);
  n2 = lo == 0 ? V[6] : (lo == 1 ? V[7] : V[8]);
  const double nn = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
  // valid: every neighbour finite, a neighbourhood with extent, and not collinear (kPlaneMinRatio)
  const bool valid = finite && l2 > 0.0 && l1 >= kPlaneMinRatio * l2 && nn > 0.0;
  n0 = valid ? n0 / nn : 0.0; n1 = valid ? n1 / nn : 0.0; n2 = valid ? n2 / nn : 0.0;
  return valid;
}

}  // namespace svnicp
