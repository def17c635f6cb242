// gicp_pair_device.hpp — one pair of the generalized-ICP residual: the combined weight of the two surfaces
// and the pair's terms of H, b and the statistics.  Stated once for k_gicp_accumulate (gicp_icp.hip), for the GICP form
// of the information matrix (information.hip) and for the GICP form of the particle scores (particle_score.hip).
//
// In the source frame, with m = Rtᵀ n_q (the winner's unit normal), n the source point's unit normal, u = Rtᵀ (Ts − q):
//   C(x) = I − (1 − ε) x xᵀ          regularised surface covariance: ε along the normal, 1 in the plane
//   S    = C(m) + C(n)               symmetric, eigenvalues in [2ε, 2], condition <= 1 / ε
//   W    = 2ε S⁻¹                    eigenvalues in [ε, 1]; parallel normals: (1 − ε) m mᵀ + ε I; ε = 1: I exactly
//   ρ    = √(uᵀ W u),  w = 1 (ρ <= δ) else δ / ρ,  G = [I₃ | −[s]×]
//   H   += w GᵀWG = w [ W , −W[s]× ; · , [s]×ᵀ W [s]× ],   b += w GᵀW u = w [ W u ; s × W u ]
// W is frozen at the linearisation pose, so b is the exact gradient of Σ Huber(ρ) with W held fixed.
//
// The header stands alone and also compiles for the host (tests/gicp_accum_driver.cpp runs it under the address and
// undefined-behaviour sanitizers): device functions under hipcc, plain inline functions elsewhere.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define SVNICP_GICP_FN __device__ __forceinline__
#define SVNICP_GICP_HOST_FN __host__ __device__ __forceinline__   // the host states a scoring's cap with the device's own function
#else
#define SVNICP_GICP_FN inline
#define SVNICP_GICP_HOST_FN inline
#endif

namespace svnicp {

constexpr double kGicpEpsilonDefault = 1e-3;   // the GICP paper's value
constexpr double kGicpEpsilonMin = 1e-6;       // cond(S) <= 1e6: the closed-form inverse keeps ten digits
constexpr int kGicpSums = 29;                  // = kPlaneSums: H upper triangle (21) | b (6) | accepted pairs | Σ w·ρ²

// W = 2ε (C(m) + C(n))⁻¹ by cofactors, upper triangle [W00 W01 W02 W11 W12 W22].  m = n = 0 (a rejected pair) gives ε I.
SVNICP_GICP_FN void gicp_weight(double m0, double m1, double m2, double n0, double n1, double n2, double eps, double (&W)[6]) {
  const double a = 1.0 - eps;
  const double s00 = 2.0 - a * (m0 * m0 + n0 * n0), s11 = 2.0 - a * (m1 * m1 + n1 * n1), s22 = 2.0 - a * (m2 * m2 + n2 * n2);
  const double s01 = -(a * (m0 * m1 + n0 * n1)), s02 = -(a * (m0 * m2 + n0 * n2)), s12 = -(a * (m1 * m2 + n1 * n2));
  const double c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
  const double c11 = s00 * s22 - s02 * s02, c12 = s01 * s02 - s00 * s12, c22 = s00 * s11 - s01 * s01;
  const double det = (s00 * c00 + s01 * c01) + s02 * c02;   // >= (2ε)·(2ε)·2 > 0
  const double k = (2.0 * eps) / det;
  W[0] = k * c00; W[1] = k * c01; W[2] = k * c02; W[3] = k * c11; W[4] = k * c12; W[5] = k * c22;
}

// The pair's metric terms, before any robust weight: W = gicp_weight(m, n, ε), v = W u, and ρ² = max(uᵀ v, 0) (returned).
// Stated once for gicp_pair_sums (H, b, the statistics) and gicp_pair_cost (the particle scores).
SVNICP_GICP_FN double gicp_pair_metric(double u0, double u1, double u2, double m0, double m1, double m2, double n0, double n1, double n2,
                                       double eps, double (&W)[6], double (&v)[3]) {
  gicp_weight(m0, m1, m2, n0, n1, n2, eps, W);
  v[0] = (W[0] * u0 + W[1] * u1) + W[2] * u2;   // W u
  v[1] = (W[1] * u0 + W[3] * u1) + W[4] * u2;
  v[2] = (W[2] * u0 + W[4] * u1) + W[5] * u2;
  const double q = (u0 * v[0] + u1 * v[1]) + u2 * v[2];
  return q > 0.0 ? q : 0.0;                     // W is positive definite: a negative value is round-off of a zero
}

// h(x) for x >= 0, handed x and its square x2: x2 inside δ, δ (2x − δ) beyond — twice Huber's ρ, so δ = +inf gives x2 itself
// and the unit stays m².  The branch is a select, and the outer term is formed from a δ that is selected to zero inside: never
// a product with an unselected inf.  Stated once for the plane and the GICP form of the particle scores.
SVNICP_GICP_HOST_FN double robust_cost(double x, double x2, double delta) {
  const bool in = x <= delta;
  const double d = in ? 0.0 : delta;
  return in ? x2 : d * (2.0 * x - d);
}

// One pair of the particle scores' GICP form (particle_score.hip): h(√ρ²) with ρ² as gicp_pair_sums forms
// it, 0 for a rejected pair; `accepted` is 1.0 or 0.0.  ok == false: every operand is selected to zero first, as below.
SVNICP_GICP_FN double gicp_pair_cost(bool ok, double u0, double u1, double u2, double m0, double m1, double m2, double n0, double n1, double n2,
                                     double eps, double delta, double& accepted, double* rho2_out = nullptr) {
  u0 = ok ? u0 : 0.0; u1 = ok ? u1 : 0.0; u2 = ok ? u2 : 0.0;
  m0 = ok ? m0 : 0.0; m1 = ok ? m1 : 0.0; m2 = ok ? m2 : 0.0;
  n0 = ok ? n0 : 0.0; n1 = ok ? n1 : 0.0; n2 = ok ? n2 : 0.0;
  double W[6], v[3];
  const double rho2 = gicp_pair_metric(u0, u1, u2, m0, m1, m2, n0, n1, n2, eps, W, v);
  if (rho2_out) *rho2_out = rho2;
  accepted = ok ? 1.0 : 0.0;
  return robust_cost(sqrt(rho2), rho2, delta);   // inside δ the term is ρ² itself; a rejected pair: ρ² = 0, h = 0 exactly
}

// One pair into the 29 sums; returns the pair's Huber weight w (0 for a rejected pair).  s: the source point, u = Rtᵀ e,
// m = Rtᵀ n_q, n: the source normal.  ok == false: every operand is selected to zero first (never multiplied: a non-finite point
// must not leak a NaN), so the pair adds exact zeros.
SVNICP_GICP_FN double gicp_pair_sums(double (&acc)[kGicpSums], bool ok, double s0, double s1, double s2, double u0, double u1, double u2,
                                     double m0, double m1, double m2, double n0, double n1, double n2, double eps, double delta) {
  s0 = ok ? s0 : 0.0; s1 = ok ? s1 : 0.0; s2 = ok ? s2 : 0.0;
  u0 = ok ? u0 : 0.0; u1 = ok ? u1 : 0.0; u2 = ok ? u2 : 0.0;
  m0 = ok ? m0 : 0.0; m1 = ok ? m1 : 0.0; m2 = ok ? m2 : 0.0;
  n0 = ok ? n0 : 0.0; n1 = ok ? n1 : 0.0; n2 = ok ? n2 : 0.0;
  double W[6], v[3];
  const double rho2 = gicp_pair_metric(u0, u1, u2, m0, m1, m2, n0, n1, n2, eps, W, v);
  const double v0 = v[0], v1 = v[1], v2 = v[2];
  const double rho = sqrt(rho2);
  const double w = ok ? (rho <= delta ? 1.0 : delta / rho) : 0.0;   // Huber: 1 inside delta, delta / ρ outside
  double ww[6];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 6; ++i) ww[i] = w * W[i];
  // A = w W [s]×: row i = (w W)_i × s
  const double a00 = ww[1] * s2 - ww[2] * s1, a01 = ww[2] * s0 - ww[0] * s2, a02 = ww[0] * s1 - ww[1] * s0;
  const double a10 = ww[3] * s2 - ww[4] * s1, a11 = ww[4] * s0 - ww[1] * s2, a12 = ww[1] * s1 - ww[3] * s0;
  const double a20 = ww[4] * s2 - ww[5] * s1, a21 = ww[5] * s0 - ww[2] * s2, a22 = ww[2] * s1 - ww[4] * s0;
  // H upper triangle, row-major (k_plane_finalize's order): rows 0-2 = [w W | −A], rows 3-5 = [s]×ᵀ A
  acc[0] += ww[0]; acc[1] += ww[1]; acc[2] += ww[2]; acc[3] -= a00; acc[4] -= a01; acc[5] -= a02;
  acc[6] += ww[3]; acc[7] += ww[4]; acc[8] -= a10; acc[9] -= a11; acc[10] -= a12;
  acc[11] += ww[5]; acc[12] -= a20; acc[13] -= a21; acc[14] -= a22;
  acc[15] += s2 * a10 - s1 * a20; acc[16] += s2 * a11 - s1 * a21; acc[17] += s2 * a12 - s1 * a22;
  acc[18] += s0 * a21 - s2 * a01; acc[19] += s0 * a22 - s2 * a02;
  acc[20] += s1 * a02 - s0 * a12;
  const double b0 = w * v0, b1 = w * v1, b2 = w * v2;       // b = w [W u ; s × W u]
  acc[21] += b0; acc[22] += b1; acc[23] += b2;
  acc[24] += s1 * b2 - s2 * b1; acc[25] += s2 * b0 - s0 * b2; acc[26] += s0 * b1 - s1 * b0;
  acc[27] += ok ? 1.0 : 0.0;
  acc[28] += w * rho2;
  return w;
}

// k_gicp_accumulate's pair: the sums alone.
SVNICP_GICP_FN void gicp_accumulate_pair(double (&acc)[kGicpSums], bool ok, double s0, double s1, double s2, double u0, double u1, double u2,
                                         double m0, double m1, double m2, double n0, double n1, double n2, double eps, double delta) {
  (void)gicp_pair_sums(acc, ok, s0, s1, s2, u0, u1, u2, m0, m1, m2, n0, n1, n2, eps, delta);
}

// One row of svnicp_eval_information_gicp (information.hip) as the plane form's 30-value record:
//   pairs, w, w ρ² | the 21 upper-triangle entries of w GᵀWG, row-major | the 6 of w GᵀWu
// R: the evaluated pose's rotation, row-major; s: the source row; e = q − p; nq: the nearest target's normal; ns: the source
// row's normal.  `on`: the row is one of evaluate's inliers.  It contributes iff both normals are non-zero, k_gicp_accumulate's
// rule; otherwise every operand is selected to zero before any product and the record is exact zeros.  The pair's terms are
// gicp_pair_sums' on sums that start at zero, so the algebra is stated once.
constexpr int kGicpInfoRecord = 30;
SVNICP_GICP_FN void gicp_information_row(double (&v)[kGicpInfoRecord], bool on, const double* R, double s0, double s1, double s2,
                                         double e0, double e1, double e2, double nq0, double nq1, double nq2,
                                         double ns0, double ns1, double ns2, double eps, double delta) {
  const bool ok = on && (nq0 != 0.0 || nq1 != 0.0 || nq2 != 0.0) && (ns0 != 0.0 || ns1 != 0.0 || ns2 != 0.0);
  const double g0 = ok ? e0 : 0.0, g1 = ok ? e1 : 0.0, g2 = ok ? e2 : 0.0;
  const double h0 = ok ? nq0 : 0.0, h1 = ok ? nq1 : 0.0, h2 = ok ? nq2 : 0.0;
  const double u0 = R[0] * g0 + R[3] * g1 + R[6] * g2;   // u = Rᵀ e
  const double u1 = R[1] * g0 + R[4] * g1 + R[7] * g2;
  const double u2 = R[2] * g0 + R[5] * g1 + R[8] * g2;
  const double m0 = R[0] * h0 + R[3] * h1 + R[6] * h2;   // m = Rᵀ n_q
  const double m1 = R[1] * h0 + R[4] * h1 + R[7] * h2;
  const double m2 = R[2] * h0 + R[5] * h1 + R[8] * h2;
  double t[kGicpSums];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < kGicpSums; ++i) t[i] = 0.0;
  const double w = gicp_pair_sums(t, ok, s0, s1, s2, u0, u1, u2, m0, m1, m2, ns0, ns1, ns2, eps, delta);
  v[0] = t[27]; v[1] = w; v[2] = t[28];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 27; ++i) v[3 + i] = t[i];
}

}  // namespace svnicp
