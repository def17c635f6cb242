// information.hip — the device half of svnicp_eval_information (include/svnicp_hip.h "information matrix of a registration",
// DESIGN.md §4.13): the Gauss-Newton normal equations H, b of the last svnicp_evaluate's pairs, right perturbation
// T Exp([v ; omega]).  Two kernels, no search: every row's q, nearest target index and d2 are the ones evaluate left.
//   k_information_pairs<form>     per row the terms of the form's sums, per workgroup ONE record (form 2: the GICP form of
//                                 svnicp_eval_information_gicp, §4.13.1)
//   k_information_finalize<form>  one workgroup adds the records in a fixed order and expands them to H[36] | b[6] | pairs,
//                                 sum w, sum w r^2
// No atomics: workgroup w owns rows [256 w, 256 w + 256) (evaluate's layout), every record is folded by fold_record
// (lane_fold_device.hpp), so the order of every addition depends on B alone.
#include "kernels.hpp"
#include "lane_fold_device.hpp"
#include "gicp_pair_device.hpp"

namespace svnicp {

static_assert(kGicpInfoRecord == kInfoPlaneRecord, "the GICP form is folded and finalized as the plane form's record");

namespace {

constexpr int NT = 256;
static_assert(NT == 4 * kWave, "the record is folded across four waves");

template <int FORM> struct Rec { static constexpr int n = FORM == 0 ? kInfoPointRecord : kInfoPlaneRecord; };

// Point record (18): pairs, sum w, sum w d2 | sum w s (3) | sum w s s^T upper triangle 00 01 02 11 12 22 | sum w c (3) |
//                    sum w (s x c) (3), c = R^T e
// Plane record (30): pairs, sum w, sum w r^2 | sum w j j^T upper triangle, row-major (21) | sum w r j (6), j = [m ; s x m],
//                    m = R^T n
// GICP record (30):  the plane record's layout: pairs, sum w, sum w rho^2 | sum w G^T W G upper triangle, row-major (21) |
//                    sum w G^T W u (6); one row's record is gicp_information_row (gicp_pair_device.hpp), where the pair algebra
//                    of k_gicp_accumulate is stated
// Operands of rows that do not contribute are SELECTED to zero before any product, so a NaN or inf row reaches no sum.
template <int FORM>
__global__ __launch_bounds__(NT) void k_information_pairs(InfoArgs a) {
  constexpr int N = Rec<FORM>::n;
  __shared__ double lds[4 * N];
  double v[N];
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = 0.0;
  const int64_t b = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (b < a.B) {
    const double d2 = a.d2[b];                       // NaN = not evaluated: never an inlier
    int64_t j = a.idx[b];
    j = j < 0 ? 0 : (j >= a.M ? a.M - 1 : j);        // never an address outside the target
    const double* p = a.rec ? a.rec + 6 * j : a.tgt + 3 * j;
    const bool inlier = d2 < a.thr2;
    const double e0 = a.q[3 * b] - p[0], e1 = a.q[3 * b + 1] - p[1], e2 = a.q[3 * b + 2] - p[2];
    const double* R = a.T.R;
    if (FORM == 0) {
      const bool on = inlier;
      const double d = sqrt(d2);
      const double w = on ? (d <= a.delta ? 1.0 : a.delta / d) : 0.0;
      const double s0 = on ? a.src[3 * b] : 0.0, s1 = on ? a.src[3 * b + 1] : 0.0, s2 = on ? a.src[3 * b + 2] : 0.0;
      const double f0 = on ? e0 : 0.0, f1 = on ? e1 : 0.0, f2 = on ? e2 : 0.0;
      const double c0 = (R[0] * f0 + R[3] * f1) + R[6] * f2;
      const double c1 = (R[1] * f0 + R[4] * f1) + R[7] * f2;
      const double c2 = (R[2] * f0 + R[5] * f1) + R[8] * f2;
      v[0] = on ? 1.0 : 0.0; v[1] = w; v[2] = w * (on ? d2 : 0.0);
      v[3] = w * s0; v[4] = w * s1; v[5] = w * s2;
      v[6] = w * (s0 * s0); v[7] = w * (s0 * s1); v[8] = w * (s0 * s2);
      v[9] = w * (s1 * s1); v[10] = w * (s1 * s2); v[11] = w * (s2 * s2);
      v[12] = w * c0; v[13] = w * c1; v[14] = w * c2;
      v[15] = w * (s1 * c2 - s2 * c1); v[16] = w * (s2 * c0 - s0 * c2); v[17] = w * (s0 * c1 - s1 * c0);
    } else if constexpr (FORM == 2) {   // constexpr: the call takes a 30-value record
      // one gathered target normal, one coalesced source normal; launched with rec and srec only.  A row that is not an
      // inlier passes on = false and its operands are never multiplied
      const double* ns = a.srec + 6 * b + 3;
      gicp_information_row(v, inlier, R, a.src[3 * b], a.src[3 * b + 1], a.src[3 * b + 2], e0, e1, e2, p[3], p[4], p[5], ns[0], ns[1], ns[2],
                           a.eps, a.delta);
    } else {
      const double n0 = p[3], n1 = p[4], n2 = p[5];   // FORM 1 is launched with rec only
      const bool on = inlier && (n0 != 0.0 || n1 != 0.0 || n2 != 0.0);
      const double rr = (n0 * e0 + n1 * e1) + n2 * e2;
      const double r = on ? rr : 0.0, ar = fabs(r);
      const double w = on ? (ar <= a.delta ? 1.0 : a.delta / ar) : 0.0;
      const double s0 = on ? a.src[3 * b] : 0.0, s1 = on ? a.src[3 * b + 1] : 0.0, s2 = on ? a.src[3 * b + 2] : 0.0;
      const double g0 = on ? n0 : 0.0, g1 = on ? n1 : 0.0, g2 = on ? n2 : 0.0;
      double jv[6];
      jv[0] = (R[0] * g0 + R[3] * g1) + R[6] * g2;
      jv[1] = (R[1] * g0 + R[4] * g1) + R[7] * g2;
      jv[2] = (R[2] * g0 + R[5] * g1) + R[8] * g2;
      jv[3] = s1 * jv[2] - s2 * jv[1]; jv[4] = s2 * jv[0] - s0 * jv[2]; jv[5] = s0 * jv[1] - s1 * jv[0];
      v[0] = on ? 1.0 : 0.0; v[1] = w; v[2] = w * (r * r);
      int k = 3;
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int jj = i; jj < 6; ++jj) v[k++] = w * (jv[i] * jv[jj]);
#pragma unroll
      for (int i = 0; i < 6; ++i) v[24 + i] = (w * r) * jv[i];
    }
  }
  fold_record<N>(v, lds, a.partial + (size_t)blockIdx.x * N);
}

// out[kInfoResult] = H[36] row-major, order [v ; omega] | b[6] | pairs, sum w, sum w r^2.  Thread t adds the records
// t, t + 256, ... in ascending order; the 256 partial records are folded as in k_information_pairs.
template <int FORM>
__global__ __launch_bounds__(NT) void k_information_finalize(const double* __restrict__ partial, int64_t nblk, double* __restrict__ out) {
  constexpr int N = Rec<FORM>::n;
  __shared__ double lds[4 * N];
  __shared__ double tot[N];
  double acc[N];
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = 0.0;
  for (int64_t w = threadIdx.x; w < nblk; w += NT)
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] += partial[(size_t)w * N + i];
  fold_record<N>(acc, lds, tot);
  __syncthreads();
  const int t = threadIdx.x;
  if (t >= kInfoResult) return;
  if (t >= 42) { out[t] = tot[t - 42]; return; }
  if (FORM == 0) {
    // H = [[sum w I, -hat(sum w s)], [hat(sum w s), sum w (|s|^2 I - s s^T)]],  b = [sum w c ; sum w s x c]
    const double* ws = tot + 3;
    const double* ss = tot + 6;   // 00 01 02 11 12 22
    if (t >= 36) { out[t] = tot[12 + (t - 36)]; return; }
    const int r = t / 6, c = t % 6;
    double h;
    if (r < 3 && c < 3) h = r == c ? tot[1] : 0.0;
    else if (r >= 3 && c >= 3) {
      const int i = r - 3, k = c - 3;
      if (i == k) h = i == 0 ? ss[3] + ss[5] : (i == 1 ? ss[0] + ss[5] : ss[0] + ss[3]);
      else { const int lo = i < k ? i : k, hi = i < k ? k : i; h = -(lo == 0 ? ss[hi] : ss[4]); }
    } else {
      // hat(u)[i][k]: (0,1) -u2 (0,2) u1 (1,0) u2 (1,2) -u0 (2,0) -u1 (2,1) u0; the upper-right block is -hat, the lower-left hat
      const int i = r % 3, k = c % 3;
      double hat = 0.0;
      if (i != k) { const int o = 3 - i - k; hat = ((k - i + 3) % 3 == 1) ? -ws[o] : ws[o]; }
      h = r < 3 ? -hat : hat;
    }
    out[t] = h;
  } else {
    if (t >= 36) { out[t] = tot[24 + (t - 36)]; return; }
    const int r = t / 6, c = t % 6;
    const int lo = r < c ? r : c, hi = r < c ? c : r;
    out[t] = tot[3 + (lo * 6 - lo * (lo - 1) / 2) + (hi - lo)];   // the row-major upper triangle: row lo starts at 6 lo - lo (lo - 1) / 2
  }
}

}  // namespace

hipError_t launch_information(int form, const InfoArgs& a, double* result, hipStream_t st) {
  if (a.B <= 0 || a.M <= 0 || form < 0 || form > 2 || (form != 0 && !a.rec) || (form == 2 && !a.srec)) return hipErrorInvalidValue;
  const int64_t nblk = evaluate_blocks(a.B);
  if (form == 0) hipLaunchKernelGGL(k_information_pairs<0>, dim3((unsigned)nblk), dim3(NT), 0, st, a);
  else if (form == 1) hipLaunchKernelGGL(k_information_pairs<1>, dim3((unsigned)nblk), dim3(NT), 0, st, a);
  else hipLaunchKernelGGL(k_information_pairs<2>, dim3((unsigned)nblk), dim3(NT), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (form == 0) hipLaunchKernelGGL(k_information_finalize<0>, dim3(1), dim3(NT), 0, st, a.partial, nblk, result);
  else hipLaunchKernelGGL(k_information_finalize<1>, dim3(1), dim3(NT), 0, st, a.partial, nblk, result);   // the GICP record has the plane record's layout
  return hipGetLastError();
}

}  // namespace svnicp
