// evaluate.hip — svnicp_evaluate (include/svnicp_hip.h "evaluate a registration"): one pose against the
// whole target.  Three kernels around stage A's own K = 1 search (api.hip: svnicp_evaluate):
//   k_evaluate_transform  q = R s + t, the expression of k_transform_cloud without its stop flag (evaluate must work after an
//                         early-stopped registration)
//   k_evaluate_pairs      per row: gather the nearest target (or its xyz | normal record), recompute d2, classify, write the
//                         index and d2; per workgroup ONE record {evaluated, inliers, plane inliers, sum d2, sum r2}
//   k_evaluate_finalize   one workgroup adds the records in a fixed order and forms the ratios and roots
// No atomics: workgroup w owns rows [256 w, 256 w + 256) and folds its record by fold_record (lane_fold_device.hpp), so every
// addition happens in an order that depends on B alone and the same context state gives the same bits on every call.
#include "kernels.hpp"
#include "lane_fold_device.hpp"

namespace svnicp {
namespace {

constexpr int NT = 256;
static_assert(NT == 4 * kWave, "the record is folded across four waves");

__global__ __launch_bounds__(NT) void k_evaluate_transform(const double* __restrict__ src, int64_t B, EvalPose T, double* __restrict__ q) {
  const int64_t b = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (b >= B) return;
  const double s0 = src[3 * b], s1 = src[3 * b + 1], s2 = src[3 * b + 2];
  q[3 * b] = (s0 * T.R[0] + s1 * T.R[1] + s2 * T.R[2]) + T.t[0];        // oracle/svnicp_oracle.c: orc_transform
  q[3 * b + 1] = (s0 * T.R[3] + s1 * T.R[4] + s2 * T.R[5]) + T.t[1];
  q[3 * b + 2] = (s0 * T.R[6] + s1 * T.R[7] + s2 * T.R[8]) + T.t[2];
}

__global__ __launch_bounds__(NT) void k_evaluate_pairs(EvalArgs a) {
  __shared__ double lds[4 * kEvalRecord];
  const int64_t b = (int64_t)blockIdx.x * NT + threadIdx.x;
  double ev = 0.0, in = 0.0, pin = 0.0, sd = 0.0, sr = 0.0;   // the counts are exact in float64 (B < 2^31)
  if (b < a.B) {
    const double q0 = a.q[3 * b], q1 = a.q[3 * b + 1], q2 = a.q[3 * b + 2];
    int64_t j = a.idx[b];
    j = j < 0 ? 0 : (j >= a.M ? a.M - 1 : j);   // never an address outside the target
    const double* p = a.rec ? a.rec + 6 * j : a.tgt + 3 * j;
    const double e0 = q0 - p[0], e1 = q1 - p[1], e2 = q2 - p[2];
    const double d2 = ((e0 * e0) + e1 * e1) + e2 * e2;
    const bool qfin = isfinite(q0) && isfinite(q1) && isfinite(q2);
    const bool evaluated = qfin && d2 == d2;    // also the contract's "index 0, d2 = 0.0" filler of a row without a neighbour
    const bool inlier = evaluated && d2 < a.thr2;   // +inf is evaluated and never an inlier
    a.idx[b] = evaluated ? (int32_t)j : -1;
    a.d2[b] = evaluated ? d2 : __builtin_nan("");
    ev = evaluated ? 1.0 : 0.0;
    in = inlier ? 1.0 : 0.0;
    sd = inlier ? d2 : 0.0;
    if (a.rec) {
      const double n0 = p[3], n1 = p[4], n2 = p[5];
      const bool pl = inlier && (n0 != 0.0 || n1 != 0.0 || n2 != 0.0);   // a zero row: no normal here
      const double r = (n0 * e0 + n1 * e1) + n2 * e2;
      pin = pl ? 1.0 : 0.0;
      sr = pl ? r * r : 0.0;
    }
  }
  double v[kEvalRecord] = {ev, in, pin, sd, sr};
  fold_record<kEvalRecord>(v, lds, a.partial + (size_t)blockIdx.x * kEvalRecord);
}

// out[kEvalResult] = {evaluated, inliers, plane inliers, sum d2, sum r2, fitness, inlier rmse, plane rmse}.  Thread t adds
// the records t, t + 256, ... in ascending order; the 256 partial records are folded as in k_evaluate_pairs.
__global__ __launch_bounds__(NT) void k_evaluate_finalize(const double* __restrict__ partial, int64_t nblk, int64_t rows, double* __restrict__ out) {
  __shared__ double lds[4 * kEvalRecord];
  __shared__ double tot[kEvalRecord];
  double acc[kEvalRecord] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t w = threadIdx.x; w < nblk; w += NT)
#pragma unroll
    for (int i = 0; i < kEvalRecord; ++i) acc[i] += partial[(size_t)w * kEvalRecord + i];
  fold_record<kEvalRecord>(acc, lds, tot);
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < kEvalRecord; ++i) out[i] = tot[i];
    out[5] = tot[1] / (double)rows;
    out[6] = tot[1] > 0.0 ? sqrt(tot[3] / tot[1]) : 0.0;
    out[7] = tot[2] > 0.0 ? sqrt(tot[4] / tot[2]) : 0.0;
  }
}

}  // namespace

int64_t evaluate_blocks(int64_t B) { return (B + NT - 1) / NT; }

hipError_t launch_evaluate_transform(const double* src, int64_t B, const EvalPose& T, double* q, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_evaluate_transform, dim3((unsigned)evaluate_blocks(B)), dim3(NT), 0, st, src, B, T, q);
  return hipGetLastError();
}

hipError_t launch_evaluate_pairs(const EvalArgs& a, double* result, hipStream_t st) {
  if (a.B <= 0 || a.M <= 0) return hipErrorInvalidValue;
  const int64_t nblk = evaluate_blocks(a.B);
  hipLaunchKernelGGL(k_evaluate_pairs, dim3((unsigned)nblk), dim3(NT), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_evaluate_finalize, dim3(1), dim3(NT), 0, st, a.partial, nblk, a.B, result);
  return hipGetLastError();
}

}  // namespace svnicp
