// minibatch.hip — SteinICPParam::use_minibatch / batch_size (SVGDICP::mini_batch_pair_generator, SVGDICP.cpp:176-199):
// iteration i works on the source rows idx[i][0..batch) of a table drawn with replacement.  Ahead of stage A, on the
// context's stream, without a host synchronisation:
//   draw + mark   the table (generated from a counter-based stream, or an explicit one that is validated here) and a
//                 flag per source row that was drawn
//   compact       exclusive scan of the flags -> pos[row]; the U drawn rows in ascending order -> src_u; rows U..n_q-1 of
//                 src_u repeat row U-1, so that stage A can run on the host-known count n_q = min(B, I*batch)
//   expand        (after stage A on src_u) the epoch-major layout the stage-B kernels index by a contiguous row number:
//                 src_mb [I*batch][3], cand_mb [I*batch][K] = cand_u[pos[idx[j]]]
// An out-of-range value of an explicit table is never used as an address: the kernel that validates is the kernel that
// marks, it skips the value, raises mbctl[0] and the registration's stop flag (every stage-B launch then returns at once),
// and the expand kernel maps such a position to unique row 0 so that the table build behind it reads defined indices.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace svnicp {

namespace {

constexpr int kMbThreads = 256;
constexpr int kMbRowsPerThread = 4;
constexpr int kMbRowsPerBlock = kMbThreads * kMbRowsPerThread;

__host__ __device__ inline unsigned long long mb_splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  unsigned long long z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(kMbThreads) void k_mb_draw_mark(MinibatchArgs a) {
  const int64_t j = (int64_t)blockIdx.x * kMbThreads + threadIdx.x;
  if (j >= a.n) return;
  int32_t v;
  if (a.explicit_idx) {
    v = a.explicit_idx[j];
    a.idx[j] = v;
    if (v < 0 || (int64_t)v >= a.B) {   // reported, never dereferenced
      a.mbctl[0] = 1;
      a.ctl[0] = 1;
      return;
    }
  } else {
    const unsigned long long bits = mb_splitmix64(a.base + (unsigned long long)j);
    v = (int32_t)__umul64hi(bits, (unsigned long long)a.B);
    a.idx[j] = v;
  }
  a.flag[v] = 1;
}

// inclusive scan of one value per thread over the workgroup (kMbThreads entries of LDS)
__device__ inline int block_inclusive_scan(int v, int* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int d = 1; d < kMbThreads; d <<= 1) {
    const int add = tid >= d ? sh[tid - d] : 0;
    __syncthreads();
    sh[tid] += add;
    __syncthreads();
  }
  return sh[tid];
}

__device__ inline void load_flags(const int32_t* flag, int64_t B, int64_t r0, int (&f)[kMbRowsPerThread]) {
#pragma unroll
  for (int u = 0; u < kMbRowsPerThread; ++u) f[u] = (r0 + u < B && flag[r0 + u]) ? 1 : 0;
}

__global__ __launch_bounds__(kMbThreads) void k_mb_count(const int32_t* flag, int64_t B, int32_t* block_sums) {
  __shared__ int sh[kMbThreads];
  const int64_t r0 = (int64_t)blockIdx.x * kMbRowsPerBlock + (int64_t)threadIdx.x * kMbRowsPerThread;
  int f[kMbRowsPerThread];
  load_flags(flag, B, r0, f);
  int c = 0;
#pragma unroll
  for (int u = 0; u < kMbRowsPerThread; ++u) c += f[u];
  const int incl = block_inclusive_scan(c, sh);
  if (threadIdx.x == kMbThreads - 1) block_sums[blockIdx.x] = incl;
}

// one workgroup: block_sums -> exclusive prefix in place, the total (U) -> mbctl[1]
__global__ __launch_bounds__(kMbThreads) void k_mb_scan_blocks(int32_t* block_sums, int nblk, int* mbctl) {
  __shared__ int sh[kMbThreads];
  __shared__ int carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int b0 = 0; b0 < nblk; b0 += kMbThreads) {
    const int i = b0 + threadIdx.x;
    const int v = i < nblk ? block_sums[i] : 0;
    const int incl = block_inclusive_scan(v, sh);
    const int carry = carry_s;
    if (i < nblk) block_sums[i] = carry + incl - v;
    __syncthreads();
    if (threadIdx.x == kMbThreads - 1) carry_s = carry + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) mbctl[1] = carry_s;
}

__global__ __launch_bounds__(kMbThreads) void k_mb_compact(const int32_t* flag, int64_t B, const int32_t* block_sums, const double* src,
                                                           int32_t* pos, double* src_u) {
  __shared__ int sh[kMbThreads];
  const int64_t r0 = (int64_t)blockIdx.x * kMbRowsPerBlock + (int64_t)threadIdx.x * kMbRowsPerThread;
  int f[kMbRowsPerThread];
  load_flags(flag, B, r0, f);
  int c = 0;
#pragma unroll
  for (int u = 0; u < kMbRowsPerThread; ++u) c += f[u];
  int p = block_sums[blockIdx.x] + block_inclusive_scan(c, sh) - c;
#pragma unroll
  for (int u = 0; u < kMbRowsPerThread; ++u) {
    const int64_t r = r0 + u;
    if (r >= B) break;
    if (f[u]) {
      pos[r] = p;
      src_u[3 * (size_t)p + 0] = src[3 * (size_t)r + 0];
      src_u[3 * (size_t)p + 1] = src[3 * (size_t)r + 1];
      src_u[3 * (size_t)p + 2] = src[3 * (size_t)r + 2];
      ++p;
    } else {
      pos[r] = -1;
    }
  }
}

// rows U..n_q-1 of src_u: copies of row U-1 (harmless duplicate queries); no row drawn at all (a table of bad values only):
// source row 0, so that stage A still reads defined coordinates
__global__ __launch_bounds__(kMbThreads) void k_mb_fill(double* src_u, const double* src, const int* mbctl, int64_t n_q) {
  const int64_t r = (int64_t)blockIdx.x * kMbThreads + threadIdx.x;
  const int64_t U = mbctl[1];
  if (r >= n_q || r < U) return;
  const double* from = U > 0 ? src_u + 3 * (size_t)(U - 1) : src;
  src_u[3 * (size_t)r + 0] = from[0];
  src_u[3 * (size_t)r + 1] = from[1];
  src_u[3 * (size_t)r + 2] = from[2];
}

// one wave per table position: a candidate row is K consecutive int32
__global__ __launch_bounds__(kMbThreads) void k_mb_expand(const int32_t* idx, int64_t n, int64_t B, const int32_t* pos, const double* src,
                                                          const int32_t* cand_u, int K, double* src_mb, int32_t* cand_mb) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * (kMbThreads / 64) + (threadIdx.x >> 6);
  if (j >= n) return;
  const int32_t v = idx[j];
  const bool ok = v >= 0 && (int64_t)v < B;
  const size_t row = ok ? (size_t)v : 0;
  const int32_t pu = ok ? pos[row] : 0;
  const size_t u = pu >= 0 ? (size_t)pu : 0;
  if (lane < 3) src_mb[3 * (size_t)j + lane] = src[3 * row + lane];
  const int32_t* from = cand_u + u * (size_t)K;
  int32_t* to = cand_mb + (size_t)j * K;
  for (int k = lane; k < K; k += 64) to[k] = from[k];
}

}  // namespace

unsigned long long minibatch_stream_base(unsigned long long seed, unsigned long long registration) {
  return mb_splitmix64(seed * 1000003ull + registration);
}

int64_t minibatch_scan_blocks(int64_t B) { return (B + kMbRowsPerBlock - 1) / kMbRowsPerBlock; }

hipError_t launch_minibatch_draw_compact(const MinibatchArgs& a, hipStream_t st) {
  if (a.n < 1 || a.B < 1 || a.n_q < 1) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.flag, 0, (size_t)a.B * sizeof(int32_t), st);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(a.mbctl, 0, 2 * sizeof(int), st)) != hipSuccess) return e;
  const unsigned nblk = (unsigned)minibatch_scan_blocks(a.B);
  hipLaunchKernelGGL(k_mb_draw_mark, dim3((unsigned)((a.n + kMbThreads - 1) / kMbThreads)), dim3(kMbThreads), 0, st, a);
  hipLaunchKernelGGL(k_mb_count, dim3(nblk), dim3(kMbThreads), 0, st, a.flag, a.B, a.block_sums);
  hipLaunchKernelGGL(k_mb_scan_blocks, dim3(1), dim3(kMbThreads), 0, st, a.block_sums, (int)nblk, a.mbctl);
  hipLaunchKernelGGL(k_mb_compact, dim3(nblk), dim3(kMbThreads), 0, st, a.flag, a.B, a.block_sums, a.src, a.pos, a.src_u);
  hipLaunchKernelGGL(k_mb_fill, dim3((unsigned)((a.n_q + kMbThreads - 1) / kMbThreads)), dim3(kMbThreads), 0, st, a.src_u, a.src,
                     a.mbctl, a.n_q);
  return hipGetLastError();
}

hipError_t launch_minibatch_expand(const MinibatchArgs& a, const int32_t* cand_u, int K, double* src_mb, int32_t* cand_mb,
                                   hipStream_t st) {
  if (a.n < 1 || K < 1) return hipErrorInvalidValue;
  const int rows_per_block = kMbThreads / 64;
  hipLaunchKernelGGL(k_mb_expand, dim3((unsigned)((a.n + rows_per_block - 1) / rows_per_block)), dim3(kMbThreads), 0, st, a.idx, a.n,
                     a.B, a.pos, a.src, cand_u, K, src_mb, cand_mb);
  return hipGetLastError();
}

}  // namespace svnicp
