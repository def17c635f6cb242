// reduce_partials.hip — the accumulate workgroups' partial records added per particle, in block order (general chain; the
// small chain's prepare lanes add the records themselves, stein_step_device.hpp: load_sums).
#include "kernels.hpp"

namespace svnicp {

namespace {

// sums[p_lo + i][s] = Σ_blk partial[blk][i][s], block order fixed.  Workgroup = 16 entries × 16 block lanes; each block
// lane walks blk = bl, bl+16, … with eight loads in flight and the 16 lanes are folded in order: deterministic, and
// independent of the launch geometry.
__global__ __launch_bounds__(256) void k_reduce_partials(const double* __restrict__ partial, int nblk, int Ppad, int p_lo,
                                                          int n_particles, double* __restrict__ sums, const int* __restrict__ ctl) {
  if (ctl[0]) return;
  __shared__ double red[16][17];
  const int el = threadIdx.x & 15, bl = threadIdx.x >> 4;
  const int entry = blockIdx.x * 16 + el;  // index into [n_particles][kNSums]
  const int n_entries = n_particles * kNSums;
  double a = 0.0;
  if (entry < n_entries) {
    const size_t stride = (size_t)Ppad * kNSums;
    const double* src = partial + entry;
    int blk = bl;
    for (; blk + 7 * 16 < nblk; blk += 8 * 16) {
      double v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = src[(size_t)(blk + 16 * i) * stride];
#pragma unroll
      for (int i = 0; i < 8; ++i) a += v[i];
    }
    for (; blk < nblk; blk += 16) a += src[(size_t)blk * stride];
  }
  red[bl][el] = a;
  __syncthreads();
  if (bl == 0 && entry < n_entries) {
    double s = red[0][el];
#pragma unroll
    for (int i = 1; i < 16; ++i) s += red[i][el];
    sums[(size_t)p_lo * kNSums + entry] = s;
  }
}

}  // namespace

hipError_t launch_reduce_partials(const double* partial, int nblk, int Ppad, int p_lo, int n_particles, double* sums, const int* ctl,
                                  hipStream_t st) {
  const int n_entries = n_particles * kNSums;
  if (n_entries <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_reduce_partials, dim3((n_entries + 15) / 16), dim3(256), 0, st, partial, nblk, Ppad, p_lo, n_particles, sums, ctl);
  return hipGetLastError();
}

}  // namespace svnicp
