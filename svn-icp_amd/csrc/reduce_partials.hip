// reduce_partials.hip — the accumulate workgroups' partial records added per particle, in block order (general chain; the
// small chain's prepare lanes add the records themselves, stein_step_device.hpp: load_sums).
#include "kernels.hpp"
#include "lane_fold_device.hpp"

namespace svnicp {

namespace {

// sums[p_lo + i][s] = Σ_blk partial[blk][i][s] in the fixed order of reduce_block_records (lane_fold_device.hpp):
// deterministic, and independent of the launch geometry.
__global__ __launch_bounds__(256) void k_reduce_partials(const double* __restrict__ partial, int nblk, int Ppad, int p_lo,
                                                          int n_particles, double* __restrict__ sums, const int* __restrict__ ctl) {
  if (ctl[0]) return;
  const int el = threadIdx.x & 15, bl = threadIdx.x >> 4;
  const int entry = blockIdx.x * 16 + el;  // index into [n_particles][kNSums]
  const int n_entries = n_particles * kNSums;
  const double s = reduce_block_records(partial + entry, (size_t)Ppad * kNSums, nblk, entry < n_entries);
  if (bl == 0 && entry < n_entries) sums[(size_t)p_lo * kNSums + entry] = s;
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
