// lane_fold_device.hpp — the lane <-> particle geometry of the stage-B style kernels and the project's fixed-order folds,
// each stated once (DESIGN.md §4.2 "Fixed-order folds").
//
// The contract they carry: every sum depends on B and P alone, never on the launch geometry — a record is built by ONE tree
// of additions, so GPU tests compare exactly and two builds can be compared bit for bit.
//   ParticleLanes<PW, WP>        a 256-thread workgroup as PW particles per wave, WP waves along the particles, the remaining
//                                lanes (BW = 64 / PW) and waves (WB = 4 / WP) along the source rows
//   load_pose                    a particle's total pose, [R row-major | t]
//   fold_particle_record<N>      N accumulators per lane -> one record per (workgroup, particle): xor butterfly over the row
//                                lanes from off = PW upward, row waves 1 … WB-1 through LDS, added in wave order
//   reduce_block_records         second stage: one entry of the workgroups' records added over the workgroups, 16 entries x
//                                16 block lanes per workgroup, block lane l adds blocks l, l + 16, … in ascending order,
//                                then the 16 lanes are folded in order
//   fold_record<N>               the row-owned kernels (thread <-> source row): xor butterfly off = 1 … 32, then the four
//                                waves ((w0 + w1) + w2) + w3
#pragma once
#include "kernels.hpp"

#define SVNICP_CONST_AS __attribute__((address_space(4)))   // read-only for the launch: wave-uniform addresses become s_load

namespace svnicp {
namespace {

template <int PW, int WP>
struct ParticleLanes {
  static constexpr int BW = kWave / PW;   // source rows a wave works on at a time
  static constexpr int WB = 4 / WP;       // waves along the source rows
  static constexpr int STEP = WB * BW;    // row slots of the workgroup
  static constexpr int NP = WP * PW;      // particles of the workgroup
  int wp, wb;   // the wave's place along the particles / the rows (wave-uniform)
  int pl, bs;   // the lane's particle inside the wave / its row slot
  int pidx;     // particle index inside the (padded) shard
  __device__ __forceinline__ explicit ParticleLanes(int by) {   // by: the workgroup's index along the particles
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    wp = wave % WP; wb = wave / WP;
    pl = lane % PW; bs = lane / PW;
    pidx = by * NP + wp * PW + pl;
  }
};

__device__ __forceinline__ void load_pose(const double* row12, double (&Rt)[9], double (&tt)[3]) {
#pragma unroll
  for (int i = 0; i < 9; ++i) Rt[i] = row12[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) tt[i] = row12[9 + i];
}

// acc summed over the workgroup's row lanes and row waves; the lane that owns the particle (wb == 0, bs == 0) stores the N
// doubles to partial + (row_base + pidx) * N.  lds: [(WB - 1)][NP][N] doubles, written without a barrier in front — a
// caller whose LDS still holds a tile places its own.
// accumulate_body (stein_split_device.hpp) spells this fold out at its end, because through this function its WP = 1
// instantiations cost one or two VGPRs at the four-wave limit: a change to either site is a change to both.
template <int N, int PW, int WP>
__device__ __forceinline__ void fold_particle_record(const ParticleLanes<PW, WP>& L, double (&acc)[N], double* lds, double* partial,
                                                     size_t row_base) {
  constexpr int WB = ParticleLanes<PW, WP>::WB, NP = ParticleLanes<PW, WP>::NP;
#pragma unroll
  for (int off = PW; off < kWave; off <<= 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] += __shfl_xor(acc[i], off, kWave);
  }
  if constexpr (WB > 1) {
    if (L.wb > 0 && L.bs == 0) {
      double* r = lds + ((size_t)(L.wb - 1) * NP + L.wp * PW + L.pl) * N;
#pragma unroll
      for (int i = 0; i < N; ++i) r[i] = acc[i];
    }
    __syncthreads();
    if (L.wb == 0 && L.bs == 0) {
      for (int o = 0; o < WB - 1; ++o) {
        const double* r = lds + ((size_t)o * NP + L.wp * PW + L.pl) * N;
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] += r[i];
      }
    }
  }
  if (L.wb == 0 && L.bs == 0) {
    double* out = partial + (row_base + L.pidx) * N;
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = acc[i];
  }
}

// Σ_blk src[blk * stride] in the fixed order above, for the entry of thread (el = tid & 15, bl = tid >> 4) of a 256-thread
// workgroup; the sum is returned to block lane 0 of each entry (bl == 0; other lanes get 0.0).  valid == false: the entry
// reads nothing and sums to 0.0.  One barrier, which every thread of the workgroup must reach.
__device__ __forceinline__ double reduce_block_records(const double* src, size_t stride, int nblk, bool valid) {
  __shared__ double red[16][17];
  const int el = threadIdx.x & 15, bl = threadIdx.x >> 4;
  double a = 0.0;
  if (valid) {
    int blk = bl;
    for (; blk + 7 * 16 < nblk; blk += 8 * 16) {   // eight loads in flight
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
  double s = 0.0;
  if (bl == 0 && valid) {
    s = red[0][el];
#pragma unroll
    for (int i = 1; i < 16; ++i) s += red[i][el];
  }
  return s;
}

// v[N] summed over a 256-thread workgroup into out[N]: each value by an xor butterfly inside its wave, then ONE pass through
// LDS — lane 0 of every wave stores its N totals, the first N threads add the four waves in order.  One barrier here; the
// caller places another before lds is written again (or before out, when it is LDS, is read).
template <int N>
__device__ __forceinline__ void fold_record(double (&v)[N], double* lds /* [4][N] */, double* out /* [N] */) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) v[i] += __shfl_xor(v[i], off, kWave);
  const int w = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) lds[w * N + i] = v[i];
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const int i = threadIdx.x;
    out[i] = ((lds[i] + lds[N + i]) + lds[2 * N + i]) + lds[3 * N + i];
  }
}

}  // namespace
}  // namespace svnicp
