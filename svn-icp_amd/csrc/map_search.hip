// map_search.hip — the coarse-to-fine pose search against the voxel map (svnicp_map_search_poses; the contract is in
// include/svnicp_hip.h, the design in DESIGN.md §4.17).  Per level: k_map_search_nodes writes the level's lattice vectors and
// poses, launch_map_score (map_score.hip, unchanged) scores them, k_map_search_rank writes the indices of the kept nodes in rank
// order; the next level's nodes are made from that list on the device.  After the last level k_map_search_gather collects what
// the host reads into one block.  Every count is known on the host before the first launch; nothing is copied between levels.
#include "map_search.hpp"

#include "device_math.hpp"

namespace svnicp {
namespace {

// The pose of a node: guess · correction_to_pose(x), x[a] = (double)k[a] * fine[a] -- one multiplication.  R = G_R · Exp(x[3:6]),
// t = ((r0·x0 + r1·x1) + r2·x2) + G_t per row of G_R; float64, unfused (-ffp-contract=off).  Stated once: nodes and gather use it.
__device__ __forceinline__ void node_correction(const MapSearchGrid& g, const int* k, double* x) {
#pragma unroll
  for (int a = 0; a < 6; ++a) x[a] = (double)k[a] * g.fine[a];
}
__device__ __forceinline__ void node_pose(const MapSearchGrid& g, const double* x, double* P) {
  double E[9];
  so3_exp(x + 3, E, nullptr);
  mat3_mul(g.G, E, P);
#pragma unroll
  for (int d = 0; d < 3; ++d) P[9 + d] = ((g.G[3 * d] * x[0] + g.G[3 * d + 1] * x[1]) + g.G[3 * d + 2] * x[2]) + g.G[9 + d];
}

// One thread per node of a level.  scale = 3^(levels-1-level).  Level 0 (parent_lat == nullptr): node i is the i-th vector of
// j·scale, j = -m..m per axis, lexicographic with x slowest.  A later level: node i is child i % 3^A of the parent of rank
// i / 3^A, the offsets {-1, 0, 1}·scale over the active axes, lexicographic with x slowest.  Every index into k, m and fine is a
// compile-time constant after unrolling: registers and kernel arguments, no scratch.
__global__ __launch_bounds__(256) void k_map_search_nodes(MapSearchGrid g, int scale, int count, const int32_t* __restrict__ parent_lat,
                                                          const int32_t* __restrict__ parent_kept, int32_t* __restrict__ lat,
                                                          double* __restrict__ poses) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= count) return;
  int k[6];
  if (parent_lat == nullptr) {
    int r = i;
#pragma unroll
    for (int a = 5; a >= 0; --a) {
      const int w = 2 * g.m[a] + 1;
      k[a] = (r % w - g.m[a]) * scale;
      r /= w;
    }
  } else {
    const int parent = parent_kept[i / g.children];
    int o = i % g.children;
#pragma unroll
    for (int a = 5; a >= 0; --a) {
      k[a] = parent_lat[6 * (int64_t)parent + a];
      if ((g.active_mask >> a) & 1) { k[a] += (o % 3 - 1) * scale; o /= 3; }
    }
  }
  double x[6], P[12];
  node_correction(g, k, x);
  node_pose(g, x, P);
#pragma unroll
  for (int a = 0; a < 6; ++a) lat[6 * (int64_t)i + a] = k[a];
#pragma unroll
  for (int j = 0; j < 12; ++j) poses[12 * (int64_t)i + j] = P[j];
}

// ---- rank --------------------------------------------------------------------------------------------------------------------
// The order is ascending (cost, k[0], ..., k[5]).  A non-negative double orders as its bit pattern, and a lattice entry offset by
// 2^20 fits 21 bits, so a node's key is three 64-bit words compared in turn: the cost bits, k[0..2] packed, k[3..5] packed.  No
// two nodes of a level share a lattice vector, so no two keys are equal.
using u64 = unsigned long long;
__device__ __forceinline__ u64 lat_word(const int32_t* __restrict__ L) {
  return ((u64)(unsigned)(L[0] + kLatOff) << 42) | ((u64)(unsigned)(L[1] + kLatOff) << 21) | (u64)(unsigned)(L[2] + kLatOff);
}

// One workgroup.  (1) A radix select, most significant byte first, finds the set of the `kept` smallest keys: S is the set of
// nodes whose key agrees with the threshold on every byte decided so far, `need` how many of S are wanted; a pass counts S by
// its next byte in a 256-bin LDS histogram and moves into the bin that holds the need-th node.  It stops as soon as all of S
// is wanted -- for costs without ties usually within the eight passes over the cost bytes; the lattice words are read only
// when costs tie at the threshold (an empty map ties everywhere and takes up to 24 passes).  (2) The nodes at or below the
// threshold prefix are collected in LDS.  (3) Each is ranked by counting the collected keys below its own, and its index is
// written at that rank.  The atomics are integer counts into the histogram and a slot counter for (2): the collected SET does
// not depend on arrival order, and (3) orders it by distinct keys, so no arrival order reaches the output.
__global__ __launch_bounds__(kRankThreads) void k_map_search_rank(const double* __restrict__ rec, const int32_t* __restrict__ lat,
                                                                  int count, int kept, int32_t* __restrict__ kept_out) {
  __shared__ unsigned int s_hist[256];
  __shared__ u64 s_w0[kSearchMaxKeep], s_w1[kSearchMaxKeep], s_w2[kSearchMaxKeep];
  __shared__ int s_idx[kSearchMaxKeep];
  __shared__ unsigned int s_bin, s_need, s_size, s_n;
  const int tid = threadIdx.x;
  u64 t0 = 0, t1 = 0, t2 = 0, M0 = 0, M1 = 0, M2 = 0;   // the threshold's decided bytes and their masks, per word
  unsigned int need = (unsigned int)kept, size = (unsigned int)count;
  for (int pass = 0; pass < 24 && size != need; ++pass) {   // uniform: every thread holds the same need and size
    const int cw = pass >> 3, shift = 56 - 8 * (pass & 7);
    if (tid < 256) s_hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < count; i += kRankThreads) {
      const u64 w0 = (u64)__double_as_longlong(rec[4 * (int64_t)i + 3]);
      bool in = (w0 & M0) == t0;
      u64 cur = w0;
      if (cw > 0 && in) {
        const u64 w1 = lat_word(lat + 6 * (int64_t)i), w2 = lat_word(lat + 6 * (int64_t)i + 3);
        in = (w1 & M1) == t1 && (w2 & M2) == t2;
        cur = cw == 1 ? w1 : w2;
      }
      if (in) atomicAdd(&s_hist[(unsigned int)(cur >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {   // the first wave finds the bin of the need-th node: four bins per lane, a prefix sum over the lanes
      unsigned int c[4], own = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { c[j] = s_hist[4 * tid + j]; own += c[j]; }
      unsigned int upto = own;   // inclusive
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned int v = __shfl_up(upto, off, 64);
        if (tid >= off) upto += v;
      }
      unsigned int below = upto - own;
      if (below < need && need <= upto) {   // exactly one lane: 1 <= need <= |S|
        unsigned int b = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (b == (unsigned int)j && below + c[j] < need) { below += c[j]; b = j + 1; }
        s_bin = 4 * tid + b; s_need = need - below; s_size = b == 0 ? c[0] : (b == 1 ? c[1] : (b == 2 ? c[2] : c[3]));
      }
    }
    __syncthreads();
    const u64 bits = (u64)s_bin << shift, mask = (u64)255 << shift;
    need = s_need; size = s_size;
    if (cw == 0) { t0 |= bits; M0 |= mask; } else if (cw == 1) { t1 |= bits; M1 |= mask; } else { t2 |= bits; M2 |= mask; }
  }
  if (tid == 0) s_n = 0;
  __syncthreads();
  for (int i = tid; i < count; i += kRankThreads) {
    const u64 w0 = (u64)__double_as_longlong(rec[4 * (int64_t)i + 3]);
    const u64 a0 = w0 & M0;
    if (a0 > t0) continue;   // most nodes leave here, before their lattice is read
    const u64 w1 = lat_word(lat + 6 * (int64_t)i), w2 = lat_word(lat + 6 * (int64_t)i + 3);
    const u64 a1 = w1 & M1, a2 = w2 & M2;
    const bool sel = a0 != t0 ? true : (a1 != t1 ? a1 < t1 : a2 <= t2);   // at or below the threshold on the decided bytes
    if (!sel) continue;
    const unsigned int slot = atomicAdd(&s_n, 1u);
    if (slot < (unsigned int)kept) { s_w0[slot] = w0; s_w1[slot] = w1; s_w2[slot] = w2; s_idx[slot] = i; }
  }
  __syncthreads();
  const int n = s_n < (unsigned int)kept ? (int)s_n : kept;
  for (int i = tid; i < n; i += kRankThreads) {
    const u64 w0 = s_w0[i], w1 = s_w1[i], w2 = s_w2[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {   // every lane reads the same j: LDS broadcasts
      const u64 v0 = s_w0[j], v1 = s_w1[j], v2 = s_w2[j];
      rank += (v0 != w0 ? v0 < w0 : (v1 != w1 ? v1 < w1 : v2 < w2)) ? 1 : 0;
    }
    kept_out[rank] = s_idx[i];
  }
}

// After the last level: stage = zero_rec[4] | n_top x {correction 6, pose 12, record 4} | n_top x 6 int32 of lattice, the kept
// nodes in rank order.  One thread per kept node; thread 0 also copies the level-0 record of the zero correction.
__global__ __launch_bounds__(256) void k_map_search_gather(MapSearchGrid g, const int32_t* __restrict__ lat, const double* __restrict__ poses,
                                                           const double* __restrict__ rec, const int32_t* __restrict__ kept, int n_top,
                                                           const double* __restrict__ zero_rec, double* __restrict__ stage) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) stage[j] = zero_rec[j];
  }
  if (i >= n_top) return;
  const int64_t node = kept[i];
  int k[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) k[a] = lat[6 * node + a];
  double x[6];
  node_correction(g, k, x);
  double* __restrict__ o = stage + 4 + (int64_t)kSearchTopDoubles * i;
#pragma unroll
  for (int a = 0; a < 6; ++a) o[a] = x[a];
#pragma unroll
  for (int j = 0; j < 12; ++j) o[6 + j] = poses[12 * node + j];
#pragma unroll
  for (int j = 0; j < 4; ++j) o[18 + j] = rec[4 * node + j];
  int32_t* __restrict__ li = reinterpret_cast<int32_t*>(stage + 4 + (int64_t)kSearchTopDoubles * n_top) + 6 * (int64_t)i;
#pragma unroll
  for (int a = 0; a < 6; ++a) li[a] = k[a];
}

}  // namespace

hipError_t launch_map_search_nodes(const MapSearchGrid& grid, int level, int levels, int64_t count, const int32_t* parent_lat,
                                   const int32_t* parent_kept, int32_t* lat, double* poses, hipStream_t stream) {
  const int scale = (int)pow3(levels - 1 - level);
  hipLaunchKernelGGL(k_map_search_nodes, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, grid, scale, (int)count,
                     level == 0 ? nullptr : parent_lat, parent_kept, lat, poses);
  return hipGetLastError();
}

hipError_t launch_map_search_rank(const double* rec, const int32_t* lat, int64_t count, int kept, int32_t* kept_out, hipStream_t stream) {
  hipLaunchKernelGGL(k_map_search_rank, dim3(1), dim3(kRankThreads), 0, stream, rec, lat, (int)count, kept, kept_out);
  return hipGetLastError();
}

hipError_t launch_map_search_gather(const MapSearchGrid& grid, const int32_t* lat, const double* poses, const double* rec,
                                    const int32_t* kept, int n_top, const double* zero_rec, double* stage, hipStream_t stream) {
  hipLaunchKernelGGL(k_map_search_gather, dim3((unsigned)((n_top + 255) / 256)), dim3(256), 0, stream, grid, lat, poses, rec, kept, n_top,
                     zero_rec, stage);
  return hipGetLastError();
}

}  // namespace svnicp
