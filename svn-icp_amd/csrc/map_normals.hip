// map_normals.hip — normals of the last query's rows, from the 27-voxel blocks of the map (svnicp_map_query_normals,
// DESIGN.md §4.4).  Not in the reference.
//
// One wave per selected voxel (key2 / slot2 / off / cnt of the last query's MapSelection).  Lanes 0..26 look the voxel's 3x3x3
// block up in the table (read-only, bounded linear probing: on past kTomb, stop at kEmpty; lane 13, the voxel itself, takes
// slot2); lane order is ascending (x, y, z) voxel index, i.e. ascending packed key.  The block's points
// are copied ONCE into LDS, in that order, slots of a voxel ascending: the candidates of every point of the voxel.  Per point
// (wave-uniform loop): d² = ((dx·dx)+dy·dy)+dz·dz in f64 of the widened f32 coordinates (stage A's expression, unfused) for a
// tile of candidates, appended to the best normal_k kept so far; the normal_k smallest by (d², enumeration order) of that
// working list become the new best.  The normal_k-th smallest d² is found by bisection on its 64-bit pattern (non-negative
// doubles order as unsigned integers; 63 ballots + popcounts per stride), everything below it is kept and the ties at it in
// list order by prefix counts; the compaction keeps list order and the kept set precedes the next tile, so list order stays
// enumeration order over all tiles.  Sums: lane l < normal_k holds neighbour l (enumeration order), the other lanes +0; each of
// the 3 + 6 sums is the butterfly v += shfl_xor(v, 32, 16, 8, 4, 2, 1): one fixed shape, every lane the same bits.  Mean and
// scatter matrix are two passes over offsets relative to the point (§4.9).  Lane i keeps the scatter matrix of the voxel's
// point i; after (at most) 64 points the lanes turn theirs into normals (plane_normal_device.hpp) side by side.
// LDS: f64 d² [64 + tile] | f32 xyz [27·max_points][3] | u16 candidate index [64 + tile]; no per-thread arrays.
#include "map_normals.hpp"

#include "plane_normal_device.hpp"
#include "voxel_table_device.hpp"

namespace svnicp {
namespace {

constexpr int kNrmTile = 1024;   // candidates whose d² are in LDS at a time (27·max_points above it: several tiles)

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// wd / wi [w], w > kn: afterwards wd / wi [0, kn) hold the kn smallest by (d², position), in position order
__device__ __forceinline__ void select_smallest(double* wd, unsigned short* wi, int w, int kn, int lane) {
  const int strides = (w + 63) >> 6;
  // the first two strides stay in registers over the bisection (w <= 128 is the common case); the others are read from LDS
  const unsigned long long x0 = lane < w ? (unsigned long long)__double_as_longlong(wd[lane]) : ~0ull;
  const unsigned long long x1 = 64 + lane < w ? (unsigned long long)__double_as_longlong(wd[64 + lane]) : ~0ull;
  unsigned long long thr = 0;   // the largest pattern with fewer than kn entries below it = the kn-th smallest entry
  for (int bit = 62; bit >= 0; --bit) {
    const unsigned long long cand = thr | (1ull << bit);
    int below = __popcll(__ballot(x0 < cand));
    if (strides > 1) below += __popcll(__ballot(x1 < cand));
    for (int s = 2; s < strides; ++s) {
      const int e = s * 64 + lane;
      const unsigned long long x = e < w ? (unsigned long long)__double_as_longlong(wd[e]) : ~0ull;
      below += __popcll(__ballot(x < cand));
    }
    if (below < kn) thr = cand;
  }
  int below = __popcll(__ballot(x0 < thr)) + __popcll(__ballot(x1 < thr));
  for (int s = 2; s < strides; ++s) {
    const int e = s * 64 + lane;
    const unsigned long long x = e < w ? (unsigned long long)__double_as_longlong(wd[e]) : ~0ull;
    below += __popcll(__ballot(x < thr));
  }
  const int need = kn - below;   // ties at the threshold to keep, first in list order
  int outp = 0, ties = 0;
  for (int s = 0; s < strides; ++s) {
    const int e = s * 64 + lane;
    const unsigned long long x = e < w ? (unsigned long long)__double_as_longlong(wd[e]) : ~0ull;
    const unsigned short idx = e < w ? wi[e] : (unsigned short)0;
    const bool tie = x == thr;
    const unsigned long long bt = __ballot(tie);
    const bool sel = x < thr || (tie && ties + lanes_below(bt) < need);
    const unsigned long long bs = __ballot(sel);
    const int pos = outp + lanes_below(bs);   // pos <= e: entries of this stride are all read before any is written
    __builtin_amdgcn_wave_barrier();
    if (sel) { wd[pos] = __longlong_as_double((long long)x); wi[pos] = idx; }
    outp += __popcll(bs); ties += __popcll(bt);
  }
  __syncthreads();
}

__global__ __launch_bounds__(64) void k_map_normals(const unsigned long long* __restrict__ keys, const int* __restrict__ counts,
                                                    const float* __restrict__ pts, int64_t cap, int max_points,
                                                    const unsigned long long* __restrict__ skey, const unsigned int* __restrict__ sslot,
                                                    const int* __restrict__ offs, const int* __restrict__ cnts, int nsel, int kn, int tile,
                                                    double* __restrict__ out,
                                                    int* __restrict__ with_normal) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ unsigned int s_slot[27];
  __shared__ int s_cnt[27], s_off[28];
  const int j = blockIdx.x, lane = threadIdx.x;
  if (j >= nsel || cnts[j] <= 0) return;   // entries the selection did not fill count zero points (workgroup-uniform)
  double* wd = reinterpret_cast<double*>(smem);
  float* cxyz = reinterpret_cast<float*>(wd + 64 + tile);
  unsigned short* wi = reinterpret_cast<unsigned short*>(cxyz + (size_t)81 * max_points);
  const unsigned long long key = skey[j];
  if (lane < 27) {
    const long long v0 = (long long)(key >> 42) - kOff + (lane / 9 - 1);
    const long long v1 = (long long)((key >> 21) & 0x1fffffull) - kOff + ((lane / 3) % 3 - 1);
    const long long v2 = (long long)(key & 0x1fffffull) - kOff + (lane % 3 - 1);
    unsigned int slot = 0;
    int c = 0;
    if (lane == 13) {   // the voxel itself: its slot is the query's
      slot = sslot[j]; c = counts[slot];
    } else if (svnicp::voxel_in_range(v0, v1, v2)) {   // outside: no such voxel
      const int64_t h = svnicp::find_slot(keys, cap, pack_key(v0, v1, v2));   // bounded; the table is only read
      if (h >= 0) { slot = (unsigned int)h; c = counts[h]; }
    }
    s_slot[lane] = slot;
    s_cnt[lane] = c < 0 ? 0 : (c > max_points ? max_points : c);
  }
  __syncthreads();
  if (lane < 28) {
    int o = 0;
    for (int i = 0; i < lane; ++i) o += s_cnt[i];
    s_off[lane] = o;
  }
  __syncthreads();
  const int n = s_off[27];   // <= 27 * max_points
  for (int v = 0; v < 27; ++v) {   // a voxel's points are contiguous in the table: coalesced copies
    const int c3 = 3 * s_cnt[v];
    const float* src = pts + (size_t)s_slot[v] * max_points * 3;
    float* dst = cxyz + 3 * s_off[v];
    for (int e = lane; e < c3; e += 64) dst[e] = src[e];
  }
  __syncthreads();
  const int own = s_cnt[13];   // = cnts[j]: the host refuses the call once the map has changed since the query
  const int own_off = s_off[13];
  double* orow = out + 3 * (size_t)offs[j];
  if (n < kn) {   // fewer candidates than neighbours asked for: no normal in this voxel
    for (int e = lane; e < 3 * own; e += 64) orow[e] = 0.0;
    return;
  }
  int nvalid = 0;
  for (int b0 = 0; b0 < own; b0 += 64) {
    const int bn = own - b0 < 64 ? own - b0 : 64;
    double S0 = 0.0, S1 = 0.0, S2 = 0.0, A01 = 0.0, A02 = 0.0, A12 = 0.0;   // scatter matrix of point b0 + lane
    for (int ii = 0; ii < bn; ++ii) {
      const int pi = own_off + b0 + ii;
      const double px = (double)cxyz[3 * pi], py = (double)cxyz[3 * pi + 1], pz = (double)cxyz[3 * pi + 2];
      int nbest = 0;
      for (int t0 = 0; t0 < n; t0 += tile) {
        const int m = n - t0 < tile ? n - t0 : tile;
        for (int e = lane; e < m; e += 64) {
          const int c = t0 + e;
          const double dx = (double)cxyz[3 * c] - px, dy = (double)cxyz[3 * c + 1] - py, dz = (double)cxyz[3 * c + 2] - pz;
          wd[nbest + e] = (dx * dx + dy * dy) + dz * dz;
          wi[nbest + e] = (unsigned short)c;
        }
        __syncthreads();
        if (nbest + m > kn) { select_smallest(wd, wi, nbest + m, kn, lane); nbest = kn; }
        else nbest += m;
      }
      // nbest == kn (n >= kn); neighbour l of the point in enumeration order is candidate wi[l]
      const bool on = lane < kn;
      const int c = on ? (int)wi[lane] : 0;
      const double o0 = on ? (double)cxyz[3 * c] - px : 0.0, o1 = on ? (double)cxyz[3 * c + 1] - py : 0.0,
                   o2 = on ? (double)cxyz[3 * c + 2] - pz : 0.0;
      const double m0 = wave_sum(o0) / kn, m1 = wave_sum(o1) / kn, m2 = wave_sum(o2) / kn;
      const double c0 = on ? o0 - m0 : 0.0, c1 = on ? o1 - m1 : 0.0, c2 = on ? o2 - m2 : 0.0;
      const double s0 = wave_sum(c0 * c0), s1 = wave_sum(c1 * c1), s2 = wave_sum(c2 * c2);
      const double a01 = wave_sum(c0 * c1), a02 = wave_sum(c0 * c2), a12 = wave_sum(c1 * c2);
      if (lane == ii) { S0 = s0; S1 = s1; S2 = s2; A01 = a01; A02 = a02; A12 = a12; }
      __syncthreads();   // the working list is rebuilt for the next point
    }
    double n0 = 0.0, n1 = 0.0, n2 = 0.0;
    bool valid = false;
    if (lane < bn) {
      valid = svnicp::normal_from_scatter(S0, S1, S2, A01, A02, A12, true, n0, n1, n2);   // stored points are finite
      double* o = orow + 3 * (size_t)(b0 + lane);
      o[0] = n0; o[1] = n1; o[2] = n2;
    }
    nvalid += __popcll(__ballot(valid));
  }
  if (lane == 0 && nvalid) atomicAdd(with_normal, nvalid);
}

// k_map_normals' d² tile and dynamic LDS for a map of max_points points per voxel (at most 91.6 KB, at 256)
int normals_tile(int max_points) { const int block = 27 * max_points; return block < kNrmTile ? (block + 63) / 64 * 64 : kNrmTile; }
size_t normals_lds(int max_points) {
  return (size_t)(64 + normals_tile(max_points)) * (sizeof(double) + sizeof(unsigned short)) + (size_t)27 * max_points * 3 * sizeof(float);
}

}  // namespace

hipError_t map_normals_prepare(int max_points) {
  if (normals_lds(max_points) <= 48 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(k_map_normals), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
}

hipError_t launch_map_normals(const MapTableView& T, const MapSelection& S, int normal_k, double* out, int* with_normal,
                              hipStream_t stream) {
  HIPTRY(hipMemsetAsync(with_normal, 0, sizeof(int), stream));
  return launch_checked(k_map_normals, dim3((unsigned)S.last_live), dim3(64), normals_lds(T.max_points), stream, T.keys, T.counts, T.pts,
                        T.cap, T.max_points, S.key2.p, S.slot2.p, S.off.p, S.cnt.p, (int)S.last_live, normal_k, normals_tile(T.max_points), out,
                        with_normal);
}

}  // namespace svnicp
