// voxel_map.hip — the local map of the scan-to-map loop, resident in HBM.
//
// SURVEY.md §8(f)-4 (second half).  Device counterpart of svnicp::VoxelHashMap
// (/root/reference/svn-icp/src/core/VoxelHashMap.cpp:22-101, include/core/VoxelHashMap.h): a hash map
// voxel -> at most max_points points in insertion order, with
//   AddPointCloud(cloud, pose)  (:22-42)  transform by the pose (float32 like pcl::PointXYZ), voxel index = coordinates /
//                                          voxel_size truncated toward zero (:29), append while the voxel has room, then
//   RemoveFarPointCloud(pos)    (:89-97)  drop every voxel whose FIRST point is farther than max_range,
//   GetMap(pose, r) / GetMap()  (:44-58)  all points of the voxels whose first point is closer than r (or of all voxels).
// Not in the reference: the normals of a query's rows from the map's own voxels (svnicp_map_query_normals) and the
// visibility-based clearing of stored points a new scan sees through (svnicp_map_clear_seen_through), both further down.
// The reference keeps it in a tsl::robin_map on the host and re-uploads the query result for every scan
// (OdometryPipeline.cpp:577-582); here the table lives in HBM and a query writes float64 rows straight into a device
// buffer the solver copies device-to-device (svnicp_set_target, SVNICP_MEM_DEVICE) — per scan only the new points go over
// PCIe.
//
// Layout: open addressing, linear probing; keys[cap] = packed voxel index (3 x 21 bits, offset 2^20) or EMPTY / TOMB;
// counts[cap]; pts[cap][max_points] float3.  Determinism: a point's slot is found (or created by atomicCAS) in parallel,
// but WHICH points a voxel keeps is decided in input order — the (slot, input index) pairs are radix-sorted (stable), a
// point's rank inside its voxel is its position in the sorted run, and it is stored at counts[slot] + rank if that is
// below max_points: exactly the points the sequential loop of the reference keeps, in the same order.  A query emits
// voxels in ascending (x, y, z) voxel index (radix sort of the selected keys), so the output is reproducible and equals
// the ordered host map of svn-icp_amd/host/registration_pipeline.hpp point for point.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/svnicp_hip.h"
#include "device_buffer.hpp"
#include "kernels.hpp"
#include "map_score.hpp"
#include "map_search.hpp"
#include "plane_normal_device.hpp"
#include "range_project_device.hpp"
#include "voxel_table_device.hpp"

namespace {

// the table's key packing, hash and read-only lookup: voxel_table_device.hpp
using svnicp::kEmpty;
using svnicp::kTomb;
using svnicp::kOff;
using svnicp::hash_key;
using svnicp::pack_key;

struct MapPose { double R[9]; double t[3]; };

// transform + voxel key + find-or-create the voxel's slot
__global__ __launch_bounds__(256) void k_map_locate(const float* __restrict__ in, int64_t n, MapPose pose, float voxel,
                                                    unsigned long long* __restrict__ keys, int64_t cap,
                                                    float* __restrict__ q, unsigned int* __restrict__ slot_of,
                                                    int* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float p0 = in[3 * i], p1 = in[3 * i + 1], p2 = in[3 * i + 2];
  // pcl::transformPointCloud with gtsam's double Matrix4 (VoxelHashMap.cpp:25): every coordinate is formed in double from the
  // widened float32 point, left to right, and rounded ONCE to float32
  float c[3];
#pragma unroll
  for (int d = 0; d < 3; ++d)
    c[d] = (float)(((pose.R[3 * d] * (double)p0 + pose.R[3 * d + 1] * (double)p1) + pose.R[3 * d + 2] * (double)p2) + pose.t[d]);
  q[3 * i] = c[0]; q[3 * i + 1] = c[1]; q[3 * i + 2] = c[2];
  long long v[3];
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float f = truncf(c[d] / voxel);   // Eigen cast<int>: toward zero (VoxelHashMap.cpp:29)
    ok = ok && (f >= (float)-kOff) && (f < (float)kOff);   // also false for NaN
    v[d] = ok ? (long long)f : 0;
  }
  if (!ok) { slot_of[i] = 0xffffffffu; atomicAdd(&stats[3], 1); return; }   // outside the index range or NaN: counted, not stored
  const unsigned long long key = pack_key(v[0], v[1], v[2]);
  unsigned long long h = hash_key(key) & (unsigned long long)(cap - 1);
  for (int64_t probe = 0; probe < cap; ++probe) {   // bounded: a full table ends the loop and is reported
    unsigned long long cur = keys[h];
    if (cur == kEmpty) cur = atomicCAS(&keys[h], kEmpty, key);
    if (cur == key || cur == kEmpty) { slot_of[i] = (unsigned int)h; return; }
    h = (h + 1) & (unsigned long long)(cap - 1);
  }
  slot_of[i] = 0xffffffffu;
  atomicOr(&stats[2], 2);
}

__global__ __launch_bounds__(256) void k_map_iota(int* __restrict__ v, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = (int)i;
}

__device__ __forceinline__ int64_t lower_bound_u32(const unsigned int* a, int64_t n, unsigned int v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a[mid] < v) lo = mid + 1; else hi = mid; }
  return lo;
}

// sorted by (slot, input index): store the points that still fit, in input order
__global__ __launch_bounds__(256) void k_map_place(const unsigned int* __restrict__ sslot, const int* __restrict__ sidx, int64_t n,
                                                   const int* __restrict__ counts, int max_points, const float* __restrict__ q,
                                                   float* __restrict__ pts) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned int s = sslot[j];
  if (s == 0xffffffffu) return;
  const int64_t rank = j - lower_bound_u32(sslot, n, s);
  const int64_t pos = (int64_t)counts[s] + rank;
  if (pos >= max_points) return;
  const int i = sidx[j];
  float* o = pts + ((size_t)s * max_points + pos) * 3;
  o[0] = q[3 * (size_t)i]; o[1] = q[3 * (size_t)i + 1]; o[2] = q[3 * (size_t)i + 2];
}

__global__ __launch_bounds__(256) void k_map_count(const unsigned int* __restrict__ sslot, int64_t n, int* __restrict__ counts,
                                                   int max_points, int* __restrict__ stats) {
  __shared__ int s_new;
  if (threadIdx.x == 0) s_new = 0;
  __syncthreads();
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) {
    const unsigned int s = sslot[j];
    if (s != 0xffffffffu && (j == 0 || sslot[j - 1] != s)) {   // one thread per run
      // a voxel next to the sensor takes thousands of points of one scan: the run's end by bisection, not by walking it
      int64_t lo = j + 1, hi = n;
      while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (sslot[mid] <= s) lo = mid + 1; else hi = mid; }
      const int before = counts[s];
      const int64_t after = before + (lo - j);
      counts[s] = after > max_points ? max_points : (int)after;
      if (before == 0) atomicAdd(&s_new, 1);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_new) atomicAdd(&stats[0], s_new);   // one global atomic per workgroup
}

// RemoveFarPointCloud (VoxelHashMap.cpp:89-97)
__global__ __launch_bounds__(256) void k_map_remove_far(unsigned long long* __restrict__ keys, int* __restrict__ counts,
                                                        const float* __restrict__ pts, int64_t cap, int max_points, double px,
                                                        double py, double pz, double r2, int* __restrict__ stats) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= cap) return;
  const unsigned long long k = keys[s];
  if (k == kEmpty || k == kTomb || counts[s] <= 0) return;
  const float* f = pts + (size_t)s * max_points * 3;
  const double dx = (double)f[0] - px, dy = (double)f[1] - py, dz = (double)f[2] - pz;
  if (dx * dx + dy * dy + dz * dz > r2) {
    keys[s] = kTomb; counts[s] = 0;
    atomicSub(&stats[0], 1); atomicAdd(&stats[1], 1);
  }
}

// GetMap(pose, r) selection (VoxelHashMap.cpp:48-58); r2 < 0 selects every voxel (GetMap(), :44-46)
constexpr int kSelChunk = 16;   // slots per thread of k_map_select
__global__ __launch_bounds__(256) void k_map_select(const unsigned long long* __restrict__ keys, const int* __restrict__ counts,
                                                    const float* __restrict__ pts, int64_t cap, int max_points, double px, double py,
                                                    double pz, double r2, unsigned long long* __restrict__ sel_key,
                                                    unsigned int* __restrict__ sel_slot, int* __restrict__ nsel, int limit) {
  // a workgroup owns kSelChunk * 256 consecutive slots: it counts its selected voxels, reserves their output range with ONE
  // global atomic (4096 workgroups with one atomic each on the same address took 45 us) and writes them (any order: the
  // keys are sorted afterwards)
  __shared__ int s_base, s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const int64_t s0 = (int64_t)blockIdx.x * (kSelChunk * 256) + threadIdx.x;
  unsigned int takes = 0;
  unsigned long long k[kSelChunk];
#pragma unroll
  for (int i = 0; i < kSelChunk; ++i) {
    const int64_t s = s0 + (int64_t)i * 256;
    k[i] = s < cap ? keys[s] : kEmpty;
  }
#pragma unroll
  for (int i = 0; i < kSelChunk; ++i) {
    const int64_t s = s0 + (int64_t)i * 256;
    if (k[i] != kEmpty && k[i] != kTomb && counts[s] > 0) {
      bool take = true;
      if (r2 >= 0.0) {
        const float* f = pts + (size_t)s * max_points * 3;
        const double dx = (double)f[0] - px, dy = (double)f[1] - py, dz = (double)f[2] - pz;
        take = dx * dx + dy * dy + dz * dz < r2;
      }
      if (take) takes |= 1u << i;
    }
  }
  int my = 0;
  if (takes) my = atomicAdd(&s_n, __popc(takes));
  __syncthreads();
  if (threadIdx.x == 0 && s_n > 0) s_base = atomicAdd(nsel, s_n);
  __syncthreads();
  int pos = s_base + my;
#pragma unroll
  for (int i = 0; i < kSelChunk; ++i) {
    if ((takes >> i) & 1u) {
      if (pos < limit) { sel_key[pos] = k[i]; sel_slot[pos] = (unsigned int)(s0 + (int64_t)i * 256); }   // limit = live voxels known to the host: never exceeded
      ++pos;
    }
  }
}

__global__ __launch_bounds__(256) void k_map_sel_counts(const unsigned long long* __restrict__ skey, const unsigned int* __restrict__ sslot, int nsel,
                                                        const int* __restrict__ counts, int* __restrict__ cnt_out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < nsel) cnt_out[j] = skey[j] == kEmpty ? 0 : counts[sslot[j]];   // entries the selection did not fill sort to the end with key ~0
}

// voxel j of the sorted selection -> its points as float64 rows (ICPUtils.cpp:27-43 widening) at offs[j]
__global__ __launch_bounds__(256) void k_map_gather(const unsigned int* __restrict__ sslot, const int* __restrict__ offs,
                                                    const int* __restrict__ cnts, int nsel, int max_points,
                                                    const float* __restrict__ pts, double* __restrict__ out, float* __restrict__ out_f32) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // one thread per (voxel, point slot)
  const int j = (int)(g / max_points), k = (int)(g % max_points);
  if (j >= nsel || k >= cnts[j]) return;
  const float* f = pts + ((size_t)sslot[j] * max_points + k) * 3;
  const size_t o = ((size_t)offs[j] + k) * 3;
  if (out) { out[o] = (double)f[0]; out[o + 1] = (double)f[1]; out[o + 2] = (double)f[2]; }
  if (out_f32) { out_f32[o] = f[0]; out_f32[o + 1] = f[1]; out_f32[o + 2] = f[2]; }
}

// rebuild without tombstones: re-insert every live voxel into a fresh table
__global__ __launch_bounds__(256) void k_map_rehash(const unsigned long long* __restrict__ okeys, const int* __restrict__ ocounts,
                                                    const float* __restrict__ opts, int64_t ocap, int max_points,
                                                    unsigned long long* __restrict__ keys, int* __restrict__ counts,
                                                    float* __restrict__ pts, int64_t cap, int* __restrict__ stats) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= ocap) return;
  const unsigned long long key = okeys[s];
  if (key == kEmpty || key == kTomb || ocounts[s] <= 0) return;
  unsigned long long h = hash_key(key) & (unsigned long long)(cap - 1);
  for (int64_t probe = 0; probe < cap; ++probe) {
    if (atomicCAS(&keys[h], kEmpty, key) == kEmpty) {
      counts[h] = ocounts[s];
      const float* a = opts + (size_t)s * max_points * 3;
      float* b = pts + (size_t)h * max_points * 3;
      for (int i = 0; i < 3 * ocounts[s]; ++i) b[i] = a[i];
      return;
    }
    h = (h + 1) & (unsigned long long)(cap - 1);
  }
  atomicOr(&stats[2], 2);
}

// ---------------------------------------------------------------------------------------------
// normals of the last query's rows, from the 27-voxel blocks of the map (svnicp_map_query_normals)
// ---------------------------------------------------------------------------------------------
// One wave per selected voxel (sel_key2 / sel_slot2 / sel_off / sel_cnt of the last query).  Lanes 0..26 look the voxel's 3x3x3
// block up in the table (read-only, bounded linear probing: on past kTomb, stop at kEmpty; lane 13, the voxel itself, takes
// sel_slot2); lane order is ascending (x, y, z) voxel index, i.e. ascending packed key.  The block's points
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
constexpr int kNrmTile = 1024;   // candidates whose d² are in LDS at a time (27·max_points above it: several tiles)

__device__ __forceinline__ int lanes_below(unsigned long long mask) {   // set bits of mask that belong to lanes below this one
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

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

// ---------------------------------------------------------------------------------------------
// visibility-based clearing (svnicp_map_clear_seen_through; the contract is in include/svnicp_hip.h)
// ---------------------------------------------------------------------------------------------
// The minimum-range image holds the bit patterns of non-negative floats, which order as unsigned integers: one 32-bit atomicMin
// per scan point, whatever the schedule.  Empty = the pattern of +inf.
constexpr unsigned int kVisEmpty = 0x7f800000u;

struct VisOpt { int wr, wc; float margin_abs, margin_rel, max_range; };

// the fills of the call in one launch: the image, the selection keys (entries the selection does not fill stay ~0), the
// selection counter and the call's statistics
__global__ __launch_bounds__(256) void k_vis_fill(unsigned int* __restrict__ img, int64_t npix, unsigned long long* __restrict__ sel_key,
                                                  int64_t live, int* __restrict__ nsel, unsigned long long* __restrict__ vstats) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < npix) img[i] = kVisEmpty;
  if (i < live) sel_key[i] = kEmpty;
  if (i < 4) vstats[i] = 0ull;
  if (i == 0) *nsel = 0;
}

__global__ __launch_bounds__(256) void k_vis_image(const float* __restrict__ in, int64_t n, svnicp::RangeSensor S,
                                                   unsigned int* __restrict__ img, unsigned long long* __restrict__ vstats) {
  __shared__ int s_new;
  if (threadIdx.x == 0) s_new = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    int row, col;
    float r;
    if (svnicp::range_project(in[3 * i], in[3 * i + 1], in[3 * i + 2], S, row, col, r)) {
      const unsigned int bits = __float_as_uint(r);   // r >= +0: the pattern orders as the value
      // a pixel counts as filled once: for the thread that finds it empty and brings a finite range
      if (atomicMin(&img[row * S.H + col], bits) == kVisEmpty && bits < kVisEmpty) atomicAdd(&s_new, 1);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_new) atomicAdd(&vstats[0], (unsigned long long)s_new);   // one global atomic per workgroup
}

// One wave per live voxel (sel_slot of an "all voxels" selection, any order).  The voxel's points are taken in blocks of 64:
// a block is read into registers, every lane decides about its point, the survivors' positions are the running base plus the
// prefix popcount of the keep ballot.  A survivor's write position never passes its read position and a block is read before
// anything of it is written (the store addresses depend on the ballot, which depends on every lane's loads), so the
// compaction is in place.  No LDS, no per-thread arrays.
__global__ __launch_bounds__(64) void k_vis_clear(unsigned long long* __restrict__ keys, int* __restrict__ counts, float* pts,
                                                  int max_points, const unsigned long long* __restrict__ sel_key,
                                                  const unsigned int* __restrict__ sel_slot, MapPose pose, svnicp::RangeSensor S, VisOpt O,
                                                  const unsigned int* __restrict__ img, int* __restrict__ stats,
                                                  unsigned long long* __restrict__ vstats) {
  const int j = blockIdx.x, lane = threadIdx.x;
  if (sel_key[j] == kEmpty) return;   // an entry the selection did not fill (workgroup-uniform)
  const unsigned int slot = sel_slot[j];
  int cnt = counts[slot];
  cnt = cnt > max_points ? max_points : cnt;
  float* P = pts + (size_t)slot * max_points * 3;
  int base = 0, tested = 0;
  for (int b0 = 0; b0 < cnt; b0 += 64) {
    const int i = b0 + lane;
    const bool have = i < cnt;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (have) { x = P[3 * i]; y = P[3 * i + 1]; z = P[3 * i + 2]; }
    bool test = false, remove = false;
    if (have) {
      const double d0 = (double)x - pose.t[0], d1 = (double)y - pose.t[1], d2 = (double)z - pose.t[2];
      const float s0 = (float)((pose.R[0] * d0 + pose.R[3] * d1) + pose.R[6] * d2);   // R^T d, rounded once
      const float s1 = (float)((pose.R[1] * d0 + pose.R[4] * d1) + pose.R[7] * d2);
      const float s2 = (float)((pose.R[2] * d0 + pose.R[5] * d1) + pose.R[8] * d2);
      int row, col;
      float rm;
      if (svnicp::range_project(s0, s1, s2, S, row, col, rm) && !(rm > O.max_range) && img[row * S.H + col] < kVisEmpty) {
        const int r_lo = row - O.wr < 0 ? 0 : row - O.wr, r_hi = row + O.wr > S.N - 1 ? S.N - 1 : row + O.wr;   // rows do not wrap
        unsigned int mn = kVisEmpty;
        for (int rr = r_lo; rr <= r_hi; ++rr)
          for (int dc = -O.wc; dc <= O.wc; ++dc) {
            int cc = (col + dc) % S.H;   // columns wrap (|dc| may exceed a tiny H: a true modulo)
            if (cc < 0) cc += S.H;
            const unsigned int v = img[rr * S.H + cc];
            mn = v < mn ? v : mn;
          }
        const float r_min = __uint_as_float(mn);   // finite: the own pixel is in the window
        test = true;
        remove = rm < r_min - fmaxf(O.margin_abs, O.margin_rel * r_min);
      }
    }
    const bool keep = have && !remove;
    const unsigned long long km = __ballot(keep);
    const int pos = base + lanes_below(km);
    if (keep && pos != i) { P[3 * pos] = x; P[3 * pos + 1] = y; P[3 * pos + 2] = z; }
    base += __popcll(km);
    tested += __popcll(__ballot(test));
  }
  if (lane == 0) {
    if (base != cnt) {
      counts[slot] = base;
      atomicAdd(&vstats[2], (unsigned long long)(cnt - base));
      if (base == 0) {   // a tombstone, as k_map_remove_far makes one
        keys[slot] = kTomb;
        atomicSub(&stats[0], 1); atomicAdd(&stats[1], 1);
        atomicAdd(&vstats[3], 1ull);
      }
    }
    if (tested) atomicAdd(&vstats[1], (unsigned long long)tested);
  }
}

}  // namespace

struct svnicp_map {
  int device = 0;
  svnicp_host::Stream stream;   // before the buffers: destroyed after them
  double voxel = 1.0, max_range = 80.0;
  int max_points = 20;
  int64_t cap = 0;
  GrowBuf<unsigned long long> keys, sel_key, sel_key2;
  GrowBuf<int> counts, stats, sidx_in, sidx, sel_cnt, sel_off, nsel;
  GrowBuf<float> pts, q, in, out_f32;
  GrowBuf<unsigned int> slot, sslot, sel_slot, sel_slot2;
  GrowBuf<double> out, nrm;
  GrowBuf<unsigned char> tmp;
  GrowBuf<unsigned int> vis_img;           // svnicp_map_clear_seen_through: the minimum-range image (float bit patterns)
  GrowBuf<unsigned long long> vis_stats;   // ... and its four statistics
  // svnicp_map_score_poses: its own rows, poses, chunk records and results (the query's buffers are not touched)
  GrowBuf<float> sc_in;
  GrowBuf<double> sc_poses, sc_psum, sc_out;
  GrowBuf<unsigned int> sc_pcnt;
  int64_t sc_C = 0;      // poses of the last scoring (0 before one)
  // svnicp_map_search_poses: its own rows, the lattice vectors, poses and records of EVERY level (the tap reads them), the kept
  // lists (kSearchMaxKeep indices per level), its own chunk records, and the staging block the host reads with one copy
  GrowBuf<float> se_in;
  GrowBuf<int32_t> se_lat, se_kept;
  GrowBuf<double> se_poses, se_rec, se_psum, se_stage;
  GrowBuf<unsigned int> se_pcnt;
  std::vector<double> se_host;       // the staging block of the last search, as map_search.hpp lays it out
  svnicp::MapSearchPlan se_plan{};   // the last search's lattice (se_done says whether there is one)
  bool se_done = false;
  int64_t last_M = 0;
  // svnicp_map_query_normals: the last query's selection (sel_key2 / sel_off / sel_cnt over last_live entries) still describes
  // the table — set by svnicp_map_query, dropped by svnicp_map_add_cloud, svnicp_map_clear_seen_through and svnicp_map_clear
  bool query_valid = false;
  int64_t last_live = 0;
  int64_t nrm_M = 0;     // rows of nrm that belong to the last query (0 until svnicp_map_query_normals ran for it)
  int64_t skipped = 0;   // points svnicp_map_add_cloud did not store (outside the index range or NaN), since creation / clear
  int64_t rebuilds = 0;  // rebuild() calls since creation (svnicp_map_table_info)
  int h_stats[4] = {0, 0, 0, 0};
  std::string err;
  static std::string& create_error() { thread_local std::string s; return s; }   // svnicp_map_last_error(nullptr)
};

namespace {
// k_map_normals' d² tile and dynamic LDS for a map of max_points points per voxel (at most 91.6 KB, at 256)
int normals_tile(int max_points) { const int block = 27 * max_points; return block < kNrmTile ? (block + 63) / 64 * 64 : kNrmTile; }
size_t normals_lds(int max_points) {
  return (size_t)(64 + normals_tile(max_points)) * (sizeof(double) + sizeof(unsigned short)) + (size_t)27 * max_points * 3 * sizeof(float);
}

int alloc_table(svnicp_map* m, int64_t cap, GrowBuf<unsigned long long>& keys, GrowBuf<int>& counts, GrowBuf<float>& pts) {
  HIPCHK(m, keys.ensure((size_t)cap));
  HIPCHK(m, counts.ensure((size_t)cap));
  HIPCHK(m, pts.ensure((size_t)cap * m->max_points * 3));
  HIPCHK(m, hipMemsetAsync(keys.p, 0xff, (size_t)cap * 8, m->stream));
  HIPCHK(m, hipMemsetAsync(counts.p, 0, (size_t)cap * 4, m->stream));
  return 0;
}

int read_stats(svnicp_map* m) {
  HIPCHK(m, hipMemcpyAsync(m->h_stats, m->stats.p, sizeof m->h_stats, hipMemcpyDeviceToHost, m->stream));
  HIPCHK(m, hipStreamSynchronize(m->stream));
  return 0;
}

int rebuild(svnicp_map* m, int64_t new_cap) {
  GrowBuf<unsigned long long> nk; GrowBuf<int> nc; GrowBuf<float> np;
  int rc = alloc_table(m, new_cap, nk, nc, np);
  if (rc) return rc;
  hipLaunchKernelGGL(k_map_rehash, dim3((unsigned)((m->cap + 255) / 256)), dim3(256), 0, m->stream, m->keys.p, m->counts.p, m->pts.p,
                     m->cap, m->max_points, nk.p, nc.p, np.p, new_cap, m->stats.p);
  HIPCHK(m, hipGetLastError());
  const int zero = 0;
  HIPCHK(m, hipMemcpyAsync(m->stats.p + 1, &zero, sizeof(int), hipMemcpyHostToDevice, m->stream));   // no tombstones left
  HIPCHK(m, hipStreamSynchronize(m->stream));
  m->keys = std::move(nk); m->counts = std::move(nc); m->pts = std::move(np);
  m->cap = new_cap;
  ++m->rebuilds;
  return 0;
}
}  // namespace

extern "C" {

const char* svnicp_map_last_error(const svnicp_map* m) { return m ? m->err.c_str() : svnicp_map::create_error().c_str(); }

int svnicp_map_create(int device, double voxel_size, double max_range, int max_points, int64_t capacity_voxels, svnicp_map** out) {
  if (!out || !(voxel_size > 0) || max_points < 1 || max_points > 256)
    return fail<svnicp_map>(nullptr, SVNICP_ERR_INVALID, "svnicp_map_create: need voxel_size > 0 and 1 <= max_points <= 256");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail<svnicp_map>(nullptr, SVNICP_ERR_NO_DEVICE, "svnicp_map_create: no HIP device visible (this library has no CPU path)");
  if (device < 0 || device >= ndev) return fail<svnicp_map>(nullptr, SVNICP_ERR_INVALID, "svnicp_map_create: bad device ordinal");
  if (hipSetDevice(device) != hipSuccess) return fail<svnicp_map>(nullptr, SVNICP_ERR_HIP, "hipSetDevice failed");
  svnicp_map* m = new svnicp_map();
  m->device = device; m->voxel = voxel_size; m->max_range = max_range; m->max_points = max_points;
  int64_t cap = 1 << 16;
  const int64_t want = capacity_voxels > 0 ? capacity_voxels : (int64_t)1 << 20;
  while (cap < want) cap <<= 1;
  m->cap = cap;
  if (m->stream.create(hipStreamNonBlocking) != hipSuccess) { delete m; return fail<svnicp_map>(nullptr, SVNICP_ERR_HIP, "hipStreamCreate failed"); }
  int rc = alloc_table(m, cap, m->keys, m->counts, m->pts);
  if (!rc && (m->stats.ensure(4) != hipSuccess || m->nsel.ensure(1) != hipSuccess)) rc = SVNICP_ERR_NOMEM;
  if (!rc && hipMemsetAsync(m->stats.p, 0, 16, m->stream) != hipSuccess) rc = SVNICP_ERR_HIP;
  if (!rc && hipStreamSynchronize(m->stream) != hipSuccess) rc = SVNICP_ERR_HIP;
  if (!rc && normals_lds(max_points) > 48 * 1024 &&   // once per process and size class, not per svnicp_map_query_normals
      hipFuncSetAttribute(reinterpret_cast<const void*>(k_map_normals), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess)
    rc = SVNICP_ERR_HIP;
  if (rc) { svnicp_map::create_error() = m->err.empty() ? "svnicp_map_create: allocation failed" : m->err; svnicp_map_destroy(m); return rc; }
  *out = m;
  return SVNICP_OK;
}

void svnicp_map_destroy(svnicp_map* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  delete m;
}

int svnicp_map_clear(svnicp_map* m) {
  if (!m) return SVNICP_ERR_INVALID;
  HIPCHK(m, hipSetDevice(m->device));
  HIPCHK(m, hipMemsetAsync(m->keys.p, 0xff, (size_t)m->cap * 8, m->stream));
  HIPCHK(m, hipMemsetAsync(m->counts.p, 0, (size_t)m->cap * 4, m->stream));
  HIPCHK(m, hipMemsetAsync(m->stats.p, 0, 16, m->stream));
  HIPCHK(m, hipStreamSynchronize(m->stream));
  std::memset(m->h_stats, 0, sizeof m->h_stats);
  m->skipped = 0;
  m->query_valid = false; m->nrm_M = 0;
  return SVNICP_OK;
}

int svnicp_map_skipped_points(svnicp_map* m, int64_t* out) {
  if (!m || !out) return SVNICP_ERR_INVALID;
  *out = m->skipped;
  return SVNICP_OK;
}

int svnicp_map_table_info(svnicp_map* m, int64_t* capacity_slots, int64_t* tombstones, int64_t* rebuilds) {
  if (!m) return SVNICP_ERR_INVALID;
  if (capacity_slots) *capacity_slots = m->cap;
  if (tombstones) *tombstones = m->h_stats[1];
  if (rebuilds) *rebuilds = m->rebuilds;
  return SVNICP_OK;
}

int svnicp_map_size(svnicp_map* m, int64_t* voxels) {
  if (!m || !voxels) return SVNICP_ERR_INVALID;
  HIPCHK(m, hipSetDevice(m->device));
  const int rc = read_stats(m);
  if (rc) return rc;
  *voxels = m->h_stats[0];
  return SVNICP_OK;
}

int svnicp_map_add_cloud(svnicp_map* m, const float* xyz, int64_t n, int mem_kind, const double R_rowmajor[9], const double t[3]) {
  if (!m || !R_rowmajor || !t || n < 0 || (n > 0 && !xyz) || n > 0x7fffffffLL) return fail(m, SVNICP_ERR_INVALID, "svnicp_map_add_cloud: bad argument");
  HIPCHK(m, hipSetDevice(m->device));
  m->query_valid = false; m->nrm_M = 0;
  if (n > 0) {
    // room for this cloud in the worst case (every point a new voxel): keep the load factor below 1/2, clear tombstones
    int rc = read_stats(m);
    if (rc) return rc;
    int64_t need = m->cap;
    while ((int64_t)(m->h_stats[0] + n) * 2 > need) need <<= 1;
    if (need != m->cap || (int64_t)m->h_stats[1] * 4 > m->cap) { rc = rebuild(m, need); if (rc) return rc; }
    const float* din = xyz;
    if (mem_kind != SVNICP_MEM_DEVICE) {
      HIPCHK(m, m->in.ensure((size_t)n * 3));
      HIPCHK(m, hipMemcpyAsync(m->in.p, xyz, (size_t)n * 12, hipMemcpyHostToDevice, m->stream));
      din = m->in.p;
    }
    HIPCHK(m, m->q.ensure((size_t)n * 3)); HIPCHK(m, m->slot.ensure((size_t)n)); HIPCHK(m, m->sslot.ensure((size_t)n));
    HIPCHK(m, m->sidx_in.ensure((size_t)n)); HIPCHK(m, m->sidx.ensure((size_t)n));
    MapPose ps;
    for (int i = 0; i < 9; ++i) ps.R[i] = R_rowmajor[i];
    for (int i = 0; i < 3; ++i) ps.t[i] = t[i];
    const unsigned g = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_map_locate, dim3(g), dim3(256), 0, m->stream, din, n, ps, (float)m->voxel, m->keys.p, m->cap, m->q.p, m->slot.p, m->stats.p);
    HIPCHK(m, hipGetLastError());
    {  // stable sort of (slot, input index): a voxel's new points become a run in input order
      hipLaunchKernelGGL(k_map_iota, dim3(g), dim3(256), 0, m->stream, m->sidx_in.p, n);
      HIPCHK(m, hipGetLastError());
      size_t bytes = 0;
      HIPCHK(m, rocprim::radix_sort_pairs(nullptr, bytes, m->slot.p, m->sslot.p, m->sidx_in.p, m->sidx.p, (size_t)n, 0, 32, m->stream));
      HIPCHK(m, m->tmp.ensure(bytes));
      HIPCHK(m, rocprim::radix_sort_pairs(m->tmp.p, bytes, m->slot.p, m->sslot.p, m->sidx_in.p, m->sidx.p, (size_t)n, 0, 32, m->stream));
    }
    hipLaunchKernelGGL(k_map_place, dim3(g), dim3(256), 0, m->stream, m->sslot.p, m->sidx.p, n, m->counts.p, m->max_points, m->q.p, m->pts.p);
    HIPCHK(m, hipGetLastError());
    hipLaunchKernelGGL(k_map_count, dim3(g), dim3(256), 0, m->stream, m->sslot.p, n, m->counts.p, m->max_points, m->stats.p);
    HIPCHK(m, hipGetLastError());
  }
  hipLaunchKernelGGL(k_map_remove_far, dim3((unsigned)((m->cap + 255) / 256)), dim3(256), 0, m->stream, m->keys.p, m->counts.p, m->pts.p,
                     m->cap, m->max_points, t[0], t[1], t[2], m->max_range * m->max_range, m->stats.p);
  HIPCHK(m, hipGetLastError());
  const int rc = read_stats(m);
  if (rc) return rc;
  if (m->h_stats[2] || m->h_stats[3]) {
    const int flags = m->h_stats[2], zero2[2] = {0, 0};
    m->skipped += m->h_stats[3];    // points outside +-2^20 voxels or NaN: not stored, not an error — the map and its
                                    // counters are consistent, the caller's drive goes on (svnicp_map_skipped_points)
    HIPCHK(m, hipMemcpyAsync(m->stats.p + 2, zero2, sizeof zero2, hipMemcpyHostToDevice, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    // cannot happen: the table is grown to twice the voxels this cloud could add before anything is inserted
    if (flags & 2) return fail(m, SVNICP_ERR_NOMEM, "svnicp_map_add_cloud: hash table full");
  }
  return SVNICP_OK;
}

int svnicp_map_clear_seen_through(svnicp_map* m, const float* scan_xyz, int64_t n, int mem_kind, const double R_rowmajor[9], const double t[3],
                                  const svnicp_seg_params* sensor, const svnicp_visibility_opt* opt, svnicp_visibility_stats* out) {
  if (!m) return SVNICP_ERR_INVALID;
  if (!R_rowmajor || !t || !sensor || !opt || !out || n < 0 || (n > 0 && !scan_xyz) || n > 0x7fffffffLL)
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_clear_seen_through: bad argument");
  if (sensor->struct_size != (int32_t)sizeof(svnicp_seg_params) || opt->struct_size != (int32_t)sizeof(svnicp_visibility_opt))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_clear_seen_through: struct_size != sizeof(svnicp_seg_params) / sizeof(svnicp_visibility_opt)");
  if (!(sensor->n_scan >= 1 && sensor->n_scan <= 128 && sensor->horizon_scan >= 1 &&
        (int64_t)sensor->n_scan * sensor->horizon_scan <= (int64_t)1 << 19))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_clear_seen_through: need 1 <= n_scan <= 128, horizon_scan >= 1 and n_scan * horizon_scan <= 2^19");
  if (!(std::isfinite(sensor->ang_res_x) && sensor->ang_res_x > 0.0f && std::isfinite(sensor->ang_res_y) && sensor->ang_res_y > 0.0f &&
        std::isfinite(sensor->ang_bottom) && std::isfinite(sensor->min_range)))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_clear_seen_through: ang_res_x / ang_res_y must be finite and positive, ang_bottom / min_range finite");
  if (!(opt->window_rows >= 0 && opt->window_rows <= 4 && opt->window_cols >= 0 && opt->window_cols <= 8))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_clear_seen_through: window_rows must be 0..4 and window_cols 0..8");
  if (!(std::isfinite(opt->margin_abs) && opt->margin_abs >= 0.0f && std::isfinite(opt->margin_rel) && opt->margin_rel >= 0.0f))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_clear_seen_through: margin_abs / margin_rel must be finite and >= 0");
  if (!(std::isfinite(opt->max_range) && opt->max_range > 0.0f))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_clear_seen_through: max_range must be finite and > 0");
  HIPCHK(m, hipSetDevice(m->device));
  m->query_valid = false; m->nrm_M = 0;
  *out = svnicp_visibility_stats{0, 0, 0, 0};
  // every call that changes the map ends by reading the statistics: the live voxels are known without asking the device
  const int64_t live = m->h_stats[0] > 0 ? m->h_stats[0] : 0;
  if (n == 0 || live == 0) return SVNICP_OK;
  const svnicp::RangeSensor S{sensor->n_scan, sensor->horizon_scan, sensor->ang_res_x, sensor->ang_res_y, sensor->ang_bottom, sensor->min_range};
  const VisOpt O{opt->window_rows, opt->window_cols, opt->margin_abs, opt->margin_rel, opt->max_range};
  const int64_t npix = (int64_t)S.N * S.H;
  const float* din = scan_xyz;
  if (mem_kind != SVNICP_MEM_DEVICE) {
    HIPCHK(m, m->in.ensure((size_t)n * 3));
    HIPCHK(m, hipMemcpyAsync(m->in.p, scan_xyz, (size_t)n * 12, hipMemcpyHostToDevice, m->stream));
    din = m->in.p;
  }
  HIPCHK(m, m->vis_img.ensure((size_t)npix)); HIPCHK(m, m->vis_stats.ensure(4));
  HIPCHK(m, m->sel_key.ensure((size_t)live)); HIPCHK(m, m->sel_slot.ensure((size_t)live));
  MapPose ps;
  for (int i = 0; i < 9; ++i) ps.R[i] = R_rowmajor[i];
  for (int i = 0; i < 3; ++i) ps.t[i] = t[i];
  const int64_t nfill = npix > live ? npix : live;
  hipLaunchKernelGGL(k_vis_fill, dim3((unsigned)((nfill + 255) / 256)), dim3(256), 0, m->stream, m->vis_img.p, npix, m->sel_key.p, live, m->nsel.p,
                     m->vis_stats.p);
  // every live voxel (r2 < 0), in any order: each is handled by itself
  hipLaunchKernelGGL(k_map_select, dim3((unsigned)((m->cap + kSelChunk * 256 - 1) / (kSelChunk * 256))), dim3(256), 0, m->stream, m->keys.p, m->counts.p,
                     m->pts.p, m->cap, m->max_points, 0.0, 0.0, 0.0, -1.0, m->sel_key.p, m->sel_slot.p, m->nsel.p, (int)live);
  hipLaunchKernelGGL(k_vis_image, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->stream, din, n, S, m->vis_img.p, m->vis_stats.p);
  hipLaunchKernelGGL(k_vis_clear, dim3((unsigned)live), dim3(64), 0, m->stream, m->keys.p, m->counts.p, m->pts.p, m->max_points, m->sel_key.p,
                     m->sel_slot.p, ps, S, O, m->vis_img.p, m->stats.p, m->vis_stats.p);
  HIPCHK(m, hipGetLastError());
  unsigned long long vs[4] = {0, 0, 0, 0};
  HIPCHK(m, hipMemcpyAsync(vs, m->vis_stats.p, sizeof vs, hipMemcpyDeviceToHost, m->stream));
  const int rc = read_stats(m);   // the only host synchronisation: live voxels and tombstones as the next call needs them
  if (rc) return rc;
  out->pixels_filled = (int64_t)vs[0]; out->points_tested = (int64_t)vs[1];
  out->points_removed = (int64_t)vs[2]; out->voxels_emptied = (int64_t)vs[3];
  return SVNICP_OK;
}

int svnicp_map_query(svnicp_map* m, const double center[3], double max_range, int64_t* count_out) {
  if (!m || !count_out) return SVNICP_ERR_INVALID;
  HIPCHK(m, hipSetDevice(m->device));
  const double r2 = (center && max_range >= 0.0) ? max_range * max_range : -1.0;
  const double c0 = center ? center[0] : 0.0, c1 = center ? center[1] : 0.0, c2 = center ? center[2] : 0.0;
  // Everything is sized by the number of live voxels the host already knows (every call that changes the map ends by
  // reading the statistics), so the whole query is queued without looking at intermediate counts and synchronises once:
  // unselected entries keep the key ~0, sort to the end and count zero points.
  const size_t live = (size_t)(m->h_stats[0] > 0 ? m->h_stats[0] : 0);
  *count_out = 0; m->last_M = 0;
  m->query_valid = false; m->nrm_M = 0; m->last_live = (int64_t)live;
  if (live == 0) { m->query_valid = true; return SVNICP_OK; }
  HIPCHK(m, m->sel_key.ensure(live)); HIPCHK(m, m->sel_key2.ensure(live)); HIPCHK(m, m->sel_slot.ensure(live)); HIPCHK(m, m->sel_slot2.ensure(live));
  HIPCHK(m, m->sel_cnt.ensure(live)); HIPCHK(m, m->sel_off.ensure(live));
  HIPCHK(m, m->out.ensure(live * (size_t)m->max_points * 3));
  size_t b1 = 0, b2 = 0;
  HIPCHK(m, rocprim::radix_sort_pairs(nullptr, b1, m->sel_key.p, m->sel_key2.p, m->sel_slot.p, m->sel_slot2.p, live, 0, 64, m->stream));
  HIPCHK(m, rocprim::exclusive_scan(nullptr, b2, m->sel_cnt.p, m->sel_off.p, 0, live, rocprim::plus<int>(), m->stream));
  HIPCHK(m, m->tmp.ensure(b1 > b2 ? b1 : b2));
  HIPCHK(m, hipMemsetAsync(m->nsel.p, 0, sizeof(int), m->stream));
  HIPCHK(m, hipMemsetAsync(m->sel_key.p, 0xff, live * sizeof(unsigned long long), m->stream));
  HIPCHK(m, hipMemsetAsync(m->sel_slot.p, 0, live * sizeof(unsigned int), m->stream));
  hipLaunchKernelGGL(k_map_select, dim3((unsigned)((m->cap + kSelChunk * 256 - 1) / (kSelChunk * 256))), dim3(256), 0, m->stream, m->keys.p, m->counts.p, m->pts.p, m->cap,
                     m->max_points, c0, c1, c2, r2, m->sel_key.p, m->sel_slot.p, m->nsel.p, (int)live);
  HIPCHK(m, hipGetLastError());
  HIPCHK(m, rocprim::radix_sort_pairs(m->tmp.p, b1, m->sel_key.p, m->sel_key2.p, m->sel_slot.p, m->sel_slot2.p, live, 0, 64, m->stream));
  const int nl = (int)live;
  hipLaunchKernelGGL(k_map_sel_counts, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, m->stream, m->sel_key2.p, m->sel_slot2.p, nl, m->counts.p, m->sel_cnt.p);
  HIPCHK(m, hipGetLastError());
  HIPCHK(m, rocprim::exclusive_scan(m->tmp.p, b2, m->sel_cnt.p, m->sel_off.p, 0, live, rocprim::plus<int>(), m->stream));
  const int64_t work = (int64_t)live * m->max_points;
  hipLaunchKernelGGL(k_map_gather, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, m->stream, m->sel_slot2.p, m->sel_off.p, m->sel_cnt.p, nl,
                     m->max_points, m->pts.p, m->out.p, (float*)nullptr);
  HIPCHK(m, hipGetLastError());
  int last[2] = {0, 0};
  HIPCHK(m, hipMemcpyAsync(&last[0], m->sel_off.p + (live - 1), sizeof(int), hipMemcpyDeviceToHost, m->stream));
  HIPCHK(m, hipMemcpyAsync(&last[1], m->sel_cnt.p + (live - 1), sizeof(int), hipMemcpyDeviceToHost, m->stream));
  HIPCHK(m, hipStreamSynchronize(m->stream));   // the rows are complete when the call returns (another stream may read them)
  const int64_t M = (int64_t)last[0] + last[1];
  m->last_M = M;
  m->query_valid = true;
  *count_out = M;
  return SVNICP_OK;
}

int svnicp_map_query_normals(svnicp_map* m, int normal_k, int64_t* with_normal_out) {
  if (!m) return SVNICP_ERR_INVALID;
  if (with_normal_out) *with_normal_out = 0;
  if (!m->query_valid)
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_query_normals: no svnicp_map_query yet, or the map changed (add_cloud / clear_seen_through / clear) since the last one");
  const int kn = normal_k ? normal_k : 16;
  if (kn < 4 || kn > 64) return fail(m, SVNICP_ERR_INVALID, "svnicp_map_query_normals: normal_k must be 4..64 (0 = 16)");
  HIPCHK(m, hipSetDevice(m->device));
  m->nrm_M = 0;
  if (m->last_M == 0) return SVNICP_OK;   // an empty selection: nothing to write
  HIPCHK(m, m->nrm.ensure((size_t)m->last_M * 3));
  const int tile = normals_tile(m->max_points);
  const size_t smem = normals_lds(m->max_points);
  HIPCHK(m, hipMemsetAsync(m->nsel.p, 0, sizeof(int), m->stream));   // the query's counter, free again: here the rows with a normal
  hipLaunchKernelGGL(k_map_normals, dim3((unsigned)m->last_live), dim3(64), smem, m->stream, m->keys.p, m->counts.p, m->pts.p, m->cap,
                     m->max_points, m->sel_key2.p, m->sel_slot2.p, m->sel_off.p, m->sel_cnt.p, (int)m->last_live, kn, tile, m->nrm.p, m->nsel.p);
  HIPCHK(m, hipGetLastError());
  int with = 0;
  HIPCHK(m, hipMemcpyAsync(&with, m->nsel.p, sizeof(int), hipMemcpyDeviceToHost, m->stream));
  HIPCHK(m, hipStreamSynchronize(m->stream));   // complete when the call returns, like the query
  m->nrm_M = m->last_M;
  if (with_normal_out) *with_normal_out = with;
  return SVNICP_OK;
}

void* svnicp_map_normals_devptr(svnicp_map* m) { return m && m->nrm_M > 0 ? (void*)m->nrm.p : nullptr; }

int svnicp_map_download_normals(svnicp_map* m, double* out_xyz, int64_t cap_points, int64_t* n_out) {
  if (!m || !n_out) return SVNICP_ERR_INVALID;
  HIPCHK(m, hipSetDevice(m->device));
  *n_out = m->nrm_M;
  const int64_t n = m->nrm_M < cap_points ? m->nrm_M : cap_points;
  if (n > 0 && out_xyz) {
    HIPCHK(m, hipMemcpyAsync(out_xyz, m->nrm.p, (size_t)n * 24, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
  }
  return SVNICP_OK;
}

int svnicp_map_score_poses(svnicp_map* m, const float* src_xyz, int64_t n, int src_mem_kind, const double* posesCx12, int64_t C,
                           int poses_mem_kind, double max_corr_dist, double* outCx4) {
  if (!m) return SVNICP_ERR_INVALID;
  if (n < 0 || n > 0x7fffffffLL || (n > 0 && !src_xyz))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_score_poses: need 0 <= n <= 2^31-1 and rows for n > 0");
  if (!posesCx12 || C < 1 || C > ((int64_t)1 << 20))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_score_poses: need poses and 1 <= C <= 2^20");
  if (!(std::isfinite(max_corr_dist) && max_corr_dist > 0.0 && max_corr_dist <= m->voxel))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_score_poses: max_corr_dist must be finite, > 0 and <= voxel_size (the 3x3x3 block "
                                       "holds the nearest point only up to that gate)");
  HIPCHK(m, hipSetDevice(m->device));
  const double thr2 = max_corr_dist * max_corr_dist;
  const float* din = src_xyz;
  if (n > 0 && src_mem_kind != SVNICP_MEM_DEVICE) {
    HIPCHK(m, m->sc_in.ensure((size_t)n * 3));
    HIPCHK(m, hipMemcpyAsync(m->sc_in.p, src_xyz, (size_t)n * 12, hipMemcpyHostToDevice, m->stream));
    din = m->sc_in.p;
  }
  const double* dposes = posesCx12;
  if (poses_mem_kind != SVNICP_MEM_DEVICE) {
    HIPCHK(m, m->sc_poses.ensure((size_t)C * 12));
    HIPCHK(m, hipMemcpyAsync(m->sc_poses.p, posesCx12, (size_t)C * 96, hipMemcpyHostToDevice, m->stream));
    dposes = m->sc_poses.p;
  }
  const int64_t chunks = svnicp::map_score_chunks(n);
  const size_t recs = (size_t)(C < svnicp::kScorePoseBatch ? C : svnicp::kScorePoseBatch) * (size_t)chunks;
  m->sc_C = 0;
  HIPCHK(m, m->sc_out.ensure((size_t)C * SVNICP_MAP_SCORE_FIELDS));
  HIPCHK(m, m->sc_pcnt.ensure(2 * recs)); HIPCHK(m, m->sc_psum.ensure(recs));
  const svnicp::MapTableView T{m->keys.p, m->counts.p, m->pts.p, m->cap, m->max_points, (float)m->voxel};
  HIPCHK(m, svnicp::launch_map_score(T, din, n, dposes, C, thr2, m->sc_pcnt.p, m->sc_psum.p, m->sc_out.p, m->stream));
  if (outCx4) HIPCHK(m, hipMemcpyAsync(outCx4, m->sc_out.p, (size_t)C * SVNICP_MAP_SCORE_FIELDS * 8, hipMemcpyDeviceToHost, m->stream));
  HIPCHK(m, hipStreamSynchronize(m->stream));   // complete when the call returns: the caller's rows and poses are free again
  m->sc_C = C;
  return SVNICP_OK;
}

void* svnicp_map_scores_devptr(svnicp_map* m) { return m && m->sc_C > 0 ? (void*)m->sc_out.p : nullptr; }

int svnicp_map_search_poses(svnicp_map* m, const float* src_xyz, int64_t n, int src_mem_kind, const double* guess_R, const double* guess_t,
                            const svnicp_map_search_opt* opt, svnicp_map_search* out) {
  if (!m) return SVNICP_ERR_INVALID;
  if (!guess_R || !guess_t || !opt || !out)
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_search_poses: guess_R, guess_t, opt and out must not be NULL");
  if (n < 0 || n > 0x7fffffffLL || (n > 0 && !src_xyz))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_search_poses: need 0 <= n <= 2^31-1 and rows for n > 0");
  if (!(std::isfinite(opt->max_corr_dist) && opt->max_corr_dist > 0.0 && opt->max_corr_dist <= m->voxel))
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_search_poses: max_corr_dist must be finite, > 0 and <= voxel_size (the 3x3x3 block "
                                       "holds the nearest point only up to that gate)");
  svnicp::MapSearchPlan P{};
  if (const char* why = svnicp::plan_map_search(opt->extent, opt->step, opt->levels, opt->keep, P))
    return fail(m, SVNICP_ERR_INVALID, std::string("svnicp_map_search_poses: ") + why);
  for (int j = 0; j < 12; ++j) {
    P.grid.G[j] = j < 9 ? guess_R[j] : guess_t[j - 9];
    if (!std::isfinite(P.grid.G[j])) return fail(m, SVNICP_ERR_INVALID, "svnicp_map_search_poses: the guess must be finite");
  }
  HIPCHK(m, hipSetDevice(m->device));
  m->se_done = false;
  const double thr2 = opt->max_corr_dist * opt->max_corr_dist;
  const float* din = src_xyz;
  if (n > 0 && src_mem_kind != SVNICP_MEM_DEVICE) {
    HIPCHK(m, m->se_in.ensure((size_t)n * 3));
    HIPCHK(m, hipMemcpyAsync(m->se_in.p, src_xyz, (size_t)n * 12, hipMemcpyHostToDevice, m->stream));
    din = m->se_in.p;
  }
  // every buffer at its final size before the first launch: growing one would drop the levels it already holds
  const int64_t chunks = svnicp::map_score_chunks(n);
  const size_t recs = (size_t)(P.max_count < svnicp::kScorePoseBatch ? P.max_count : svnicp::kScorePoseBatch) * (size_t)chunks;
  const int n_top = P.kept[P.levels - 1];
  const size_t stage_bytes = svnicp::map_search_stage_bytes(n_top);
  HIPCHK(m, m->se_lat.ensure((size_t)P.total * 6));
  HIPCHK(m, m->se_poses.ensure((size_t)P.total * 12));
  HIPCHK(m, m->se_rec.ensure((size_t)P.total * SVNICP_MAP_SCORE_FIELDS));
  HIPCHK(m, m->se_kept.ensure((size_t)svnicp::kSearchMaxLevels * svnicp::kSearchMaxKeep));
  HIPCHK(m, m->se_pcnt.ensure(2 * recs)); HIPCHK(m, m->se_psum.ensure(recs));
  HIPCHK(m, m->se_stage.ensure(stage_bytes / 8));
  HIPCHK(m, hipMemsetAsync(m->se_kept.p, 0, (size_t)svnicp::kSearchMaxLevels * svnicp::kSearchMaxKeep * 4, m->stream));
  const svnicp::MapTableView T{m->keys.p, m->counts.p, m->pts.p, m->cap, m->max_points, (float)m->voxel};
  for (int l = 0; l < P.levels; ++l) {   // per level: nodes, score (one or two launches per 32768 poses), rank
    int32_t* lat = m->se_lat.p + 6 * P.first[l];
    double* poses = m->se_poses.p + 12 * P.first[l];
    double* rec = m->se_rec.p + SVNICP_MAP_SCORE_FIELDS * P.first[l];
    int32_t* kept = m->se_kept.p + (size_t)l * svnicp::kSearchMaxKeep;
    HIPCHK(m, svnicp::launch_map_search_nodes(P.grid, l, P.levels, P.count[l], l ? m->se_lat.p + 6 * P.first[l - 1] : nullptr,
                                              l ? kept - svnicp::kSearchMaxKeep : nullptr, lat, poses, m->stream));
    HIPCHK(m, svnicp::launch_map_score(T, din, n, poses, P.count[l], thr2, m->se_pcnt.p, m->se_psum.p, rec, m->stream));
    HIPCHK(m, svnicp::launch_map_search_rank(rec, lat, P.count[l], P.kept[l], kept, m->stream));
  }
  const int last = P.levels - 1;
  HIPCHK(m, svnicp::launch_map_search_gather(P.grid, m->se_lat.p + 6 * P.first[last], m->se_poses.p + 12 * P.first[last],
                                             m->se_rec.p + SVNICP_MAP_SCORE_FIELDS * P.first[last],
                                             m->se_kept.p + (size_t)last * svnicp::kSearchMaxKeep, n_top,
                                             m->se_rec.p + SVNICP_MAP_SCORE_FIELDS * P.zero_index, m->se_stage.p, m->stream));
  m->se_host.resize(stage_bytes / 8);
  HIPCHK(m, hipMemcpyAsync(m->se_host.data(), m->se_stage.p, stage_bytes, hipMemcpyDeviceToHost, m->stream));
  HIPCHK(m, hipStreamSynchronize(m->stream));   // complete when the call returns: the caller's rows are free again
  m->se_plan = P;
  m->se_done = true;
  std::memset(out, 0, sizeof *out);
  out->levels = P.levels; out->active_axes = P.active_axes; out->nodes_scored = P.total;
  for (int l = 0; l < P.levels; ++l) { out->level_count[l] = P.count[l]; out->level_kept[l] = P.kept[l]; }
  std::memcpy(out->fine_step, P.grid.fine, sizeof out->fine_step);
  const double* h = m->se_host.data();
  std::memcpy(out->zero_record, h, 4 * 8);
  std::memcpy(out->best_correction, h + 4, 6 * 8);
  std::memcpy(out->best_pose, h + 10, 12 * 8);
  std::memcpy(out->best_record, h + 22, 4 * 8);
  std::memcpy(out->best_lattice, h + 4 + svnicp::kSearchTopDoubles * n_top, 6 * 4);
  return SVNICP_OK;
}

int svnicp_map_search_top(svnicp_map* m, int cap, int32_t* latticeNx6, double* correctionsNx6, double* posesNx12, double* recordsNx4,
                          int* n_out) {
  if (!m) return SVNICP_ERR_INVALID;
  if (!m->se_done) return fail(m, SVNICP_ERR_INVALID, "svnicp_map_search_top: no successful svnicp_map_search_poses yet");
  if (cap < 0) return fail(m, SVNICP_ERR_INVALID, "svnicp_map_search_top: cap must be >= 0");
  const int n_top = m->se_plan.kept[m->se_plan.levels - 1];
  if (n_out) *n_out = n_top;
  const int k = cap < n_top ? cap : n_top;
  const double* h = m->se_host.data() + 4;
  const int32_t* hl = reinterpret_cast<const int32_t*>(h + svnicp::kSearchTopDoubles * n_top);
  for (int i = 0; i < k; ++i, h += svnicp::kSearchTopDoubles) {
    if (latticeNx6) std::memcpy(latticeNx6 + 6 * i, hl + 6 * i, 6 * 4);
    if (correctionsNx6) std::memcpy(correctionsNx6 + 6 * i, h, 6 * 8);
    if (posesNx12) std::memcpy(posesNx12 + 12 * i, h + 6, 12 * 8);
    if (recordsNx4) std::memcpy(recordsNx4 + 4 * i, h + 18, 4 * 8);
  }
  return SVNICP_OK;
}

int svnicp_map_search_level(svnicp_map* m, int level, int64_t cap, int32_t* latticeCx6, double* posesCx12, double* recordsCx4,
                            int32_t* kept_indices, int64_t* count_out, int* kept_out) {
  if (!m) return SVNICP_ERR_INVALID;
  if (!m->se_done) return fail(m, SVNICP_ERR_INVALID, "svnicp_map_search_level: no successful svnicp_map_search_poses yet");
  const svnicp::MapSearchPlan& P = m->se_plan;
  if (level < 0 || level >= P.levels || cap < 0)
    return fail(m, SVNICP_ERR_INVALID, "svnicp_map_search_level: need 0 <= level < levels of the last search and cap >= 0");
  HIPCHK(m, hipSetDevice(m->device));
  if (count_out) *count_out = P.count[level];
  if (kept_out) *kept_out = P.kept[level];
  const size_t c = (size_t)(cap < P.count[level] ? cap : P.count[level]);
  const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
  if (c && latticeCx6) HIPCHK(m, hipMemcpyAsync(latticeCx6, m->se_lat.p + 6 * P.first[level], c * 24, d2h, m->stream));
  if (c && posesCx12) HIPCHK(m, hipMemcpyAsync(posesCx12, m->se_poses.p + 12 * P.first[level], c * 96, d2h, m->stream));
  if (c && recordsCx4) HIPCHK(m, hipMemcpyAsync(recordsCx4, m->se_rec.p + 4 * P.first[level], c * 32, d2h, m->stream));
  if (kept_indices)
    HIPCHK(m, hipMemcpyAsync(kept_indices, m->se_kept.p + (size_t)level * svnicp::kSearchMaxKeep, (size_t)P.kept[level] * 4, d2h, m->stream));
  HIPCHK(m, hipStreamSynchronize(m->stream));
  return SVNICP_OK;
}

void* svnicp_map_points_devptr(svnicp_map* m) { return m ? (void*)m->out.p : nullptr; }

int svnicp_map_download(svnicp_map* m, double* out_xyz, int64_t cap_points, int64_t* n_out) {
  if (!m || !n_out) return SVNICP_ERR_INVALID;
  HIPCHK(m, hipSetDevice(m->device));
  *n_out = m->last_M;
  const int64_t n = m->last_M < cap_points ? m->last_M : cap_points;
  if (n > 0 && out_xyz) {
    HIPCHK(m, hipMemcpyAsync(out_xyz, m->out.p, (size_t)n * 24, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
  }
  return SVNICP_OK;
}

}  // extern "C"
