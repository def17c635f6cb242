// map_table.hip — the voxel map's hash table: insert, remove-far, select / gather and rebuild (the layout and the determinism
// argument are in voxel_map.hip's header comment, the design in DESIGN.md §4.4).  Device counterpart of svnicp::VoxelHashMap
// (VoxelHashMap.cpp:22-101 of the reference); the key packing, hash and read-only lookup are in voxel_table_device.hpp.
#include "map_table.hpp"

#include <utility>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "voxel_table_device.hpp"

namespace svnicp {
namespace {

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
  if (!ok) { slot_of[i] = kNoSlot; atomicAdd(&stats[kStatSkipped], 1); return; }   // outside the index range or NaN: counted, not stored
  const unsigned long long key = pack_key(v[0], v[1], v[2]);
  unsigned long long h = hash_key(key) & (unsigned long long)(cap - 1);
  for (int64_t probe = 0; probe < cap; ++probe) {   // bounded: a full table ends the loop and is reported
    unsigned long long cur = keys[h];
    if (cur == kEmpty) cur = atomicCAS(&keys[h], kEmpty, key);
    if (cur == key || cur == kEmpty) { slot_of[i] = (unsigned int)h; return; }
    h = (h + 1) & (unsigned long long)(cap - 1);
  }
  slot_of[i] = kNoSlot;
  atomicOr(&stats[kStatFlags], kFlagTableFull);
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
  if (s == kNoSlot) return;
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
    if (s != kNoSlot && (j == 0 || sslot[j - 1] != s)) {   // one thread per run
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
  if (threadIdx.x == 0 && s_new) atomicAdd(&stats[kStatLive], s_new);   // one global atomic per workgroup
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
    atomicSub(&stats[kStatLive], 1); atomicAdd(&stats[kStatTombs], 1);
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
                                                    const float* __restrict__ pts, double* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // one thread per (voxel, point slot)
  const int j = (int)(g / max_points), k = (int)(g % max_points);
  if (j >= nsel || k >= cnts[j]) return;
  const float* f = pts + ((size_t)sslot[j] * max_points + k) * 3;
  const size_t o = ((size_t)offs[j] + k) * 3;
  out[o] = (double)f[0]; out[o + 1] = (double)f[1]; out[o + 2] = (double)f[2];
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
  atomicOr(&stats[kStatFlags], kFlagTableFull);
}

hipError_t alloc_slots(int64_t cap, int max_points, GrowBuf<unsigned long long>& keys, GrowBuf<int>& counts, GrowBuf<float>& pts,
                       hipStream_t stream) {
  HIPTRY(keys.ensure((size_t)cap));
  HIPTRY(counts.ensure((size_t)cap));
  HIPTRY(pts.ensure((size_t)cap * max_points * 3));
  HIPTRY(hipMemsetAsync(keys.p, 0xff, (size_t)cap * 8, stream));
  return hipMemsetAsync(counts.p, 0, (size_t)cap * 4, stream);
}

}  // namespace

hipError_t map_table_alloc(MapTable& T, int64_t cap, int max_points, hipStream_t stream) {
  HIPTRY(alloc_slots(cap, max_points, T.keys, T.counts, T.pts, stream));
  T.cap = cap;
  return hipSuccess;
}

hipError_t map_table_clear(MapTable& T, hipStream_t stream) {
  HIPTRY(hipMemsetAsync(T.keys.p, 0xff, (size_t)T.cap * 8, stream));
  HIPTRY(hipMemsetAsync(T.counts.p, 0, (size_t)T.cap * 4, stream));
  HIPTRY(hipMemsetAsync(T.stats.p, 0, kMapStats * sizeof(int), stream));
  HIPTRY(hipStreamSynchronize(stream));
  for (int& s : T.h_stats) s = 0;
  T.skipped = 0;
  return hipSuccess;
}

hipError_t map_table_read_stats(MapTable& T, hipStream_t stream) {
  HIPTRY(hipMemcpyAsync(T.h_stats, T.stats.p, sizeof T.h_stats, hipMemcpyDeviceToHost, stream));
  return hipStreamSynchronize(stream);
}

hipError_t map_table_rebuild(MapTable& T, int max_points, int64_t new_cap, hipStream_t stream) {
  GrowBuf<unsigned long long> nk; GrowBuf<int> nc; GrowBuf<float> np;
  HIPTRY(alloc_slots(new_cap, max_points, nk, nc, np, stream));
  HIPTRY(launch_checked(k_map_rehash, dim3(blocks_of(T.cap)), dim3(256), 0, stream, T.keys.p, T.counts.p, T.pts.p, T.cap, max_points,
                        nk.p, nc.p, np.p, new_cap, T.stats.p));
  const int zero = 0;
  HIPTRY(hipMemcpyAsync(T.stats.p + kStatTombs, &zero, sizeof(int), hipMemcpyHostToDevice, stream));   // no tombstones left
  HIPTRY(hipStreamSynchronize(stream));
  T.keys = std::move(nk); T.counts = std::move(nc); T.pts = std::move(np);
  T.cap = new_cap;
  ++T.rebuilds;
  return hipSuccess;
}

hipError_t map_table_reserve(MapTable& T, int max_points, int64_t n, hipStream_t stream) {
  HIPTRY(map_table_read_stats(T, stream));
  int64_t need = T.cap;
  while ((int64_t)(T.h_stats[kStatLive] + n) * 2 > need) need <<= 1;
  if (need != T.cap || (int64_t)T.h_stats[kStatTombs] * 4 > T.cap) return map_table_rebuild(T, max_points, need, stream);
  return hipSuccess;
}

hipError_t map_table_insert(const MapTableMut& T, const float* in, int64_t n, const MapPose& pose, MapInsertScratch& S,
                            GrowBuf<unsigned char>& tmp, hipStream_t stream) {
  HIPTRY(S.q.ensure((size_t)n * 3)); HIPTRY(S.slot.ensure((size_t)n)); HIPTRY(S.sslot.ensure((size_t)n));
  HIPTRY(S.sidx_in.ensure((size_t)n)); HIPTRY(S.sidx.ensure((size_t)n));
  const dim3 g(blocks_of(n)), b(256);
  HIPTRY(launch_checked(k_map_locate, g, b, 0, stream, in, n, pose, T.voxel, T.keys, T.cap, S.q.p, S.slot.p, T.stats));
  {  // stable sort of (slot, input index): a voxel's new points become a run in input order
    HIPTRY(launch_checked(k_map_iota, g, b, 0, stream, S.sidx_in.p, n));
    size_t bytes = 0;
    HIPTRY(rocprim::radix_sort_pairs(nullptr, bytes, S.slot.p, S.sslot.p, S.sidx_in.p, S.sidx.p, (size_t)n, 0, 32, stream));
    HIPTRY(tmp.ensure(bytes));
    HIPTRY(rocprim::radix_sort_pairs(tmp.p, bytes, S.slot.p, S.sslot.p, S.sidx_in.p, S.sidx.p, (size_t)n, 0, 32, stream));
  }
  HIPTRY(launch_checked(k_map_place, g, b, 0, stream, S.sslot.p, S.sidx.p, n, T.counts, T.max_points, S.q.p, T.pts));
  return launch_checked(k_map_count, g, b, 0, stream, S.sslot.p, n, T.counts, T.max_points, T.stats);
}

hipError_t launch_map_remove_far(const MapTableMut& T, const double centre[3], double r2, hipStream_t stream) {
  return launch_checked(k_map_remove_far, dim3(blocks_of(T.cap)), dim3(256), 0, stream, T.keys, T.counts, T.pts, T.cap, T.max_points,
                        centre[0], centre[1], centre[2], r2, T.stats);
}

hipError_t map_table_take_flags(MapTable& T, hipStream_t stream, int* flags) {
  *flags = T.h_stats[kStatFlags];
  if (!T.h_stats[kStatFlags] && !T.h_stats[kStatSkipped]) return hipSuccess;
  T.skipped += T.h_stats[kStatSkipped];   // points outside +-2^20 voxels or NaN: not stored, not an error — the map and its
                                          // counters are consistent, the caller's drive goes on (svnicp_map_skipped_points)
  static_assert(kStatSkipped == kStatFlags + 1, "the two words are cleared with one copy");
  const int zero2[2] = {0, 0};
  HIPTRY(hipMemcpyAsync(T.stats.p + kStatFlags, zero2, sizeof zero2, hipMemcpyHostToDevice, stream));
  return hipStreamSynchronize(stream);
}

hipError_t launch_map_select(const MapTableView& T, double px, double py, double pz, double r2, unsigned long long* sel_key,
                             unsigned int* sel_slot, int* nsel, int limit, hipStream_t stream) {
  return launch_checked(k_map_select, dim3(blocks_of(T.cap, kSelChunk * 256)), dim3(256), 0, stream, T.keys, T.counts, T.pts, T.cap,
                        T.max_points, px, py, pz, r2, sel_key, sel_slot, nsel, limit);
}

hipError_t map_table_query(const MapTableView& T, double px, double py, double pz, double r2, size_t live, MapSelection& S,
                           GrowBuf<unsigned char>& tmp, hipStream_t stream, int64_t* rows) {
  // Everything is sized by the number of live voxels the host already knows (every call that changes the map ends by
  // reading the statistics), so the whole query is queued without looking at intermediate counts and synchronises once:
  // unselected entries keep the key ~0, sort to the end and count zero points.
  HIPTRY(S.key.ensure(live)); HIPTRY(S.key2.ensure(live)); HIPTRY(S.slot.ensure(live)); HIPTRY(S.slot2.ensure(live));
  HIPTRY(S.cnt.ensure(live)); HIPTRY(S.off.ensure(live));
  HIPTRY(S.out.ensure(live * (size_t)T.max_points * 3));
  size_t b1 = 0, b2 = 0;
  HIPTRY(rocprim::radix_sort_pairs(nullptr, b1, S.key.p, S.key2.p, S.slot.p, S.slot2.p, live, 0, 64, stream));
  HIPTRY(rocprim::exclusive_scan(nullptr, b2, S.cnt.p, S.off.p, 0, live, rocprim::plus<int>(), stream));
  HIPTRY(tmp.ensure(b1 > b2 ? b1 : b2));
  HIPTRY(hipMemsetAsync(S.nsel.p, 0, sizeof(int), stream));
  HIPTRY(hipMemsetAsync(S.key.p, 0xff, live * sizeof(unsigned long long), stream));
  HIPTRY(hipMemsetAsync(S.slot.p, 0, live * sizeof(unsigned int), stream));
  HIPTRY(launch_map_select(T, px, py, pz, r2, S.key.p, S.slot.p, S.nsel.p, (int)live, stream));
  HIPTRY(rocprim::radix_sort_pairs(tmp.p, b1, S.key.p, S.key2.p, S.slot.p, S.slot2.p, live, 0, 64, stream));
  const int nl = (int)live;
  HIPTRY(launch_checked(k_map_sel_counts, dim3(blocks_of(nl)), dim3(256), 0, stream, S.key2.p, S.slot2.p, nl, T.counts, S.cnt.p));
  HIPTRY(rocprim::exclusive_scan(tmp.p, b2, S.cnt.p, S.off.p, 0, live, rocprim::plus<int>(), stream));
  const int64_t work = (int64_t)live * T.max_points;
  HIPTRY(launch_checked(k_map_gather, dim3(blocks_of(work)), dim3(256), 0, stream, S.slot2.p, S.off.p, S.cnt.p, nl, T.max_points, T.pts,
                        S.out.p));
  int last[2] = {0, 0};
  HIPTRY(hipMemcpyAsync(&last[0], S.off.p + (live - 1), sizeof(int), hipMemcpyDeviceToHost, stream));
  HIPTRY(hipMemcpyAsync(&last[1], S.cnt.p + (live - 1), sizeof(int), hipMemcpyDeviceToHost, stream));
  HIPTRY(hipStreamSynchronize(stream));   // the rows are complete when the call returns (another stream may read them)
  *rows = (int64_t)last[0] + last[1];
  return hipSuccess;
}

}  // namespace svnicp
