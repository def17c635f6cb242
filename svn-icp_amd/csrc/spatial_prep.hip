// spatial_prep.hip — spatial ordering for the pruned stage-A kernel (knn_tiles.hip).
//
// Targets and (transformed) queries are sorted along a 30-bit Morton curve (a three-pass radix sort
// of this file, or rocPRIM's device radix sort; the pair loop, not the sort, is the hot op).  Targets are then stored tile-wise: 512
// consecutive curve points form a tile with a float32 bounding box rounded OUTWARD, so that a
// box-to-box / point-to-box distance is a rigorous lower bound of every pair distance inside.
// Nothing here changes results: the ordering only decides which tiles can be skipped.  Each tile is also written in
// tile-local float32 rows in MFMA A-operand order, for the scan kernel's pre-filter on the matrix pipe.
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "kernels.hpp"

namespace svnicp {

namespace {

// order-preserving map double -> uint64 (for atomicMin/atomicMax on signed values)
__device__ __forceinline__ unsigned long long enc_f64(double v) {
  const long long b = __double_as_longlong(v);
  return b < 0 ? ~(unsigned long long)b : ((unsigned long long)b | 0x8000000000000000ull);
}
__device__ __forceinline__ double dec_f64(unsigned long long e) {
  const unsigned long long b = (e & 0x8000000000000000ull) ? (e & 0x7fffffffffffffffull) : ~e;
  return __longlong_as_double((long long)b);
}
__device__ __forceinline__ float next_down(float f) {  // largest float < f (f finite)
  if (f == 0.0f) return -1.401298464e-45f;
  int b = __float_as_int(f);
  b += (f > 0.0f) ? -1 : 1;
  return __int_as_float(b);
}
__device__ __forceinline__ float next_up(float f) {
  if (f == 0.0f) return 1.401298464e-45f;
  int b = __float_as_int(f);
  b += (f > 0.0f) ? 1 : -1;
  return __int_as_float(b);
}
__device__ __forceinline__ float f32_floor(double v) { float f = (float)v; return ((double)f > v) ? next_down(f) : f; }
__device__ __forceinline__ float f32_ceil(double v) { float f = (float)v; return ((double)f < v) ? next_up(f) : f; }

// bbox[0..2] = min xyz, bbox[3..5] = max xyz (encoded); NaN coordinates are ignored
__global__ __launch_bounds__(256) void k_bbox(const double* __restrict__ pts, int64_t n, unsigned long long* __restrict__ bbox) {
  double lo[3] = {__builtin_huge_val(), __builtin_huge_val(), __builtin_huge_val()};
  double hi[3] = {-__builtin_huge_val(), -__builtin_huge_val(), -__builtin_huge_val()};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
    for (int d = 0; d < 3; ++d) { const double v = pts[3 * i + d]; lo[d] = fmin(lo[d], v); hi[d] = fmax(hi[d], v); }  // fmin/fmax skip NaN
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    for (int off = 32; off > 0; off >>= 1) {
      lo[d] = fmin(lo[d], __shfl_xor(lo[d], off, kWave));
      hi[d] = fmax(hi[d], __shfl_xor(hi[d], off, kWave));
    }
  }
  // one set of atomics per workgroup (same-address atomics from every wave serialise at L2)
  __shared__ double s_lo[4][3], s_hi[4][3];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) { s_lo[wave][d] = lo[d]; s_hi[wave][d] = hi[d]; }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int d = threadIdx.x;
    double l = s_lo[0][d], h = s_hi[0][d];
    for (int w = 1; w < 4; ++w) { l = fmin(l, s_lo[w][d]); h = fmax(h, s_hi[w][d]); }
    if (l <= h) { atomicMin(&bbox[d], enc_f64(l)); atomicMax(&bbox[3 + d], enc_f64(h)); }
  }
}


__device__ __forceinline__ unsigned int spread10(unsigned int v) {  // 10 bits -> every third bit
  v &= 0x3ffu;
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

// 30-bit Morton key of point i (optionally transformed by R0,t0) inside the encoded bbox
// (key_or: bits set in every key — bit 30 puts a joint sort's queries behind its targets)
// fill_ff[0, fill_words): set to -1 on the way, grid-stride (the tile kernels' chunk table, instead of a fill launch of its own)
__global__ void k_morton_keys(const double* __restrict__ pts, int64_t i0, int64_t n, int transform, Pose0 pose,
                              const unsigned long long* __restrict__ bbox, unsigned int* __restrict__ keys,
                              int32_t* __restrict__ vals, unsigned int key_or, int32_t* __restrict__ fill_ff, size_t fill_words) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t w = (size_t)e; w < fill_words; w += (size_t)gridDim.x * blockDim.x) fill_ff[w] = -1;
  if (e >= n) return;
  const int64_t i = i0 + e;
  double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
  if (transform) {
    double x, y, z;
    stage_a_query(pose, p[0], p[1], p[2], &x, &y, &z);
    p[0] = x; p[1] = y; p[2] = z;
  }
  unsigned int c[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double lo = dec_f64(bbox[d]), hi = dec_f64(bbox[3 + d]);
    double u = (hi > lo) ? (p[d] - lo) / (hi - lo) : 0.0;
    if (!(u > 0.0)) u = 0.0;          // also NaN
    if (u > 0.999999) u = 0.999999;
    c[d] = (unsigned int)(u * 1024.0);
  }
  keys[e] = spread10(c[0]) | (spread10(c[1]) << 1) | (spread10(c[2]) << 2) | key_or;
  vals[e] = (int32_t)i;
}

// one workgroup per 512-slot tile: gather the curve-ordered targets, write SoA (f64 + f32) and the
// original index, reduce the tile's outward-rounded float32 box and the global max |coordinate|
__global__ __launch_bounds__(256) void k_targets_sorted(const double* __restrict__ tgt, int64_t M,
                                                        const int32_t* __restrict__ order, double* __restrict__ tx,
                                                        double* __restrict__ ty, double* __restrict__ tz,
                                                        float* __restrict__ txf, float* __restrict__ tyf,
                                                        float* __restrict__ tzf, int32_t* __restrict__ torig,
                                                        float* __restrict__ tile_box /* [6][n_tiles] */, int n_tiles,
                                                        unsigned long long* __restrict__ emax_bits,
                                                        float4* __restrict__ tile_a /* [n_tiles][8][64] */,
                                                        float4* __restrict__ tile_o /* [n_tiles] */) {
  __shared__ float red[4][6];
  __shared__ float s_org[3], s_c[4];
  __shared__ __align__(16) float s_rows[2048];
  const int tile = blockIdx.x;
  float lo[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()};
  float hi[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
  double e = 0.0;
  double px[2], py[2], pz[2];   // this thread's two slots, kept for the tile-local rows below
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int r = threadIdx.x + 256 * h;
    const int64_t j = (int64_t)tile * 512 + r;
    const double nan = __builtin_nan("");
    double x = nan, y = nan, z = nan;
    int32_t o = 0;
    if (j < M) {
      o = order[j];
      x = tgt[3 * (int64_t)o]; y = tgt[3 * (int64_t)o + 1]; z = tgt[3 * (int64_t)o + 2];
      const double m = fmax(fabs(x), fmax(fabs(y), fabs(z)));
      e = fmax(e, (m == m) ? m : __builtin_huge_val());  // NaN input disables the float32 filter
      if (x == x) { lo[0] = __builtin_fminf(lo[0], f32_floor(x)); hi[0] = __builtin_fmaxf(hi[0], f32_ceil(x)); }
      if (y == y) { lo[1] = __builtin_fminf(lo[1], f32_floor(y)); hi[1] = __builtin_fmaxf(hi[1], f32_ceil(y)); }
      if (z == z) { lo[2] = __builtin_fminf(lo[2], f32_floor(z)); hi[2] = __builtin_fmaxf(hi[2], f32_ceil(z)); }
    }
    tx[j] = x; ty[j] = y; tz[j] = z;
    txf[j] = (float)x; tyf[j] = (float)y; tzf[j] = (float)z;
    torig[j] = o;
    px[h] = x; py[h] = y; pz[h] = z;
  }
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      lo[d] = __builtin_fminf(lo[d], __shfl_xor(lo[d], off, kWave));
      hi[d] = __builtin_fmaxf(hi[d], __shfl_xor(hi[d], off, kWave));
    }
    e = fmax(e, __shfl_xor(e, off, kWave));
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) { red[wave][d] = lo[d]; red[wave][3 + d] = hi[d]; }
    if (e > 0.0) atomicMax(emax_bits, (unsigned long long)__double_as_longlong(e));
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int d = threadIdx.x;
    float v = red[0][d];
    for (int w = 1; w < 4; ++w) v = d < 3 ? __builtin_fminf(v, red[w][d]) : __builtin_fmaxf(v, red[w][d]);
    tile_box[(size_t)d * n_tiles + tile] = v;  // empty tile: lo = +inf, hi = -inf  => never needed
    red[0][d] = v;
  }
  // ---- tile-local rows for the matrix-pipe pre-filter (knn_tiles.hip) ----
  // origin o = the box centre in float32 (any finite float32 serves: the bound is written in |t - o|); row of a target =
  // t' = fl32(t - o) (float64 subtraction, rounded once), cc = fl32(|t'|²); C_t = max |t'|₂ rounded up, +inf when a row is
  // not finite.  Padding slots: zero coordinates and cc = 1e30 — finite, never below a finite threshold.
  __syncthreads();
  if (threadIdx.x < 3) {
    const int d = threadIdx.x;
    const float c = (float)(0.5 * ((double)red[0][d] + (double)red[0][3 + d]));
    s_org[d] = (c - c == 0.0f) ? c : 0.0f;   // empty or unbounded box: any origin
  }
  __syncthreads();
  const float o0 = s_org[0], o1 = s_org[1], o2 = s_org[2];
  float cmax = 0.0f;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int r = threadIdx.x + 256 * h;
    const int64_t j = (int64_t)tile * 512 + r;
    float v[4] = {0.0f, 0.0f, 0.0f, 1e30f};
    if (j < M) {
      v[0] = (float)(px[h] - (double)o0); v[1] = (float)(py[h] - (double)o1); v[2] = (float)(pz[h] - (double)o2);
      const double n2 = ((double)v[0] * (double)v[0] + (double)v[1] * (double)v[1]) + (double)v[2] * (double)v[2];
      v[3] = (float)n2;
      const float n = next_up(f32_ceil(sqrt(n2)));
      cmax = (n - n == 0.0f) ? __builtin_fmaxf(cmax, n) : __builtin_huge_valf();   // NaN or inf row: no finite bound
    }
    // A-operand order: lane = 16 * component + (row mod 16), float4 index = row block / 4, element = row block mod 4
    const int rb = r >> 4, mj = r & 15;
#pragma unroll
    for (int c = 0; c < 4; ++c) s_rows[(((rb >> 2) * 64) + c * 16 + mj) * 4 + (rb & 3)] = v[c];
  }
  for (int off = 32; off > 0; off >>= 1) cmax = __builtin_fmaxf(cmax, __shfl_xor(cmax, off, kWave));
  if (lane == 0) s_c[wave] = cmax;
  __syncthreads();
  const float4* rows4 = reinterpret_cast<const float4*>(s_rows);
  tile_a[(size_t)tile * 512 + threadIdx.x] = rows4[threadIdx.x];
  tile_a[(size_t)tile * 512 + 256 + threadIdx.x] = rows4[256 + threadIdx.x];
  if (threadIdx.x == 0)
    tile_o[tile] = make_float4(o0, o1, o2, __builtin_fmaxf(__builtin_fmaxf(s_c[0], s_c[1]), __builtin_fmaxf(s_c[2], s_c[3])));
}

// ---------------- stable LSD radix sort of (key, index) pairs: three passes, two launches each ----------------
// The pairs are one or two segments that are sorted apart in the same launches: one cloud, or the target's pairs followed
// by the queries' (the joint sort: bit 30 of a query key only says "behind every target key", which the segments do by
// position, so every pass sorts a 10-bit digit of the 30-bit Morton key).  A workgroup owns kSortBlockItems consecutive
// pairs of one segment, a wave 256 of them, 64 per round.  k_sort_hist counts the workgroup's digits into
// hist[workgroup][digit]; k_sort_scatter ranks every pair among the equal digits ahead of it in its workgroup (wave rounds
// in order, lanes in order: stable), sums the table's columns over its segment for its own start per digit — all
// workgroups ahead, all smaller digits — and writes.  No scan launch: a workgroup reads its segment's rows of 4 KB from L2
// (C3: 64 + 32 rows).  The ranks come from one ballot per digit bit, not from contended LDS atomics, and the counts take a
// wave whose 64 digits are equal in one add, so a cloud in one Morton cell (or all NaN: key 0) costs what a spread one does.
#ifndef SVNICP_SORT_ITEMS
#define SVNICP_SORT_ITEMS 4
#endif
constexpr int kSortThreads = 1024, kSortItems = SVNICP_SORT_ITEMS, kSortWaves = kSortThreads / kWave;   // pairs per thread (8 and 2 measured slower: DESIGN §4.1)
constexpr int kSortBlockItems = kSortThreads * kSortItems;   // 4096 pairs
constexpr int kSortBits = 10, kSortBins = 1 << kSortBits;    // one digit per thread
constexpr int kSortMaxBlocks = 512;                          // 2 M pairs; the column sums grow with the square (larger sorts: rocPRIM)
static_assert(kSortBins == kSortThreads, "k_sort_scatter: thread t owns digit t");

// segment 0: pairs [0, n0) in workgroups [0, nb0); segment 1: pairs [n0, n0 + n1) in workgroups [nb0, gridDim.x)
struct SortSegs { unsigned int n0, n1; int nb0; };
struct SortBlock { unsigned int lo, n, first; int b0, b1; };   // the segment's pairs [lo, lo + n), its workgroups [b0, b1), this one's first pair
__device__ __forceinline__ SortBlock sort_block(const SortSegs& s) {
  SortBlock k;
  const int b = (int)blockIdx.x;
  if (b < s.nb0) { k.lo = 0u; k.n = s.n0; k.b0 = 0; k.b1 = s.nb0; }
  else { k.lo = s.n0; k.n = s.n1; k.b0 = s.nb0; k.b1 = (int)gridDim.x; }
  k.first = k.lo + (unsigned int)(b - k.b0) * (unsigned int)kSortBlockItems;
  return k;
}

__device__ __forceinline__ unsigned long long digit_peers(unsigned int d, unsigned long long live) {   // live lanes whose digit equals d
  unsigned long long m = live;
#pragma unroll
  for (int k = 0; k < kSortBits; ++k) {
    const unsigned int bit = (d >> k) & 1u;
    m &= __ballot(bit) ^ ((unsigned long long)bit - 1ull);   // the lanes that have the bit, or those that do not
  }
  return m;
}

__global__ __launch_bounds__(kSortThreads) void k_sort_hist(const unsigned int* __restrict__ keys, SortSegs segs, int shift,
                                                            unsigned int* __restrict__ hist /* [gridDim.x][kSortBins] */) {
  __shared__ unsigned int h[kSortBins];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const SortBlock blk = sort_block(segs);
  const int lane = threadIdx.x & (kWave - 1);
  const unsigned int base = blk.first + (threadIdx.x >> 6) * (unsigned int)(kWave * kSortItems) + lane;
  unsigned int key[kSortItems];
#pragma unroll
  for (int r = 0; r < kSortItems; ++r) {
    const unsigned int i = base + r * kWave;
    key[r] = i - blk.lo < blk.n ? keys[i] : 0u;
  }
#pragma unroll
  for (int r = 0; r < kSortItems; ++r) {   // wave-uniform
    const bool live = base + r * kWave - blk.lo < blk.n;
    const unsigned int d = (key[r] >> shift) & (kSortBins - 1);
    const unsigned int d0 = (unsigned int)__builtin_amdgcn_readfirstlane((int)d);
    if (__all(live && d == d0)) {   // 64 equal digits: one add, not 64 on one address
      if (lane == 0) atomicAdd(&h[d0], (unsigned int)kWave);
    } else if (live) {
      atomicAdd(&h[d], 1u);
    }
  }
  __syncthreads();
  hist[(size_t)blockIdx.x * kSortBins + threadIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(kSortThreads) void k_sort_scatter(const unsigned int* __restrict__ keys_in, const int32_t* __restrict__ vals_in,
                                                               unsigned int* __restrict__ keys_out /* or nullptr */, int32_t* __restrict__ vals_out,
                                                               SortSegs segs, int shift, const unsigned int* __restrict__ hist) {
  __shared__ unsigned short cnt[kSortWaves][kSortBins];   // per wave and digit: pairs so far, then the pairs of the waves ahead
  __shared__ unsigned int off[kSortBins];                 // where the workgroup's first pair of a digit goes, from the segment's start
  __shared__ unsigned int wsum[kSortWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  for (int w = 0; w < kSortWaves; ++w) cnt[w][tid] = 0;
  __syncthreads();
  const SortBlock blk = sort_block(segs);
  // ranks inside the wave's 256 pairs; a wave touches only its own row of cnt, and its LDS operations keep their order
  volatile unsigned short* mine = cnt[wave];
  const unsigned int base = blk.first + wave * (unsigned int)(kWave * kSortItems) + lane;
  const unsigned long long lt = (1ull << lane) - 1ull;
  unsigned int key[kSortItems];
  int32_t val[kSortItems];
  unsigned short rank[kSortItems];
#pragma unroll
  for (int r = 0; r < kSortItems; ++r) {
    const unsigned int i = base + r * kWave;
    const bool live = i - blk.lo < blk.n;
    key[r] = live ? keys_in[i] : 0u;
    val[r] = live ? vals_in[i] : 0;
  }
#pragma unroll
  for (int r = 0; r < kSortItems; ++r) {
    const bool live = base + r * kWave - blk.lo < blk.n;
    const unsigned int d = (key[r] >> shift) & (kSortBins - 1);
    const unsigned long long m = digit_peers(d, __ballot(live));
    const unsigned int prior = mine[d];
    rank[r] = (unsigned short)(prior + (unsigned int)__popcll(m & lt));
    if (live && lane == __ffsll((long long)m) - 1) mine[d] = (unsigned short)(prior + (unsigned int)__popcll(m));
  }
  __syncthreads();
  // digit tid: the table's column sums over the segment's workgroups, all of them and those ahead of this one
  unsigned int tot = 0u, pre = 0u;
  for (int b = blk.b0; b < blk.b1; ++b) {
    const unsigned int v = hist[(size_t)b * kSortBins + tid];
    tot += v;
    pre += b < (int)blockIdx.x ? v : 0u;
  }
  unsigned int inc = tot;   // inclusive scan over the digits: wave, then the waves' totals
  for (int o = 1; o < kWave; o <<= 1) { const unsigned int x = __shfl_up(inc, o, kWave); if (lane >= o) inc += x; }
  if (lane == kWave - 1) wsum[wave] = inc;
  __syncthreads();
  unsigned int start = inc - tot;
  for (int w = 0; w < wave; ++w) start += wsum[w];
  off[tid] = start + pre;
  unsigned int run = 0u;
  for (int w = 0; w < kSortWaves; ++w) { const unsigned int c = cnt[w][tid]; cnt[w][tid] = (unsigned short)run; run += c; }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kSortItems; ++r) {
    const bool live = base + r * kWave - blk.lo < blk.n;
    const unsigned int d = (key[r] >> shift) & (kSortBins - 1);
    const unsigned int dst = off[d] + cnt[wave][d] + rank[r];
    if (live && dst < blk.n) {   // (dst < n holds whenever the table was counted from these keys)
      if (keys_out) keys_out[blk.lo + dst] = key[r];
      vals_out[blk.lo + dst] = val[r];
    }
  }
}

size_t lsd_sort_blocks(size_t n) { return (n + kSortBlockItems - 1) / kSortBlockItems; }
size_t lsd_sort_temp_bytes(size_t n) { return (lsd_sort_blocks(n) + 1) * kSortBins * sizeof(unsigned int); }   // two segments: one more workgroup
bool lsd_sort_serves(size_t n0, size_t n1, size_t temp_bytes) {
  return n0 > 0 && lsd_sort_blocks(n0) + lsd_sort_blocks(n1) <= (size_t)kSortMaxBlocks && temp_bytes >= lsd_sort_temp_bytes(n0 + n1);
}

hipError_t lsd_sort_pass(const unsigned int* keys_in, const int32_t* vals_in, unsigned int* keys_out, int32_t* vals_out, const SortSegs& segs, int nb,
                         int shift, unsigned int* hist, hipStream_t st) {
  hipLaunchKernelGGL(k_sort_hist, dim3(nb), dim3(kSortThreads), 0, st, keys_in, segs, shift, hist);
  hipLaunchKernelGGL(k_sort_scatter, dim3(nb), dim3(kSortThreads), 0, st, keys_in, vals_in, keys_out, vals_out, segs, shift, (const unsigned int*)hist);
  return hipGetLastError();
}

// vals_a[0, n0) sorted by keys_a (stable, 30 bits) into order[0, n0), and vals_a[n0, n0 + n1) into order[n0, n0 + n1); keys_a,
// keys_b and vals_a are scratch.  Six launches whatever the keys are.
hipError_t lsd_sort_pairs(unsigned int* keys_a, unsigned int* keys_b, int32_t* vals_a, int32_t* order, size_t n0, size_t n1, void* temp,
                          hipStream_t st) {
  unsigned int* hist = static_cast<unsigned int*>(temp);
  const SortSegs segs{(unsigned int)n0, (unsigned int)n1, (int)lsd_sort_blocks(n0)};
  const int nb = segs.nb0 + (int)lsd_sort_blocks(n1);
  hipError_t e = lsd_sort_pass(keys_a, vals_a, keys_b, order, segs, nb, 0, hist, st);
  if (e != hipSuccess) return e;
  e = lsd_sort_pass(keys_b, order, keys_a, vals_a, segs, nb, kSortBits, hist, st);
  if (e != hipSuccess) return e;
  return lsd_sort_pass(keys_a, vals_a, nullptr, order, segs, nb, 2 * kSortBits, hist, st);
}

// the Morton sorts' one entry: n0 pairs, or n0 target pairs and n1 query pairs whose keys carry bit 30 — the chain above
// (Tuning::sort_merge = 0, sizes it serves) or rocPRIM's radix_sort_pairs over all of them
hipError_t sort_pairs(bool rocprim_sort, unsigned int* keys_a, unsigned int* keys_b, int32_t* vals_a, int32_t* order, size_t n0, size_t n1,
                      void* temp, size_t temp_bytes, hipStream_t st) {
  if (!rocprim_sort && lsd_sort_serves(n0, n1, temp_bytes)) return lsd_sort_pairs(keys_a, keys_b, vals_a, order, n0, n1, temp, st);
  return rocprim::radix_sort_pairs(temp, temp_bytes, keys_a, keys_b, vals_a, order, n0 + n1, 0, n1 ? 31 : 30, st);
}

}  // namespace

size_t sort_temp_bytes(size_t n, int key_bits) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_pairs(nullptr, bytes, (unsigned int*)nullptr, (unsigned int*)nullptr, (int32_t*)nullptr,
                                  (int32_t*)nullptr, n, 0, key_bits, (hipStream_t)0);
  return bytes > lsd_sort_temp_bytes(n) ? bytes : lsd_sort_temp_bytes(n);
}

// order[0..n) = indices i0..i0+n of pts sorted along the Morton curve of `bbox`
// (fill_ff, fill_words: words the key kernel sets to -1 on the way, or nullptr)
hipError_t launch_morton_order(const double* pts, int64_t i0, int64_t n, int transform, const Pose0& pose,
                               const unsigned long long* bbox, unsigned int* keys_a, unsigned int* keys_b,
                               int32_t* vals_a, int32_t* order, void* temp, size_t temp_bytes, bool rocprim_sort, int32_t* fill_ff,
                               size_t fill_words, hipStream_t st) {
  if (n <= 0) return fill_words ? hipMemsetAsync(fill_ff, 0xff, fill_words * sizeof(int32_t), st) : hipSuccess;
  hipLaunchKernelGGL(k_morton_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pts, i0, n, transform, pose, bbox,
                     keys_a, vals_a, 0u, fill_ff, fill_words);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return sort_pairs(rocprim_sort, keys_a, keys_b, vals_a, order, (size_t)n, 0, temp, temp_bytes, st);
}

// One sort for both clouds: the target's keys in [0, M), the keys of the n queries (pose · qsrc[0, n), inside the target's
// box like every query key) behind them with bit 30 set, one stable 31-bit sort of the M + n pairs.  Every query key sorts
// behind every target key and equal keys keep their input order, so order[0, M) is launch_morton_order's permutation of
// the target and order[M, M + n) its permutation of the queries (values are row indices of their own cloud).
hipError_t launch_morton_order_joint(const double* tgt, int64_t M, const double* qsrc, int64_t n, const Pose0& pose,
                                     const unsigned long long* bbox, unsigned int* keys_a, unsigned int* keys_b,
                                     int32_t* vals_a, int32_t* order, void* temp, size_t temp_bytes, bool rocprim_sort, int32_t* fill_ff,
                                     size_t fill_words, hipStream_t st) {
  if (M <= 0 || n <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_morton_keys, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, tgt, 0, M, 0, pose, bbox, keys_a, vals_a, 0u,
                     (int32_t*)nullptr, (size_t)0);
  hipLaunchKernelGGL(k_morton_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, qsrc, 0, n, 1, pose, bbox, keys_a + M,
                     vals_a + M, 1u << 30, fill_ff, fill_words);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return sort_pairs(rocprim_sort, keys_a, keys_b, vals_a, order, (size_t)M, (size_t)n, temp, temp_bytes, st);
}

// cleared: the six words already hold their start values (min: all ones, max: zero) — the launch that begins a registration wrote them
hipError_t launch_bbox(const double* pts, int64_t n, unsigned long long* bbox, bool cleared, hipStream_t st) {
  if (!cleared) {
    hipError_t e = hipMemsetAsync(bbox, 0xff, 3 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(bbox + 3, 0, 3 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
  }
  int64_t nb = (n + 255) / 256;
  if (nb > 256) nb = 256;  // grid-stride; one set of atomics per workgroup (1024 workgroups: 27 us, most of it the 6 x 1024 same-address atomics)
  hipLaunchKernelGGL(k_bbox, dim3((unsigned)nb), dim3(256), 0, st, pts, n, bbox);
  return hipGetLastError();
}

hipError_t launch_targets_sorted(const double* tgt, int64_t M, int64_t Mp, const int32_t* order, double* tx, double* ty,
                                 double* tz, float* txf, float* tyf, float* tzf, int32_t* torig, float* tile_box,
                                 unsigned long long* emax_bits, bool emax_cleared, float4* tile_a, float4* tile_o, hipStream_t st) {
  if (!emax_cleared) {
    hipError_t e = hipMemsetAsync(emax_bits, 0, sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
  }
  const int n_tiles = (int)(Mp / 512);
  hipLaunchKernelGGL(k_targets_sorted, dim3(n_tiles), dim3(256), 0, st, tgt, M, order, tx, ty, tz, txf, tyf, tzf, torig,
                     tile_box, n_tiles, emax_bits, tile_a, tile_o);
  return hipGetLastError();
}

}  // namespace svnicp
