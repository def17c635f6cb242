// map_visibility.hip — visibility-based clearing of the voxel map (svnicp_map_clear_seen_through; the
// contract is in include/svnicp_hip.h).  Not in the reference.  The projection is range_project_device.hpp's, shared with the
// range-image segmentation, so a map point and a scan point that lie on one ray land in one pixel.
//
// The minimum-range image holds the bit patterns of non-negative floats, which order as unsigned integers: one 32-bit atomicMin
// per scan point, whatever the schedule.  Empty = the pattern of +inf.
#include "map_visibility.hpp"

#include "voxel_table_device.hpp"

namespace svnicp {
namespace {

constexpr unsigned int kVisEmpty = 0x7f800000u;

// the fills of the call in one launch: the image, the selection keys (entries the selection does not fill stay ~0), the
// selection counter and the call's statistics
__global__ __launch_bounds__(256) void k_vis_fill(unsigned int* __restrict__ img, int64_t npix, unsigned long long* __restrict__ sel_key,
                                                  int64_t live, int* __restrict__ nsel, unsigned long long* __restrict__ vstats) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < npix) img[i] = kVisEmpty;
  if (i < live) sel_key[i] = kEmpty;
  if (i < kVisStats) vstats[i] = 0ull;
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
  if (threadIdx.x == 0 && s_new) atomicAdd(&vstats[kVisPixelsFilled], (unsigned long long)s_new);   // one global atomic per workgroup
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
      atomicAdd(&vstats[kVisPointsRemoved], (unsigned long long)(cnt - base));
      if (base == 0) {   // a tombstone, as k_map_remove_far makes one
        keys[slot] = kTomb;
        atomicSub(&stats[kStatLive], 1); atomicAdd(&stats[kStatTombs], 1);
        atomicAdd(&vstats[kVisVoxelsEmptied], 1ull);
      }
    }
    if (tested) atomicAdd(&vstats[kVisPointsTested], (unsigned long long)tested);
  }
}

}  // namespace

hipError_t launch_map_clear_seen_through(const MapTableMut& T, const float* scan, int64_t n, const MapPose& pose, const RangeSensor& S,
                                         const VisOpt& O, int64_t live, MapSelection& sel, MapVisibility& V, hipStream_t stream) {
  const int64_t npix = (int64_t)S.N * S.H;
  HIPTRY(V.img.ensure((size_t)npix)); HIPTRY(V.stats.ensure(kVisStats));
  HIPTRY(sel.key.ensure((size_t)live)); HIPTRY(sel.slot.ensure((size_t)live));
  const int64_t nfill = npix > live ? npix : live;
  HIPTRY(launch_checked(k_vis_fill, dim3(blocks_of(nfill)), dim3(256), 0, stream, V.img.p, npix, sel.key.p, live, sel.nsel.p, V.stats.p));
  // every live voxel (r2 < 0), in any order: each is handled by itself
  HIPTRY(launch_map_select(T.view(), 0.0, 0.0, 0.0, -1.0, sel.key.p, sel.slot.p, sel.nsel.p, (int)live, stream));
  HIPTRY(launch_checked(k_vis_image, dim3(blocks_of(n)), dim3(256), 0, stream, scan, n, S, V.img.p, V.stats.p));
  return launch_checked(k_vis_clear, dim3((unsigned)live), dim3(64), 0, stream, T.keys, T.counts, T.pts, T.max_points, sel.key.p, sel.slot.p,
                        pose, S, O, V.img.p, T.stats, V.stats.p);
}

}  // namespace svnicp
