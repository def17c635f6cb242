// map_score.hip — how well does a scan fit the voxel map at each of C candidate poses (svnicp_map_score_poses; the contract is
// in include/svnicp_hip.h, the design in DESIGN.md §4.16).  Not in the reference: its map lives on the host and is only ever
// turned into a target cloud.
//
// One thread per (pose, source row).  The grid is (row chunk, pose): a workgroup owns the kScoreRows consecutive rows of one
// chunk for ONE pose, so the 12 doubles of the pose are workgroup-uniform, neighbouring lanes transform neighbouring rows of the
// scan and probe neighbouring voxels.  The table is only read (find_slot of voxel_table_device.hpp).  No atomics: a wave adds
// its 64 values with one butterfly, thread 0 adds the four waves in wave order, the record of the chunk is written with plain
// stores, and k_map_score_finish adds the chunks of a pose in chunk order.  The counts are ballots and integer sums throughout.
// With a single chunk the workgroup writes the pose's final record itself.
#include "map_score.hpp"
#include "voxel_table_device.hpp"

namespace svnicp {
namespace {

// {located, inliers, sum_d2, cost}; n == 0: nothing to average, the cost is the gate
__device__ __forceinline__ void write_record(double* __restrict__ o, unsigned long long located, unsigned long long inliers, double sum,
                                             int64_t n, double thr2) {
  o[0] = (double)located;
  o[1] = (double)inliers;
  o[2] = sum;
  o[3] = n > 0 ? (sum + (double)(n - (int64_t)inliers) * thr2) / (double)n : thr2;
}

__global__ __launch_bounds__(kScoreRows) void k_map_score(MapTableView T, const float* __restrict__ src, int64_t n,
                                                          const double* __restrict__ poses, double thr2, int64_t chunks,
                                                          unsigned int* __restrict__ part_cnt, double* __restrict__ part_sum,
                                                          double* __restrict__ out) {
  __shared__ double s_sum[kScoreRows / 64];
  __shared__ unsigned int s_loc[kScoreRows / 64], s_inl[kScoreRows / 64];
  const int64_t chunk = blockIdx.x, pose = blockIdx.y;
  const int64_t i = chunk * kScoreRows + threadIdx.x;
  const double* __restrict__ P = poses + 12 * pose;   // workgroup-uniform
  bool located = false;
  double dmin2 = 0.0;
  if (i < n) {
    const float p0 = src[3 * i], p1 = src[3 * i + 1], p2 = src[3 * i + 2];
    // k_map_locate's expression: formed in double from the widened float32 point, left to right, rounded ONCE to float32
    float c[3];
    long long v[3];
    bool ok = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      c[d] = (float)(((P[3 * d] * (double)p0 + P[3 * d + 1] * (double)p1) + P[3 * d + 2] * (double)p2) + P[9 + d]);
      const float f = truncf(c[d] / T.voxel);
      ok = ok && (f >= (float)-kOff) && (f < (float)kOff);   // also false for NaN and inf
      v[d] = ok ? (long long)f : 0;
    }
    if (ok) {
      // Conservative skip.  Every point stored in voxel w lies in the box [lo, hi] per axis: lo = w * vs for w > 0, (w - 1) * vs
      // otherwise (truncation toward zero makes voxel 0 twice as wide: (-vs, vs)), hi likewise; widened by 2^-20 of the bound
      // because the index is the truncated FLOAT32 quotient, which rounds.  A voxel whose box is at least the gate away ("far")
      // cannot hold an inlier's nearest point: it is never searched, and looked up only if no near voxel settles `located`.
      const double vs = (double)T.voxel;
      const double cc[3] = {(double)c[0], (double)c[1], (double)c[2]};
      double gap2[3][3];   // [axis][offset + 1]; every index below is a compile-time constant: registers
#pragma unroll
      for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int o = 0; o < 3; ++o) {
          const long long w = v[d] + (o - 1);
          double lo = (double)(w <= 0 ? w - 1 : w) * vs, hi = (double)(w >= 0 ? w + 1 : w) * vs;
          lo -= fabs(lo) * 0x1p-20; hi += fabs(hi) * 0x1p-20;
          const double g = fmax(0.0, fmax(lo - cc[d], cc[d] - hi));
          gap2[d][o] = g * g;
        }
      const unsigned long long mask = (unsigned long long)(T.cap - 1);
      double best = 0.0;
      bool have = false;
      unsigned int far_left = 0;   // bit j: voxel j exists, is far and has not been looked up
      // The near voxels, one x-slab of nine at a time: the nine first probes are issued together, then the nine counts, so a
      // thread waits for memory three times per slab instead of twice per voxel (the kernel is bound by that latency).
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        unsigned long long key[9], cur[9];
        bool want[9];
#pragma unroll
        for (int b = 0; b < 9; ++b) {
          const long long w0 = v[0] + (a - 1), w1 = v[1] + (b / 3 - 1), w2 = v[2] + (b % 3 - 1);
          const bool exists = voxel_in_range(w0, w1, w2);        // no such voxel: never packed into a key
          const bool far = (gap2[0][a] + gap2[1][b / 3]) + gap2[2][b % 3] >= thr2;
          want[b] = exists && !far;
          if (exists && far) far_left |= 1u << (9 * a + b);
          key[b] = want[b] ? pack_key(w0, w1, w2) : kEmpty;
          cur[b] = want[b] ? T.keys[hash_key(key[b]) & mask] : kEmpty;
        }
        int cnt[9];
        int64_t slot[9];
#pragma unroll
        for (int b = 0; b < 9; ++b) {
          slot[b] = -1;
          if (want[b]) {
            if (cur[b] == key[b]) slot[b] = (int64_t)(hash_key(key[b]) & mask);
            else if (cur[b] != kEmpty) slot[b] = find_slot(T.keys, T.cap, key[b]);   // a collision or a tombstone: the full probe
          }
          cnt[b] = slot[b] >= 0 ? T.counts[slot[b]] : 0;
        }
#pragma unroll
        for (int b = 0; b < 9; ++b) {
          const int n_pts = cnt[b] < 0 ? 0 : (cnt[b] > T.max_points ? T.max_points : cnt[b]);
          if (n_pts == 0) continue;
          located = true;
          const float* __restrict__ q = T.pts + (size_t)slot[b] * T.max_points * 3;
          for (int k = 0; k < n_pts; ++k) {
            const double dx = (double)q[3 * k] - cc[0], dy = (double)q[3 * k + 1] - cc[1], dz = (double)q[3 * k + 2] - cc[2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (!have || d2 < best) { best = d2; have = true; }
          }
        }
      }
      for (int j = 0; j < 27 && !located; ++j) {   // nothing near: a far voxel with a point still makes the row located
        if (!((far_left >> j) & 1u)) continue;
        const int64_t slot = find_slot(T.keys, T.cap, pack_key(v[0] + (j / 9 - 1), v[1] + ((j / 3) % 3 - 1), v[2] + (j % 3 - 1)));
        located = slot >= 0 && T.counts[slot] > 0;
      }
      dmin2 = have ? best : thr2;   // only far voxels hold points: not an inlier
    }
  }
  const bool inlier = located && dmin2 < thr2;
  double sum = inlier ? dmin2 : 0.0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);   // one fixed shape
  const unsigned int nloc = (unsigned int)__popcll(__ballot(located)), ninl = (unsigned int)__popcll(__ballot(inlier));
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_sum[wave] = sum; s_loc[wave] = nloc; s_inl[wave] = ninl; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double total = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    const unsigned int loc = s_loc[0] + s_loc[1] + s_loc[2] + s_loc[3], inl = s_inl[0] + s_inl[1] + s_inl[2] + s_inl[3];
    if (chunks == 1) {
      write_record(out + 4 * pose, loc, inl, total, n, thr2);
    } else {
      const int64_t r = pose * chunks + chunk;
      part_cnt[2 * r] = loc; part_cnt[2 * r + 1] = inl;
      part_sum[r] = total;
    }
  }
}

// one thread per pose: the chunk records in chunk order; chunks == 0 (no rows) writes {0, 0, 0, thr2}
__global__ __launch_bounds__(256) void k_map_score_finish(const unsigned int* __restrict__ part_cnt, const double* __restrict__ part_sum,
                                                          int64_t chunks, int64_t poses, int64_t n, double thr2,
                                                          double* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= poses) return;
  unsigned long long loc = 0, inl = 0;
  double sum = 0.0;
#pragma unroll 8
  for (int64_t k = 0; k < chunks; ++k) {   // the loads run ahead, the sums stay in chunk order
    const int64_t r = p * chunks + k;
    loc += part_cnt[2 * r]; inl += part_cnt[2 * r + 1];
    sum += part_sum[r];
  }
  write_record(out + 4 * p, loc, inl, sum, n, thr2);
}

}  // namespace

hipError_t launch_map_score(const MapTableView& T, const float* src, int64_t n, const double* poses, int64_t C, double thr2,
                            unsigned int* part_cnt, double* part_sum, double* out, hipStream_t stream) {
  const int64_t chunks = map_score_chunks(n);   // <= 2^23: chunks * kScoreRows threads fit the grid's x extent
  for (int64_t c0 = 0; c0 < C; c0 += kScorePoseBatch) {
    const int64_t nb = C - c0 < kScorePoseBatch ? C - c0 : kScorePoseBatch;
    if (chunks > 0)
      hipLaunchKernelGGL(k_map_score, dim3((unsigned)chunks, (unsigned)nb), dim3(kScoreRows), 0, stream, T, src, n, poses + 12 * c0, thr2,
                         chunks, part_cnt, part_sum, out + 4 * c0);
    if (chunks != 1)
      hipLaunchKernelGGL(k_map_score_finish, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, stream, part_cnt, part_sum, chunks, nb, n,
                         thr2, out + 4 * c0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace svnicp
