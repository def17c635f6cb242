// particle_modes.hip — svnicp_particle_modes (include/svnicp_hip.h "particle modes"): the particle set grouped
// into the connected components of its link graph, and each component's mass, mean, covariance and best-scored member.
// One kernel, one workgroup: the set is small (P <= kModesMaxP) and every step needs all of it.
//   stage     the [6][P] poses and the weights into LDS, as k_stats does; a particle with a non-finite component gets label -1
//   label     sweeps until one changes nothing: every particle finds the lowest label among the particles it links to (the
//             pair distances are recomputed each sweep: a P x P bitmap does not fit beside the poses; a partner whose label
//             cannot lower this particle's is skipped before any arithmetic), every root hooks onto the lowest label its
//             members found, and the pointers are jumped until every tree is a star again.  A label is always the index of
//             a particle of the same component and only ever decreases, each thread writes its own particles' entries
//             alone, and at the fixed point linked particles agree and every label is its own root: the component's lowest
//             index, whatever the schedule.  Hooking the roots is what keeps a chain short: every tree that has a lower
//             neighbour merges in every sweep, so a chain of 1030 shuffled particles takes 8 sweeps, not hundreds (DESIGN.md
//             §4.14).
//   rank      the thread of each root adds its members' weights in particle order and counts the roots ahead of it by (W, label)
//   sums      one thread per (reported mode, output): members in ascending particle order, the expressions of the header
// The sums are written without a branch -- a particle of another mode adds a selected + 0.0, never its own term -- so that
// the loads of eight particles are in flight at a time.  That changes no bit: a sum that starts at + 0.0 is never - 0.0 (only
// - 0.0 + - 0.0 gives it), and s + 0.0 == s for every other s, NaN and infinities included.
// No atomics, no stop flag, no scratch.  The counts are __syncthreads_count's.
#include "kernels.hpp"

namespace svnicp {
namespace {

constexpr int NT = 1024;
constexpr int kPer = kModesMaxP / NT;   // particles a thread owns: tid, tid + NT

__global__ __launch_bounds__(NT) void k_particle_modes(ModesArgs a) {
  extern __shared__ __align__(16) double lds[];
  const int P = a.P;
  const int tid = threadIdx.x;
  double* x = lds;                                   // [6][P]; the costs [P] once the sums are done
  double* w = x + 6 * (size_t)P;                     // [P]
  double* Wr = w + P;                                // [P] W of the mode rooted here
  int* lab = reinterpret_cast<int*>(Wr + P);         // [P] label, -1 = non-finite
  int* rnk = lab + P;                                // [P] rank of the mode rooted here
  __shared__ double s_Wall;
  __shared__ int m_root[kModesMax], m_count[kModesMax];
  __shared__ double m_W[kModesMax], m_mean[kModesMax][6];

  for (int e = tid; e < 6 * P; e += NT) x[e] = a.pose[e];
  for (int e = tid; e < P; e += NT) w[e] = a.w ? a.w[e] : 1.0;
  __syncthreads();
  int nonfinite = 0;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int p = tid + i * NT;
    bool bad = false;
    if (p < P) {
      bool fin = true;
#pragma unroll
      for (int c = 0; c < 6; ++c) fin = fin && isfinite(x[c * P + p]);
      lab[p] = fin ? p : -1;
      bad = !fin;
    }
    nonfinite += __syncthreads_count(bad);
  }

  // ---- labels: every sweep starts from stars (lab[p] is p's root, lab[root] == root) ----
  int sweeps = 0;
  for (;;) {
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int p = tid + i * NT;
      if (p < P) {
        int best = lab[p];
        if (best >= 0) {
          const double p0 = x[p], p1 = x[P + p], p2 = x[2 * P + p], p3 = x[3 * P + p], p4 = x[4 * P + p], p5 = x[5 * P + p];
          for (int q0 = 0; q0 < P; q0 += 8) {   // eight labels in flight; x[.. + q] and lab[q] are broadcasts
            int l8[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) l8[j] = q0 + j < P ? lab[q0 + j] : -1;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const int q = q0 + j, lq = l8[j];
              if (lq < 0 || lq >= best) continue;   // past the set, non-finite, or nothing to gain
              const double d0 = p0 - x[q], d1 = p1 - x[P + q], d2 = p2 - x[2 * P + q];
              const double d3 = p3 - x[3 * P + q], d4 = p4 - x[4 * P + q], d5 = p5 - x[5 * P + q];
              const double dt2 = ((d0 * d0) + d1 * d1) + d2 * d2;
              const double dr2 = ((d3 * d3) + d4 * d4) + d5 * d5;
              if (dt2 <= a.lt2 && dr2 <= a.lr2) best = lq;
            }
          }
        }
        rnk[p] = best;   // the lowest label among p and its links (rnk is free until the modes are ranked)
      }
    }
    __syncthreads();
    // hook: a root takes the lowest label any of its members has seen (its members are at or above it; no atomics: the
    // root's own thread gathers)
    int hook[kPer];
    bool hooked = false;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int p = tid + i * NT;
      hook[i] = -1;
      if (p < P && lab[p] == p) {
        int h = p;
#pragma unroll 8
        for (int q = p; q < P; ++q) {
          const int mq = rnk[q];
          h = (lab[q] == p && mq < h) ? mq : h;
        }
        if (h < p) { hook[i] = h; hooked = true; }
      }
    }
    __syncthreads();   // every gather has read the labels of this sweep
#pragma unroll
    for (int i = 0; i < kPer; ++i)
      if (hook[i] >= 0) lab[tid + i * NT] = hook[i];
    ++sweeps;
    if (!__syncthreads_or(hooked)) break;
    for (;;) {   // jump back to stars: lab[l] <= l always, so a jump never raises a label; a stale read only costs a round
      bool jumped = false;
#pragma unroll
      for (int i = 0; i < kPer; ++i) {
        const int p = tid + i * NT;
        if (p < P) {
          const int l = lab[p];
          if (l >= 0) {
            const int ll = lab[l];
            if (ll < l) { lab[p] = ll; jumped = true; }
          }
        }
      }
      if (!__syncthreads_or(jumped)) break;
    }
  }

  // ---- W per mode in particle order, W_all, the count of modes ----
  int n_modes = 0;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int p = tid + i * NT;
    const bool root = p < P && lab[p] == p;
    if (root) {
      double s = 0.0;
#pragma unroll 8
      for (int q = p; q < P; ++q) {   // members have q >= p
        const double t = w[q];   // loaded whether a member or not: nothing waits for the label
        s += lab[q] == p ? t : 0.0;
      }
      Wr[p] = s;
    }
    n_modes += __syncthreads_count(root);
  }
  if (tid == NT - 1) {
    double s = 0.0;
#pragma unroll 8
    for (int q = 0; q < P; ++q) {
      const double t = w[q];
      s += lab[q] >= 0 ? t : 0.0;
    }
    s_Wall = s;
  }
  if (tid < kModesMax) { m_root[tid] = -1; m_count[tid] = 0; m_W[tid] = 0.0; }
  __syncthreads();

  // ---- rank by (W descending, label ascending) ----
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int p = tid + i * NT;
    if (p < P && lab[p] == p) {
      const double Wp = Wr[p];
      int r = 0;
#pragma unroll 8
      for (int q = 0; q < P; ++q) {
        const double Wq = Wr[q];   // of a root; anything else is read and not used
        r += (lab[q] == q && (Wq > Wp || (Wq == Wp && q < p))) ? 1 : 0;
      }
      rnk[p] = r;
      if (r < a.max_modes) { m_root[r] = p; m_W[r] = Wp; }
    }
  }
  __syncthreads();
  const int n_rep = n_modes < a.max_modes ? n_modes : a.max_modes;
  int32_t* labels = reinterpret_cast<int32_t*>(a.result + kModesResult);
  for (int p = tid; p < P; p += NT) labels[p] = lab[p] < 0 ? -1 : rnk[lab[p]];

  // ---- means (six per mode) and member counts (a seventh task) ----
  for (int t = tid; t < n_rep * 7; t += NT) {
    const int k = t / 7, c = t % 7, root = m_root[k];
    const int q0 = root < 0 ? P : root;   // never an index below the set (a NaN weight could leave a rank unfilled)
    if (c == 6) {
      int n = 0;
#pragma unroll 8
      for (int q = q0; q < P; ++q) n += lab[q] == root ? 1 : 0;
      m_count[k] = n;
    } else {
      const double* xc = x + (size_t)c * P;
      double s = 0.0;
#pragma unroll 8
      for (int q = q0; q < P; ++q) {
        const double t = w[q] * xc[q];
        s += lab[q] == root ? t : 0.0;
      }
      m_mean[k][c] = s / m_W[k];
    }
  }
  __syncthreads();

  // ---- covariances: the 21 entries of the upper triangle, mirrored (the product commutes bit for bit) ----
  for (int t = tid; t < n_rep * 21; t += NT) {
    const int k = t / 21, root = m_root[k];
    const int q0 = root < 0 ? P : root;
    int e = t % 21, r = 0;
    while (e >= 6 - r) { e -= 6 - r; ++r; }
    const int c = r + e;
    const double* xr = x + (size_t)r * P;
    const double* xc = x + (size_t)c * P;
    const double mr = m_mean[k][r], mc = m_mean[k][c];
    double s = 0.0;
#pragma unroll 8
    for (int q = q0; q < P; ++q) {
      const double t = w[q] * ((xr[q] - mr) * (xc[q] - mc));
      s += lab[q] == root ? t : 0.0;
    }
    const double v = s / m_W[k];
    double* rec = a.result + kModesHeader + (size_t)k * kModesRecord;
    rec[12 + 6 * r + c] = v;
    rec[12 + 6 * c + r] = v;
  }
  __syncthreads();   // the poses have been read for the last time

  // ---- the best-scored member ----
  if (a.scores)
    for (int p = tid; p < P; p += NT) x[p] = a.scores[(size_t)p * kScoreFields + 5];
  __syncthreads();
  for (int k = tid; k < kModesMax; k += NT) {
    double* rec = a.result + kModesHeader + (size_t)k * kModesRecord;
    if (k >= n_rep) {
      for (int i = 0; i < kModesRecord; ++i) rec[i] = i == 2 ? -1.0 : 0.0;
      continue;
    }
    const int root = m_root[k];
    int best = -1;
    double cmin = 0.0, cmean = 0.0;
    if (a.scores && root >= 0) {
      best = root; cmin = x[root];
      double s = 0.0;
#pragma unroll 8
      for (int q = root; q < P; ++q) {
        const bool mem = lab[q] == root;
        const double cq = x[q];
        s += mem ? cq : 0.0;
        const bool lt = mem && cq < cmin;   // strict: ties to the lowest index
        cmin = lt ? cq : cmin;
        best = lt ? q : best;
      }
      cmean = s / (double)m_count[k];
    }
    rec[0] = (double)root; rec[1] = (double)m_count[k]; rec[2] = (double)best;
    rec[3] = m_W[k] / s_Wall; rec[4] = cmin; rec[5] = cmean;
#pragma unroll
    for (int i = 0; i < 6; ++i) rec[6 + i] = m_mean[k][i];
  }
  if (tid == 0) {
    a.result[0] = (double)P; a.result[1] = (double)nonfinite; a.result[2] = (double)n_modes; a.result[3] = (double)n_rep;
    a.result[4] = (double)sweeps; a.result[5] = s_Wall; a.result[6] = 0.0; a.result[7] = 0.0;
  }
}

}  // namespace

hipError_t launch_particle_modes(const ModesArgs& a, hipStream_t st) {
  if (a.P < 1 || a.P > kModesMaxP || a.max_modes < 1 || a.max_modes > kModesMax) return hipErrorInvalidValue;   // refused, never overflowed
  const size_t smem = (size_t)a.P * (8 * sizeof(double) + 2 * sizeof(int));
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_particle_modes), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_particle_modes, dim3(1), dim3(NT), smem, st, a);
  return hipGetLastError();
}

}  // namespace svnicp
