// plane_icp.hip — the point-to-plane residual (svnicp_set_residual(SVNICP_RESIDUAL_PLANE)): normals of the
// target cloud, and the per-iteration Huber-weighted accumulation of H and b.  An extension: the reference has no such mode.
//
//   k_target_normals    per target point: covariance of its normal_k nearest target points (stage A's exact top-K with the
//                       target as the query cloud), eigen-decomposition by cyclic Jacobi, normal = eigenvector of the
//                       smallest eigenvalue; writes the packed record [M][6] = xyz | normal (one 48-byte gather per winner).
//   k_pack_normals      the same record from normals the caller supplied (svnicp_set_target_normals).
//   k_plane_accumulate  lane <-> particle like k_stein_accumulate_w: consumes the search kernel's winner index, gathers the
//                       winner's record, forms r = n·(Ts − q), the Huber weight and j = [Rtᵀn ; s × Rtᵀn], and accumulates the
//                       21 sums of H's upper triangle, the 6 of b, the accepted-pair count and Σ w·r².
//   k_plane_finalize    adds the workgroups' records in a fixed order, mirrors H, adds the 1e-6 damping: [P][42] = H | b,
//                       which the Stein-step kernels read in place of finalize_Hb's output (UpdateArgs::plane_Hb).
#include "kernels.hpp"
#include "lane_fold_device.hpp"
#include "plane_normal_device.hpp"
#include "stein_common.hpp"

namespace svnicp {

namespace {

// ---------------------------------------------------------------------------------------------
// normals
// ---------------------------------------------------------------------------------------------
// nbr: [rows][kn] target indices of the rows' neighbours (row r = target point row_lo + r), nearest first, itself included
__global__ __launch_bounds__(256) void k_target_normals(const double* __restrict__ tgt, int64_t M, const int32_t* __restrict__ nbr,
                                                        int64_t row_lo, int64_t rows, int kn, double* __restrict__ rec) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const int64_t i = row_lo + r;
  const double x0 = tgt[3 * i], x1 = tgt[3 * i + 1], x2 = tgt[3 * i + 2];
  const int32_t* nb = nbr + r * kn;
  // offsets relative to the point itself: at map-frame coordinates of kilometres the differences are still exact to 1e-13 m
  double m0 = 0.0, m1 = 0.0, m2 = 0.0;
  // "finite" offsets are those whose square float32 can hold (|d| < 2^64): a junk return of 1e20 or 1e160 is a finite number,
  // but its neighbourhood is the first kn targets at one rounded distance and its scatter matrix is rounding noise — such a
  // point has no normal, like a NaN or an infinite one (include/svnicp_hip.h, "non-finite and huge points")
  constexpr double kOffsetMax = 0x1p64;
  bool finite = true;
  for (int k = 0; k < kn; ++k) {
    int64_t j = nb[k];
    j = j < 0 ? 0 : (j >= M ? M - 1 : j);   // clamped: a corrupted list must never become a wild gather
    const double d0 = tgt[3 * j] - x0, d1 = tgt[3 * j + 1] - x1, d2 = tgt[3 * j + 2] - x2;
    finite = finite && (fabs(d0) < kOffsetMax) && (fabs(d1) < kOffsetMax) && (fabs(d2) < kOffsetMax);   // (false for NaN)
    m0 += d0; m1 += d1; m2 += d2;
  }
  m0 /= kn; m1 /= kn; m2 /= kn;
  double d[3] = {0.0, 0.0, 0.0}, a01 = 0.0, a02 = 0.0, a12 = 0.0;   // second pass: Σ (d − mean)(d − mean)ᵀ, neighbour order
  for (int k = 0; k < kn; ++k) {
    int64_t j = nb[k];
    j = j < 0 ? 0 : (j >= M ? M - 1 : j);
    const double c0 = (tgt[3 * j] - x0) - m0, c1 = (tgt[3 * j + 1] - x1) - m1, c2 = (tgt[3 * j + 2] - x2) - m2;
    d[0] += c0 * c0; d[1] += c1 * c1; d[2] += c2 * c2;
    a01 += c0 * c1; a02 += c0 * c2; a12 += c1 * c2;
  }
  double n0, n1, n2;
  normal_from_scatter(d[0], d[1], d[2], a01, a02, a12, finite, n0, n1, n2);   // plane_normal_device.hpp
  double* o = rec + 6 * i;
  o[0] = x0; o[1] = x1; o[2] = x2; o[3] = n0; o[4] = n1; o[5] = n2;
}

// supplied normals: normalised; a zero or non-finite row (or a non-finite point) means "no normal here", and so does a finite
// row whose squared norm overflows or underflows to 0 in f64 (1e160, 1e-170, subnormals): the norm is not scaled
__global__ __launch_bounds__(256) void k_pack_normals(const double* __restrict__ tgt, const double* __restrict__ nrm, int64_t M,
                                                      double* __restrict__ rec) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const double x0 = tgt[3 * i], x1 = tgt[3 * i + 1], x2 = tgt[3 * i + 2];
  double n0 = nrm[3 * i], n1 = nrm[3 * i + 1], n2 = nrm[3 * i + 2];
  const double nn = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
  const bool valid = nn > 0.0 && nn < __builtin_inf() && fabs(x0) < __builtin_inf() && fabs(x1) < __builtin_inf() && fabs(x2) < __builtin_inf();
  double* o = rec + 6 * i;
  o[0] = x0; o[1] = x1; o[2] = x2;
  o[3] = valid ? n0 / nn : 0.0; o[4] = valid ? n1 / nn : 0.0; o[5] = valid ? n2 / nn : 0.0;
}

// ---------------------------------------------------------------------------------------------
// accumulation from the search kernel's winner indices
// ---------------------------------------------------------------------------------------------
// Lane <-> particle by ParticleLanes (lane_fold_device.hpp), U points per wave and loop trip so that the index -> record
// gathers go out as batches, then fold_particle_record: one record per (workgroup, particle).  Ts and d² are the search
// kernel's unfused expressions: the winner was certified for exactly that Ts and the gate compares exactly that d².
template <int PW, int WP, bool TRACE>
__device__ __forceinline__ void plane_body(const PlaneArgs& a, int bx, int by, double* lds) {
  if (a.ctl[0]) return;
  constexpr int U = 2;   // 29 accumulators + the pose: two 48-byte records in flight per lane keep the kernel at three waves per SIMD
  using Lanes = ParticleLanes<PW, WP>;
  constexpr int BW = Lanes::BW, STEP = Lanes::STEP;
  const Lanes L(by);
  const int wb = L.wb, bs = L.bs, pidx = L.pidx;
  const int p = a.p_lo + pidx;
  const bool pvalid = p < a.p_hi;

  double Rt[9], tt[3];
  load_pose(a.Rtot + 12 * (size_t)(pvalid ? p : a.p_lo), Rt, tt);
  double acc[kPlaneSums];
#pragma unroll
  for (int i = 0; i < kPlaneSums; ++i) acc[i] = 0.0;
  const int64_t blk_lo = (int64_t)bx * a.pts_per_block;
  const int64_t blk_hi = (blk_lo + a.pts_per_block < a.B) ? blk_lo + a.pts_per_block : a.B;
  const SVNICP_CONST_AS double* csrc = (const SVNICP_CONST_AS double*)a.src;   // wave-uniform rows become s_load
  const SVNICP_CONST_AS double* crec = (const SVNICP_CONST_AS double*)a.rec;
  const int32_t* kip = a.kidx + pidx;

  auto load_ki = [&](int64_t n) -> int {   // rows are clamped, never predicated: a point past the block only changes `on`
    const int64_t b = n + bs;
    const int64_t bc = b < blk_hi ? b : blk_lo;
    return kip[(size_t)bc * a.Ppad];
  };
  const double delta = a.delta;
  auto accumulate = [&](bool on, double s0, double s1, double s2, const double* q) {
    const double T0 = (s0 * Rt[0] + s1 * Rt[1] + s2 * Rt[2]) + tt[0];   // the search kernel's expression
    const double T1 = (s0 * Rt[3] + s1 * Rt[4] + s2 * Rt[5]) + tt[1];
    const double T2 = (s0 * Rt[6] + s1 * Rt[7] + s2 * Rt[8]) + tt[2];
    const double e0 = T0 - q[0], e1 = T1 - q[1], e2 = T2 - q[2];
    const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
    // the project's gate (squared distance against max_dist, as point mode has it) and a winner that has a normal; a
    // rejected pair contributes exact zeros (selected, not multiplied: a non-finite point must not leak a NaN)
    const bool ok = on && d2 < a.max_dist && (q[3] != 0.0 || q[4] != 0.0 || q[5] != 0.0);
    const double n0 = ok ? q[3] : 0.0, n1 = ok ? q[4] : 0.0, n2 = ok ? q[5] : 0.0;
    const double r = ok ? (n0 * e0 + n1 * e1) + n2 * e2 : 0.0;
    const double ar = fabs(r);
    const double w = ok ? (ar <= delta ? 1.0 : delta / ar) : 0.0;   // Huber: 1 inside delta, delta / |r| outside
    const double z0 = ok ? s0 : 0.0, z1 = ok ? s1 : 0.0, z2 = ok ? s2 : 0.0;
    double j[6], wj[6];
    j[0] = Rt[0] * n0 + Rt[3] * n1 + Rt[6] * n2;   // m = Rtᵀ n
    j[1] = Rt[1] * n0 + Rt[4] * n1 + Rt[7] * n2;
    j[2] = Rt[2] * n0 + Rt[5] * n1 + Rt[8] * n2;
    j[3] = z1 * j[2] - z2 * j[1];                  // s × m
    j[4] = z2 * j[0] - z0 * j[2];
    j[5] = z0 * j[1] - z1 * j[0];
#pragma unroll
    for (int i = 0; i < 6; ++i) wj[i] = w * j[i];
    int e = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int k = i; k < 6; ++k) { acc[e] = fma(wj[i], j[k], acc[e]); ++e; }   // H upper triangle, row-major: 21 sums
    const double wr = w * r;
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] = fma(wr, j[i], acc[21 + i]);     // b
    acc[27] += ok ? 1.0 : 0.0;
    acc[28] = fma(wr, r, acc[28]);
  };

  const int64_t n0 = blk_lo + wb * BW;
  int kin[U];
#pragma unroll
  for (int u = 0; u < U; ++u) kin[u] = load_ki(n0 + u * STEP);
  for (int64_t n = n0; n < blk_hi; n += U * STEP) {  // wave-uniform
    int64_t ti[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t t = kin[u];
      ti[u] = t < 0 ? 0 : (t >= a.M ? a.M - 1 : t);   // clamped like k_build_table3
    }
#pragma unroll
    for (int u = 0; u < U; ++u) kin[u] = load_ki(n + (U + u) * STEP);
    double q[U][6];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const SVNICP_CONST_AS double* r = crec + 6 * ti[u];
#pragma unroll
      for (int i = 0; i < 6; ++i) q[u][i] = r[i];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t b = n + u * STEP + bs;
      const int64_t bl = b < blk_hi ? b : blk_lo;
      const SVNICP_CONST_AS double* sp = csrc + 3 * bl;
      const double s0 = sp[0], s1 = sp[1], s2 = sp[2];
      if (TRACE && a.corr && pvalid && b < blk_hi) a.corr[(size_t)p * a.B + b] = (int)a.kbest[(size_t)b * a.Ppad + pidx];
      accumulate(b < blk_hi, s0, s1, s2, q[u]);
    }
  }

  fold_particle_record(L, acc, lds, a.partial, (size_t)bx * a.Ppad);
}

template <int PW, int WP, bool TRACE>
__global__ __launch_bounds__(NT, 3) void k_plane_accumulate(PlaneArgs a) {
  extern __shared__ __align__(16) double lds[];
  plane_body<PW, WP, TRACE>(a, xcd_block((int)blockIdx.x, (int)gridDim.x), (int)blockIdx.y, lds);
}

// Hb[p] = H (36, mirrored, + 1e-6 on the diagonal) | b (6), stats[p] = {accepted pairs, Σ w·r²} from the workgroups'
// records, added by reduce_block_records (lane_fold_device.hpp): one fixed order of additions, whatever the launch geometry.
__global__ __launch_bounds__(256) void k_plane_finalize(const double* __restrict__ partial, int nblk, int Ppad, int p_lo, int n_particles,
                                                        double* __restrict__ Hb, double* __restrict__ stats, const int* __restrict__ ctl) {
  if (ctl[0]) return;
  const int el = threadIdx.x & 15, bl = threadIdx.x >> 4;
  const int entry = blockIdx.x * 16 + el;  // index into [n_particles][kPlaneSums]
  const int n_entries = n_particles * kPlaneSums;
  const double s = reduce_block_records(partial + entry, (size_t)Ppad * kPlaneSums, nblk, entry < n_entries);
  if (bl == 0 && entry < n_entries) {
    const int p = p_lo + entry / kPlaneSums, e = entry % kPlaneSums;
    double* o = Hb + (size_t)p * 42;
    if (e < 21) {
      int i = 0, rem = e;
      while (rem >= 6 - i) { rem -= 6 - i; ++i; }   // row i of the upper triangle, column i + rem
      const int k = i + rem;
      if (i == k) o[7 * i] = s + 1e-6;
      else { o[6 * i + k] = s; o[6 * k + i] = s; }
    } else if (e < 27) {
      o[36 + (e - 21)] = s;
    } else {
      stats[(size_t)p * 2 + (e - 27)] = s;
    }
  }
}

template <int PW, int WP>
hipError_t launch_p(const AccumPlan& plan, const PlaneArgs& a, hipStream_t st) {
  constexpr int WB = 4 / WP;
  const size_t smem = (size_t)(WB - 1) * (WP * PW) * kPlaneSums * sizeof(double);   // at most 3 * 64 * 29 * 8 = 44.5 KB
  if (a.corr) hipLaunchKernelGGL((k_plane_accumulate<PW, WP, true>), dim3(plan.grid_x, plan.grid_y), dim3(NT), smem, st, a);
  else hipLaunchKernelGGL((k_plane_accumulate<PW, WP, false>), dim3(plan.grid_x, plan.grid_y), dim3(NT), smem, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_target_normals(const double* tgt, int64_t M, const int32_t* nbr, int64_t row_lo, int64_t rows, int kn, double* rec,
                                 hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  if (row_lo < 0 || row_lo + rows > M || kn < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_target_normals, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, tgt, M, nbr, row_lo, rows, kn, rec);
  return hipGetLastError();
}

hipError_t launch_pack_normals(const double* tgt, const double* nrm, int64_t M, double* rec, hipStream_t st) {
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pack_normals, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, tgt, nrm, M, rec);
  return hipGetLastError();
}

// the grid of the split accumulate kernel (plan.grid_x x plan.grid_y workgroups, plan.pts_per_block points each)
hipError_t launch_plane_accumulate(const AccumPlan& plan, PlaneArgs a, hipStream_t st) {
  if (plan.f32 != 3) return hipErrorInvalidValue;   // the kernel consumes the search kernel's winner index
  a.Ppad = plan.Ppad; a.pts_per_block = plan.pts_per_block;
  return dispatch_lanes(plan.PW, plan.WP, [&](auto l) { return launch_p<l.PW, l.WP>(plan, a, st); });
}

hipError_t launch_plane_finalize(const double* partial, int nblk, int Ppad, int p_lo, int n_particles, double* Hb, double* stats,
                                 const int* ctl, hipStream_t st) {
  const int n_entries = n_particles * kPlaneSums;
  if (n_entries <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_plane_finalize, dim3((n_entries + 15) / 16), dim3(256), 0, st, partial, nblk, Ppad, p_lo, n_particles, Hb, stats, ctl);
  return hipGetLastError();
}

}  // namespace svnicp
