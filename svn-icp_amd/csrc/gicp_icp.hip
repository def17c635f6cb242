// gicp_icp.hip — the generalized-ICP residual (svnicp_set_residual_gicp): every pair is weighted by the
// combined covariance of both local surfaces.  An extension: the reference has no such mode.
//
//   k_gicp_accumulate   the shape of k_plane_accumulate (plane_icp.hip): lane <-> particle, consumes the search kernel's winner
//                       index, gathers the winner's 48-byte record xyz | normal, reads the source row from its own packed record
//                       [B][6] = xyz | normal, and adds the pair's terms (gicp_pair_device.hpp) to the 29 sums of the particle.
// Everything around it is plane mode's: the normal pass and the packing of supplied normals (launch_target_normals /
// launch_pack_normals, run on the source cloud as well), k_plane_finalize and the [P][42] / [P][2] records behind it.
#include "kernels.hpp"
#include "lane_fold_device.hpp"
#include "gicp_pair_device.hpp"
#include "stein_common.hpp"

namespace svnicp {

static_assert(kGicpSums == kPlaneSums, "k_plane_finalize reduces the records of both residuals");

namespace {

// Lane <-> particle by ParticleLanes (lane_fold_device.hpp), U points per wave and loop trip, then fold_particle_record: one
// record per (workgroup, particle).  Ts and d² are the search kernel's unfused expressions: the winner was certified for
// exactly that Ts and the gate compares exactly that d².
template <int PW, int WP, bool TRACE>
__device__ __forceinline__ void gicp_body(const GicpArgs& a, int bx, int by, double* lds) {
  if (a.ctl[0]) return;
  // one 48-byte record in flight per lane (the winner index still one trip ahead): 148-156 VGPRs, no scratch, three waves per
  // SIMD.  Two records, as plane_body has them, reach the 168-VGPR limit of three waves and spill 32-84 bytes per lane.
  constexpr int U = 1;
  using Lanes = ParticleLanes<PW, WP>;
  constexpr int BW = Lanes::BW, STEP = Lanes::STEP;
  const Lanes L(by);
  const int wb = L.wb, bs = L.bs, pidx = L.pidx;
  const int p = a.p_lo + pidx;
  const bool pvalid = p < a.p_hi;

  double Rt[9], tt[3];
  load_pose(a.Rtot + 12 * (size_t)(pvalid ? p : a.p_lo), Rt, tt);
  double acc[kGicpSums];
#pragma unroll
  for (int i = 0; i < kGicpSums; ++i) acc[i] = 0.0;
  const int64_t blk_lo = (int64_t)bx * a.pts_per_block;
  const int64_t blk_hi = (blk_lo + a.pts_per_block < a.B) ? blk_lo + a.pts_per_block : a.B;
  const SVNICP_CONST_AS double* csrc = (const SVNICP_CONST_AS double*)a.srec;   // wave-uniform rows become s_load
  const SVNICP_CONST_AS double* crec = (const SVNICP_CONST_AS double*)a.rec;
  const int32_t* kip = a.kidx + pidx;

  auto load_ki = [&](int64_t n) -> int {   // rows are clamped, never predicated: a point past the block only changes `on`
    const int64_t b = n + bs;
    const int64_t bc = b < blk_hi ? b : blk_lo;
    return kip[(size_t)bc * a.Ppad];
  };
  const double delta = a.delta, eps = a.eps;
  auto accumulate = [&](bool on, const double* s, const double* q) {
    const double T0 = (s[0] * Rt[0] + s[1] * Rt[1] + s[2] * Rt[2]) + tt[0];   // the search kernel's expression
    const double T1 = (s[0] * Rt[3] + s[1] * Rt[4] + s[2] * Rt[5]) + tt[1];
    const double T2 = (s[0] * Rt[6] + s[1] * Rt[7] + s[2] * Rt[8]) + tt[2];
    const double e0 = T0 - q[0], e1 = T1 - q[1], e2 = T2 - q[2];
    const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
    // the project's gate (squared distance against max_dist, as point mode has it), a winner that has a normal and a source
    // row that has one
    const bool ok = on && d2 < a.max_dist && (q[3] != 0.0 || q[4] != 0.0 || q[5] != 0.0) && (s[3] != 0.0 || s[4] != 0.0 || s[5] != 0.0);
    const double g0 = ok ? e0 : 0.0, g1 = ok ? e1 : 0.0, g2 = ok ? e2 : 0.0;
    const double h0 = ok ? q[3] : 0.0, h1 = ok ? q[4] : 0.0, h2 = ok ? q[5] : 0.0;
    const double u0 = Rt[0] * g0 + Rt[3] * g1 + Rt[6] * g2;   // u = Rtᵀ e
    const double u1 = Rt[1] * g0 + Rt[4] * g1 + Rt[7] * g2;
    const double u2 = Rt[2] * g0 + Rt[5] * g1 + Rt[8] * g2;
    const double m0 = Rt[0] * h0 + Rt[3] * h1 + Rt[6] * h2;   // m = Rtᵀ n_q
    const double m1 = Rt[1] * h0 + Rt[4] * h1 + Rt[7] * h2;
    const double m2 = Rt[2] * h0 + Rt[5] * h1 + Rt[8] * h2;
    gicp_accumulate_pair(acc, ok, s[0], s[1], s[2], u0, u1, u2, m0, m1, m2, s[3], s[4], s[5], eps, delta);
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
      const SVNICP_CONST_AS double* sp = csrc + 6 * bl;
      double s[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) s[i] = sp[i];
      if (TRACE && a.corr && pvalid && b < blk_hi) a.corr[(size_t)p * a.B + b] = (int)a.kbest[(size_t)b * a.Ppad + pidx];
      accumulate(b < blk_hi, s, q[u]);
    }
  }

  fold_particle_record(L, acc, lds, a.partial, (size_t)bx * a.Ppad);
}

template <int PW, int WP, bool TRACE>
__global__ __launch_bounds__(NT, 3) void k_gicp_accumulate(GicpArgs a) {
  extern __shared__ __align__(16) double lds[];
  gicp_body<PW, WP, TRACE>(a, xcd_block((int)blockIdx.x, (int)gridDim.x), (int)blockIdx.y, lds);
}

template <int PW, int WP>
hipError_t launch_g(const AccumPlan& plan, const GicpArgs& a, hipStream_t st) {
  constexpr int WB = 4 / WP;
  const size_t smem = (size_t)(WB - 1) * (WP * PW) * kGicpSums * sizeof(double);   // at most 3 * 64 * 29 * 8 = 44.5 KB
  if (a.corr) hipLaunchKernelGGL((k_gicp_accumulate<PW, WP, true>), dim3(plan.grid_x, plan.grid_y), dim3(NT), smem, st, a);
  else hipLaunchKernelGGL((k_gicp_accumulate<PW, WP, false>), dim3(plan.grid_x, plan.grid_y), dim3(NT), smem, st, a);
  return hipGetLastError();
}

}  // namespace

// the grid of the split accumulate kernel (plan.grid_x x plan.grid_y workgroups, plan.pts_per_block points each)
hipError_t launch_gicp_accumulate(const AccumPlan& plan, GicpArgs a, hipStream_t st) {
  if (plan.f32 != 3) return hipErrorInvalidValue;   // the kernel consumes the search kernel's winner index
  a.Ppad = plan.Ppad; a.pts_per_block = plan.pts_per_block;
  return dispatch_lanes(plan.PW, plan.WP, [&](auto l) { return launch_g<l.PW, l.WP>(plan, a, st); });
}

}  // namespace svnicp
