// particle_score.hip — svnicp_score_particles / svnicp_set_particle_weighting (include/svnicp_hip.h "score and weight the
// particles"): every particle's total pose scored through the candidate table of the registration, by the
// nearest-of-K rule the iterations use — in the point cost, or (svnicp_score_particles_objective, §4.12.1) in the plane or the
// generalized-ICP residual the solver minimised: k_particle_score's FORM.  Three kernels:
//   k_particle_score           lanes along the particles (ParticleLanes, lane_fold_device.hpp), source rows in LDS tiles: the
//                              K candidate rows of a tile are gathered once, cooperatively (indices coalesced, the target
//                              rows or xyz | normal records behind them), and every particle lane reads them as broadcasts.
//                              Five float64 accumulators per lane; fold_particle_record: one record per (workgroup, particle)
//   k_particle_score_finalize  the records added in reduce_block_records' fixed order, [P][6] with the cost
//   k_particle_weights         one workgroup: cost_min, exp, Z in particle order, the weights
// No atomics, no stop flag (a registration that stopped early is scored at the poses it stopped at).  Workgroup x owns rows
// [64 x, 64 x + 64); inside it row b belongs to slot b mod STEP of the workgroup whatever the tile height, so every
// addition happens in an order that depends on B and P alone.
#include "kernels.hpp"
#include "gicp_pair_device.hpp"
#include "lane_fold_device.hpp"

namespace svnicp {
namespace {

constexpr int NT = 256;
constexpr int kTileBytes = 40 * 1024;   // a tile of candidate rows: three workgroups per CU keep theirs in 160 KB of LDS
constexpr int kTileRowsMax = 16;        // rows of a tile: the row slots of the narrowest geometry (16 particles per wave)
constexpr int kTileBytesMax = 64 * 1024;   // one source row's candidates at most (K = 620 with normals: 29 KB)

// FORM (SVNICP_SCORE_*): 0 = the point cost, 1 = the Huber-weighted plane residual, 2 = the generalized-ICP
// residual.  Staging, the winner loop, the row slots and the fold are shared: only the tail after the winner differs.  Forms 1
// and 2 always stage the 48-byte records; their record is {evaluated, inliers, accepted, sum d2, sum h}.
template <int FORM, int PW, int WP>
__global__ __launch_bounds__(NT) void k_particle_score(ScoreArgs a) {
  extern __shared__ __align__(16) double lds[];
  using Lanes = ParticleLanes<PW, WP>;
  constexpr int BW = Lanes::BW, STEP = Lanes::STEP;
  static_assert(kScoreRowsPerBlock % STEP == 0, "a workgroup's rows are whole trips of its slots");
  const int tid = threadIdx.x;
  const Lanes L((int)blockIdx.y);
  const int pidx = L.pidx;
  const bool pvalid = pidx < a.P;
  const int slot = L.wb * BW + L.bs;

  double Rt[9], tt[3];
  load_pose(a.Rtot + 12 * (size_t)(pvalid ? pidx : 0), Rt, tt);
  const bool normals = FORM != 0 || a.rec != nullptr;
  const int W = normals ? 6 : 3;
  const int K = a.K;
  double ev = 0.0, in = 0.0, pin = 0.0, sd = 0.0, sr = 0.0;   // the counts are exact in float64 (B < 2^31)
  const int64_t blk_lo = (int64_t)blockIdx.x * kScoreRowsPerBlock;
  const int64_t blk_hi = blk_lo + kScoreRowsPerBlock < a.B ? blk_lo + kScoreRowsPerBlock : a.B;

  for (int64_t t0 = blk_lo; t0 < blk_hi; t0 += a.TH) {   // workgroup-uniform
    const int nrows = (int)(blk_hi - t0 < a.TH ? blk_hi - t0 : a.TH);
    __syncthreads();   // the previous tile has been read
    const int32_t* ci = a.cand + (size_t)t0 * K;
    for (int e = tid; e < nrows * K; e += NT) {
      int64_t j = ci[e];
      j = j < 0 ? 0 : (j >= a.M ? a.M - 1 : j);   // never an address outside the target
      double* d = lds + (size_t)e * W;
      if (normals) {
        const double* p = a.rec + 6 * j;
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = p[i];
      } else {
        const double* p = a.tgt + 3 * j;
        d[0] = p[0]; d[1] = p[1]; d[2] = p[2];
      }
    }
    __syncthreads();
    // the rows of this tile whose index inside the workgroup's range is this lane's slot (mod STEP), in ascending order
    const int off = (slot - (int)((t0 - blk_lo) & (STEP - 1)) + STEP) & (STEP - 1);
    for (int r = off; r < nrows; r += STEP) {
      const double* sp = a.src + 3 * (size_t)(t0 + r);
      const double s0 = sp[0], s1 = sp[1], s2 = sp[2];
      const double T0 = (s0 * Rt[0] + s1 * Rt[1] + s2 * Rt[2]) + tt[0];   // the search kernel's expression
      const double T1 = (s0 * Rt[3] + s1 * Rt[4] + s2 * Rt[5]) + tt[1];
      const double T2 = (s0 * Rt[6] + s1 * Rt[7] + s2 * Rt[8]) + tt[2];
      const double* row = lds + (size_t)r * K * W;
      double best;
      int kb = 0;
      {
        const double e0 = T0 - row[0], e1 = T1 - row[1], e2 = T2 - row[2];
        best = ((e0 * e0) + e1 * e1) + e2 * e2;
      }
      for (int k = 1; k < K; ++k) {   // strict '<' from candidate 0: a NaN first distance is never replaced
        const double* q = row + (size_t)k * W;
        const double e0 = T0 - q[0], e1 = T1 - q[1], e2 = T2 - q[2];
        const double d2 = ((e0 * e0) + e1 * e1) + e2 * e2;
        const bool lt = d2 < best;
        best = lt ? d2 : best;
        kb = lt ? k : kb;
      }
      const bool tfin = isfinite(T0) && isfinite(T1) && isfinite(T2);
      const bool evaluated = pvalid && tfin && best == best;
      const bool inlier = evaluated && best < a.thr2;   // +inf is evaluated and never an inlier
      ev += evaluated ? 1.0 : 0.0;
      in += inlier ? 1.0 : 0.0;
      sd += inlier ? best : 0.0;
      if constexpr (FORM != 0) {
        const double* q = row + (size_t)kb * W;
        const bool pli = inlier && (q[3] != 0.0 || q[4] != 0.0 || q[5] != 0.0);
        if constexpr (FORM == 1) {   // form 0's expressions; h(|r|) in r * r's place (delta = +inf: r * r itself)
          const double e0 = pli ? T0 - q[0] : 0.0, e1 = pli ? T1 - q[1] : 0.0, e2 = pli ? T2 - q[2] : 0.0;
          const double n0 = pli ? q[3] : 0.0, n1 = pli ? q[4] : 0.0, n2 = pli ? q[5] : 0.0;
          const double res = (n0 * e0 + n1 * e1) + n2 * e2;
          pin += pli ? 1.0 : 0.0;
          sr += robust_cost(fabs(res), res * res, a.delta);
        } else {                     // k_gicp_accumulate's pair: the row's source normal is one address for every particle lane
          const double* sn = a.srec + 6 * (size_t)(t0 + r);
          const double ns0 = sn[3], ns1 = sn[4], ns2 = sn[5];
          const bool ok = pli && (ns0 != 0.0 || ns1 != 0.0 || ns2 != 0.0);
          const double g0 = ok ? T0 - q[0] : 0.0, g1 = ok ? T1 - q[1] : 0.0, g2 = ok ? T2 - q[2] : 0.0;
          const double h0 = ok ? q[3] : 0.0, h1 = ok ? q[4] : 0.0, h2 = ok ? q[5] : 0.0;
          const double u0 = Rt[0] * g0 + Rt[3] * g1 + Rt[6] * g2;   // u = Rtᵀ e
          const double u1 = Rt[1] * g0 + Rt[4] * g1 + Rt[7] * g2;
          const double u2 = Rt[2] * g0 + Rt[5] * g1 + Rt[8] * g2;
          const double m0 = Rt[0] * h0 + Rt[3] * h1 + Rt[6] * h2;   // m = Rtᵀ n_q
          const double m1 = Rt[1] * h0 + Rt[4] * h1 + Rt[7] * h2;
          const double m2 = Rt[2] * h0 + Rt[5] * h1 + Rt[8] * h2;
          double accepted;
          sr += gicp_pair_cost(ok, u0, u1, u2, m0, m1, m2, ns0, ns1, ns2, a.eps, a.delta, accepted);
          pin += accepted;
        }
      } else if (normals) {
        const double* q = row + (size_t)kb * W;
        const bool pli = inlier && (q[3] != 0.0 || q[4] != 0.0 || q[5] != 0.0);   // a zero row: no normal here
        // a rejected pair's operands are selected to zero, not multiplied: a non-finite point must not leak a NaN
        const double e0 = pli ? T0 - q[0] : 0.0, e1 = pli ? T1 - q[1] : 0.0, e2 = pli ? T2 - q[2] : 0.0;
        const double n0 = pli ? q[3] : 0.0, n1 = pli ? q[4] : 0.0, n2 = pli ? q[5] : 0.0;
        const double res = (n0 * e0 + n1 * e1) + n2 * e2;
        pin += pli ? 1.0 : 0.0;
        sr += res * res;
      }
    }
  }

  double acc[kScoreRecord] = {ev, in, pin, sd, sr};
  if constexpr (Lanes::WB > 1) __syncthreads();   // the last tile has been read: its LDS now carries the waves' records
  fold_particle_record(L, acc, lds, a.partial, (size_t)blockIdx.x * a.Ppad);
}

// scores[p] = {evaluated, inliers, plane inliers, sum d2, sum r2, cost} from the workgroups' records, added by
// reduce_block_records (lane_fold_device.hpp); a workgroup's 16 entries are the five sums of three particles (one entry
// idle).  cost = (sum + (B - count) * cap) / B with (count, sum, cap) = (inliers, sum_d2, thr2) of the point cost, (accepted,
// sum_h, h(max_corr_dist)) of the plane and GICP forms: count_f and sum_f are the two fields' places in the record.
__global__ __launch_bounds__(NT) void k_particle_score_finalize(const double* __restrict__ partial, int nblk, int Ppad, int P, double rows,
                                                                 int count_f, int sum_f, double cap, double* __restrict__ scores) {
  __shared__ double tot[16];
  const int el = threadIdx.x & 15, bl = threadIdx.x >> 4;
  const int p = (int)blockIdx.x * 3 + el / kScoreRecord, f = el % kScoreRecord;
  const bool valid = el < 3 * kScoreRecord && p < P;
  const double s = reduce_block_records(partial + (size_t)p * kScoreRecord + f, (size_t)Ppad * kScoreRecord, nblk, valid);
  if (bl == 0) {
    tot[el] = s;
    if (valid) scores[(size_t)p * kScoreFields + f] = s;
  }
  __syncthreads();
  if (bl == 0 && valid && f == 0) {
    const double cnt = tot[el + count_f], sum = tot[el + sum_f];
    scores[(size_t)p * kScoreFields + 5] = (sum + (rows - cnt) * cap) / rows;
  }
}

// w[p] = exp(-(cost_p - cost_min) / temperature) / Z; the costs are finite (a row that is no inlier costs the finite gate)
__global__ __launch_bounds__(NT) void k_particle_weights(const double* __restrict__ scores, int P, double temperature, double* __restrict__ w) {
  __shared__ double red[NT];
  __shared__ double z;
  const int tid = threadIdx.x;
  double m = scores[5];
  for (int p = tid; p < P; p += NT) { const double c = scores[(size_t)p * kScoreFields + 5]; m = c < m ? c : m; }
  red[tid] = m;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid + s] < red[tid] ? red[tid + s] : red[tid];
    __syncthreads();
  }
  const double cmin = red[0];
  for (int p = tid; p < P; p += NT) w[p] = exp(-(scores[(size_t)p * kScoreFields + 5] - cmin) / temperature);
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int p = 0; p < P; ++p) s += w[p];   // in particle order
    z = s;
  }
  __syncthreads();
  const double Z = z;
  for (int p = tid; p < P; p += NT) w[p] = w[p] / Z;
}

template <int FORM, int PW, int WP>
hipError_t launch_s(const ScoreArgs& a, int grid_y, hipStream_t st) {
  constexpr int WB = 4 / WP;
  const size_t tile = (size_t)a.TH * a.K * (FORM != 0 || a.rec ? 6 : 3) * sizeof(double);
  const size_t red = (size_t)(WB - 1) * (WP * PW) * kScoreRecord * sizeof(double);   // at most 3 * 64 * 5 * 8 = 7.5 KB
  hipLaunchKernelGGL((k_particle_score<FORM, PW, WP>), dim3((unsigned)score_blocks(a.B), grid_y), dim3(NT), tile > red ? tile : red, st, a);
  return hipGetLastError();
}

}  // namespace

int64_t score_blocks(int64_t B) { return (B + kScoreRowsPerBlock - 1) / kScoreRowsPerBlock; }

// the particles across lanes, waves and workgroups as the split stage B lays them out, whatever variant the registration ran
static AccumPlan score_shape(int P, int K) { return stage_b_shape(3, P, K); }

int score_padded_particles(int P, int K) { return score_shape(P, K).Ppad; }

int score_tile_rows(int P, int K, bool normals) {
  const AccumPlan sh = score_shape(P, K);
  if (sh.PW <= 0 || K < 1) return 0;
  const int step = (4 / sh.WP) * (kWave / sh.PW);
  const int64_t row_bytes = (int64_t)K * (normals ? 6 : 3) * (int64_t)sizeof(double);
  int th = (int)(kTileBytes / row_bytes);
  if (th > kTileRowsMax) th = kTileRowsMax;
  if (th > step) th -= th % step;   // whole trips of the workgroup's row slots
  if (th < 1) th = row_bytes <= kTileBytesMax ? 1 : 0;
  return th;
}

hipError_t launch_particle_score(ScoreArgs a, double* scores, hipStream_t st) {
  if (a.B <= 0 || a.M <= 0 || a.P <= 0 || a.K < 1) return hipErrorInvalidValue;
  const AccumPlan sh = score_shape(a.P, a.K);
  a.Ppad = sh.Ppad;
  if (a.form < 0 || a.form > 2 || (a.form != 0 && !a.rec) || (a.form == 2 && !a.srec)) return hipErrorInvalidValue;
  a.TH = score_tile_rows(a.P, a.K, a.form != 0 || a.rec != nullptr);
  if (a.TH < 1) return hipErrorInvalidValue;   // refused, never overflowed
  const hipError_t e = dispatch_lanes(sh.PW, sh.WP, [&](auto l) {
    if (a.form == 1) return launch_s<1, l.PW, l.WP>(a, sh.grid_y, st);
    if (a.form == 2) return launch_s<2, l.PW, l.WP>(a, sh.grid_y, st);
    return launch_s<0, l.PW, l.WP>(a, sh.grid_y, st);
  });
  if (e != hipSuccess) return e;
  // the point cost: a row that is no inlier costs the gate; the other forms: a row that is not accepted costs h(gate)
  const bool point = a.form == 0;
  hipLaunchKernelGGL(k_particle_score_finalize, dim3((a.P + 2) / 3), dim3(NT), 0, st, a.partial, (int)score_blocks(a.B), a.Ppad, a.P,
                     (double)a.B, point ? 1 : 2, point ? 3 : 4, point ? a.thr2 : a.cap, scores);
  return hipGetLastError();
}

hipError_t launch_particle_weights(const double* scores, int P, double temperature, double* w, hipStream_t st) {
  if (P <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_particle_weights, dim3(1), dim3(NT), 0, st, scores, P, temperature, w);
  return hipGetLastError();
}

}  // namespace svnicp
