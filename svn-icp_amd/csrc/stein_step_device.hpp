// stein_step_device.hpp — the device pieces of the per-iteration Stein step, each stated once.  Included by
// particle_update.hip (the Stein-step kernels and their launchers), small_registration.hip (the persistent kernel runs the
// same bodies on virtual blocks) and stein_iter.hip (the one-particle step in k_icp_single's last workgroup).
//
// Replaces (SVN mode) the tail of SVNICP::stein_align per iteration (src/core/SVNICP.cpp:71-107):
//   Newton_grad_right's finalisation H + 1e-6·I, linalg::solve (SVNICP.cpp:149-162)   particle_Hb, newton_step
//   rbf_hessian_kernel incl. torch::median (:254-266)                                  rbf_bandwidth / median_body, block_select
//   svgd_grad (:218-227), svn_full_grad (:229-252), SVGD-ICP's svgd_grad               stein_direction_{default,full,svgd}
//   pose_update (:268-279), pose_particles_ (:103-106)                                 pose_update
//   the early-stop test (:95-101, on the device: no per-iteration host sync)           one_workgroup_finish / finish_body
// The library is built with -ffp-contract=off: a function inlined into several kernels performs the same roundings in
// each of them.  What differs between the launch shapes — the order of a sum over particles — stays with the shape.
#pragma once
#include "kernels.hpp"

namespace svnicp {
namespace {

constexpr int UT = 512;     // threads of the update workgroup (2 waves per SIMD: up to 256 VGPRs, no spills)
constexpr int KREG = 32;    // pairwise-distance keys a thread keeps in registers for the median (n <= KREG*UT)

// debug option: cycles of ONE thread (`mine`) between phase boundaries, added to dbg[i]
struct PhaseStamp {
  unsigned long long* dbg;
  unsigned long long t;
  __device__ PhaseStamp(unsigned long long* d, bool mine) : dbg(mine ? d : nullptr), t(d ? __builtin_readcyclecounter() : 0ull) {}
  __device__ __forceinline__ void operator()(int i) {
    if (!dbg) return;
    const unsigned long long now = __builtin_readcyclecounter();
    dbg[i] += now - t;
    t = now;
  }
};

// H (6x6) and b (6) of one particle from its 22 raw sums and Rc = R0·R  (see stein_iter.hip)
__device__ inline void finalize_Hb(const double* s, const double* Rc, double* H, double* b) {
  const double sw = s[0];
  const double a0 = s[1], a1 = s[2], a2 = s[3];
  const double xx = s[4], xy = s[5], xz = s[6], yy = s[7], yz = s[8], zz = s[9];
  const double tr = xx + yy + zz;
#pragma unroll
  for (int i = 0; i < 36; ++i) H[i] = 0.0;
  H[0] = H[7] = H[14] = sw;                      // Σ w·I
  // top-right −Σw·ŝ, bottom-left +Σw·ŝ with ŝ = [[0,−s2,s1],[s2,0,−s0],[−s1,s0,0]]
  H[0 * 6 + 4] = a2;  H[0 * 6 + 5] = -a1;
  H[1 * 6 + 3] = -a2; H[1 * 6 + 5] = a0;
  H[2 * 6 + 3] = a1;  H[2 * 6 + 4] = -a0;
  H[3 * 6 + 1] = -a2; H[3 * 6 + 2] = a1;
  H[4 * 6 + 0] = a2;  H[4 * 6 + 2] = -a0;
  H[5 * 6 + 0] = -a1; H[5 * 6 + 1] = a0;
  // bottom-right Σw(‖s‖²I − ssᵀ)
  H[3 * 6 + 3] = tr - xx; H[3 * 6 + 4] = -xy;     H[3 * 6 + 5] = -xz;
  H[4 * 6 + 3] = -xy;     H[4 * 6 + 4] = tr - yy; H[4 * 6 + 5] = -yz;
  H[5 * 6 + 3] = -xz;     H[5 * 6 + 4] = -yz;     H[5 * 6 + 5] = tr - zz;
#pragma unroll
  for (int i = 0; i < 6; ++i) H[7 * i] += 1e-6;  // SVNICP.cpp:153
  // b_t = Rcᵀ Σwe ; b_r = vee-part of G = Rcᵀ·C, C[i][j] = Σ (we)_i s_j
  mat3T_vec(Rc, s + 10, b);
  double G[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) G[3 * i + j] = Rc[i] * s[13 + j] + Rc[3 + i] * s[16 + j] + Rc[6 + i] * s[19 + j];
  b[3] = G[7] - G[5];  // s_y u_z − s_z u_y  with u_i s_j = G[i][j]
  b[4] = G[2] - G[6];
  b[5] = G[3] - G[1];
}

// point-to-plane mode: H and b come finished from k_plane_finalize (UpdateArgs::plane_Hb)
__device__ __forceinline__ void load_plane_Hb(const double* rec, double* H, double* b) {
#pragma unroll
  for (int i = 0; i < 36; ++i) H[i] = rec[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) b[i] = rec[36 + i];
}

// HBM workspace (doubles): H[P][36] b[P][6] N[P][6] x[P][6] phi[P][6] sq[P][P].  The update kernel
// works out of LDS copies of x, N, b (and H when it fits); HBM keeps H for the traces, sq only for
// particle counts whose P² keys do not fit the register budget.
struct Work {
  double *H, *b, *N, *x, *phi, *sq;
  __device__ Work(double* w, int P) {
    H = w; b = H + (size_t)P * 36; N = b + (size_t)P * 6; x = N + (size_t)P * 6; phi = x + (size_t)P * 6;
    sq = phi + (size_t)P * 6;
  }
};

// The 22 raw sums of particle p.  One rank (or particle sharding): the context's own record.  Source-row sharding
// (svnicp_set_row_shard): a.sums is the all-gathered [n_ranks][P][22] array of the ranks' partial records — rank r summed
// its own source rows — and every rank adds the same records in the same (rank) order, so the replicas stay bit-identical.
// Small registrations (api.hip: small chain): a.sums is the accumulate kernel's `partial` array itself — one record per
// workgroup, record stride sums_stride — added here in block order: no k_reduce_partials launch.
__device__ __forceinline__ void load_sums(const UpdateArgs& a, int p, double* s) {
  const double* rec = a.sums + (size_t)p * kNSums;
  const size_t stride = a.sums_stride ? (size_t)a.sums_stride : (size_t)a.P * kNSums;
#pragma unroll
  for (int i = 0; i < kNSums; ++i) s[i] = rec[i];
  for (int r = 1; r < a.n_ranks; ++r) {
    rec += stride;
#pragma unroll
    for (int i = 0; i < kNSums; ++i) s[i] += rec[i];
  }
}

// H (+1e-6·I) and b of particle p (SVNICP.cpp:146-157): the plane record where the context holds one (point-to-plane mode;
// wave-uniform, never taken in point mode), else from the particle's 22 sums.  Those come from load_sums; kKeepSums (small
// chain) also leaves the reduced record where k_reduce_partials would have (svnicp_sums_devptr); kGivenSums: the caller holds
// the reduced record already (`given`).
enum SumsFrom { kLoadSums, kKeepSums, kGivenSums };
template <SumsFrom FROM = kLoadSums>
__device__ __forceinline__ void particle_Hb(const UpdateArgs& a, int p, double* H, double* b, const double* given = nullptr) {
  double Rc[9];
  mat3_mul(a.pose.R0, a.R + 9 * p, Rc);
  if (a.plane_Hb) { load_plane_Hb(a.plane_Hb + (size_t)p * 42, H, b); return; }
  if constexpr (FROM == kGivenSums) {
    finalize_Hb(given, Rc, H, b);
  } else {
    double sm[kNSums];
    load_sums(a, p, sm);
    if (FROM == kKeepSums && a.sums_out) {
#pragma unroll
      for (int i = 0; i < kNSums; ++i) a.sums_out[(size_t)p * kNSums + i] = sm[i];
    }
    finalize_Hb(sm, Rc, H, b);
  }
}

// Newton step N = H⁻¹b (linalg::solve, SVNICP.cpp:162); NaN where H is singular
__device__ __forceinline__ void newton_step(const double* H, const double* b, double* N) {
  double LU[36];
  int piv[6];
#pragma unroll
  for (int i = 0; i < 36; ++i) LU[i] = H[i];
  const bool ok = lu6(LU, piv);
#pragma unroll
  for (int i = 0; i < 6; ++i) N[i] = b[i];
  lu6_solve(LU, piv, N);
#pragma unroll
  for (int i = 0; i < 6; ++i) N[i] = ok ? N[i] : __builtin_nan("");
}

// column c of M⁻¹ (linalg::inv of the mean Hessian, SVNICP.cpp:225), stored with row stride 6; NaN where M is singular
__device__ __forceinline__ void inverse_column(const double* M, int c, double* inv) {
  double LU[36], col[6];
  int piv[6];
#pragma unroll
  for (int i = 0; i < 36; ++i) LU[i] = M[i];
  const bool ok = lu6(LU, piv);
#pragma unroll
  for (int r = 0; r < 6; ++r) col[r] = (r == c) ? 1.0 : 0.0;
  lu6_solve(LU, piv, col);
#pragma unroll
  for (int r = 0; r < 6; ++r) inv[6 * r + c] = ok ? col[r] : __builtin_nan("");
}

// pose update of particle p by the Stein direction phi (SVNICP.cpp:268-279): R ← R·Exp(phi_r), t ← t + R_new·J_l·phi_t, and
// the next iteration's total pose (SVNICP.cpp:58-59) are stored; the new [t ; Log R] (pose_particles_, SVNICP.cpp:103-106) and
// the step norm are returned — where they go differs between the launch shapes.
struct PoseStep { double x[6]; double norm; };
__device__ __forceinline__ PoseStep pose_update(const UpdateArgs& a, int p, const double* phi) {
  PoseStep s;
  double dR[9], Jl[9], dt[3], Rn[9], Rdt[3], Ro[9];
  so3_exp(phi + 3, dR, Jl);
  mat3_vec(Jl, phi, dt);
#pragma unroll
  for (int i = 0; i < 9; ++i) Ro[i] = a.R[9 * p + i];
  mat3_mul(Ro, dR, Rn);
  mat3_vec(Rn, dt, Rdt);                                    // uses the UPDATED R (:277-278)
#pragma unroll
  for (int i = 0; i < 3; ++i) s.x[i] = Rdt[i] + a.t[3 * p + i];
#pragma unroll
  for (int i = 0; i < 9; ++i) a.R[9 * p + i] = Rn[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) a.t[3 * p + i] = s.x[i];
  double Rt[9], tt[3];
  mat3_mul(a.pose.R0, Rn, Rt);
  mat3_vec(a.pose.R0, s.x, tt);
#pragma unroll
  for (int i = 0; i < 9; ++i) a.Rtot[12 * p + i] = Rt[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) a.Rtot[12 * p + 9 + i] = a.pose.t0[i] + tt[i];
  double n2 = 0.0;
#pragma unroll
  for (int d = 0; d < 6; ++d) n2 += phi[d] * phi[d];
  s.norm = sqrt(n2);
  so3_log(Rn, s.x + 3);
#pragma unroll
  for (int d = 0; d < 6; ++d) a.pose_out[d * a.P + p] = s.x[d];
  return s;
}
// particle p's entries of this iteration's history row (SVNICP.cpp:103-107; SVGDICP.cpp:133)
__device__ __forceinline__ void history_one(const UpdateArgs& a, int p, const double* x6) {
  float* hrow = a.history + (size_t)a.iteration * 6 * a.P;
#pragma unroll
  for (int d = 0; d < 6; ++d) hrow[d * a.P + p] = (float)x6[d];
}

// P = 1 (SVNICP.cpp:81-89: no kernel, no repulsion — the Stein direction is the Newton step itself, phi = −H⁻¹b): the whole
// step of the only particle, run by ONE thread.  `s` = the particle's 22 reduced sums.
__device__ inline void update_single_particle(const UpdateArgs& a, const double* s) {
  double H[36], b[6], N[6], phi[6];
  particle_Hb<kGivenSums>(a, 0, H, b, s);
  newton_step(H, b, N);
#pragma unroll
  for (int i = 0; i < 6; ++i) phi[i] = -N[i];                // SVNICP.cpp:89
  if (a.trH) {   // traces (tests only)
#pragma unroll
    for (int i = 0; i < 36; ++i) a.trH[i] = H[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) { a.trb[i] = b[i]; a.trN[i] = N[i]; a.trphi[i] = phi[i]; }
    *a.trh = __builtin_nan("");                             // no bandwidth with one particle
  }
  const PoseStep st = pose_update(a, 0, phi);
  if (a.check_early_stop && (float)st.norm < (float)a.conv_thr) {   // float32 compare (SVNICP.cpp:42,96-97)
    a.ctl[0] = 1; a.ctl[1] = a.iteration + 1;
    return;                                                 // the stopping epoch's history row stays zero
  }
  history_one(a, 0, st.x);
}

// shared state of the exact-median selection
struct SelShared {
  unsigned int hist[256];
  unsigned long long prefix;
  unsigned int rank;
  int nan_flag;
  double h;
};
// rank of the lower median among the P² pair distances (torch::median)
__device__ __forceinline__ unsigned int lower_median_rank(int P) { return (unsigned int)(((size_t)P * P - 1) / 2); }
__device__ __forceinline__ void sel_init(SelShared* S, unsigned int rank, unsigned long long prefix0, int tid) {
  if (tid < 256) S->hist[tid] = 0;
  if (tid == 0) { S->nan_flag = 0; S->prefix = prefix0; S->rank = rank; S->h = __builtin_nan(""); }
}

__device__ __forceinline__ double pair_sq(const double* lx, int i, int j) {  // SVNICP.cpp:257-260
  double s = 0.0;
#pragma unroll
  for (int d = 0; d < 6; ++d) { const double df = lx[i * 6 + d] - lx[j * 6 + d]; s += df * df; }
  return s;
}

// Block-wide exact rank selection over non-negative f64 keys: one 8-bit radix pass per digit from first_pass down (the digits
// above it are S->prefix: keys known to share those bits), two barriers per pass, the 256-bin scan runs in wave 0.
// each_key(f) calls f(k) for every key the calling thread holds.  S as sel_init left it and a barrier since; returns the
// key of rank S->rank.
template <class Each>
__device__ __forceinline__ unsigned long long block_select(Each each_key, int first_pass, SelShared* S, int lane, int wave) {
  for (int pass = first_pass; pass >= 0; --pass) {
    const int shift = pass * 8;
    const unsigned long long pre = S->prefix;
    each_key([&](unsigned long long k) {
      if (pass == 7 || (k >> (shift + 8)) == pre) atomicAdd(&S->hist[(k >> shift) & 255ull], 1u);
    });
    __syncthreads();
    if (wave == 0) {
      unsigned int c[4], tot = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) { c[i] = S->hist[4 * lane + i]; tot += c[i]; S->hist[4 * lane + i] = 0; }
      unsigned int incl = tot;
#pragma unroll
      for (int off = 1; off < kWave; off <<= 1) {
        const unsigned int v = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += v;
      }
      unsigned int cum = incl - tot;  // elements in bins before mine
      const unsigned int rank = S->rank;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (rank >= cum && rank < cum + c[i]) {
          S->prefix = (pre << 8) | (unsigned long long)(4 * lane + i);
          S->rank = rank - cum;
        }
        cum += c[i];
      }
    }
    __syncthreads();
  }
  return S->prefix;
}

// h = median(all P² pair distances) / log(P+1)  (SVNICP.cpp:254-262 / SVGDICP.cpp:464-471): exact lower
// median (torch::median) by an 8-pass block_select on the f64 bit patterns; keys stay in registers when
// P² <= KREG*T.  Block-wide call; S = sel_init(S, lower_median_rank(P), 0, tid) and a barrier since.
template <int T>   // T: threads of the calling workgroup
__device__ __attribute__((noinline)) void rbf_bandwidth(const double* lx, int P, double* sq_global, SelShared* S, int tid, int lane, int wave) {
  const int n = P * P;
  const bool keys_in_regs = n <= KREG * T;
  const float invP = 1.0f / (float)P;
  unsigned long long key[KREG];
  if (keys_in_regs) {
#pragma unroll
    for (int i = 0; i < KREG; ++i) {
      const int e = i * T + tid;
      key[i] = ~0ull;
      if (e < n) {
        int r = (int)((float)e * invP);
        if (r * P > e) --r;
        if ((r + 1) * P <= e) ++r;
        const double s = pair_sq(lx, r, e - r * P);
        key[i] = (unsigned long long)__double_as_longlong(s);
        if (s != s) S->nan_flag = 1;
      }
    }
  } else {
    for (int e = tid; e < n; e += T) {
      const int r = e / P;
      const double s = pair_sq(lx, r, e - r * P);
      sq_global[e] = s;
      if (s != s) S->nan_flag = 1;
    }
    __syncthreads();
  }
  const int nk = (n - tid + T - 1) / T;   // keys this thread holds in registers
  block_select([&](auto count) {
    if (keys_in_regs) {
#pragma unroll
      for (int i = 0; i < KREG; ++i)
        if (i < nk) count(key[i]);
    } else {
      for (int e = tid; e < n; e += T) count((unsigned long long)__double_as_longlong(sq_global[e]));
    }
  }, 7, S, lane, wave);
  if (tid == 0) {
    const double med = S->nan_flag ? __builtin_nan("") : __longlong_as_double((long long)S->prefix);
    S->h = med / log((double)(P + 1));
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------
// Large particle sets (P > 256: several GPUs' shards, or C4 on one GPU): the same per-iteration
// Stein step as k_particle_update, cut into workgroup-parallel kernels so that the O(P²) pair work
// runs on the whole chip instead of one CU.  Same arithmetic per particle.  The exact lower median of
// the P² pair distances comes from two parallel passes over the pairs: (1) a histogram of the f64 keys
// in logarithmic bins (48 octaves from 2^-40, 256 mantissa steps each; everything outside lands in the
// edge bins) locates the bin holding the median and the rank inside it; (2) the keys of that one bin
// (~0.4 % of the pairs) are collected and an exact radix select runs on them.  Deterministic, no
// sampling, exact for any input (a degenerate distribution only makes the last select longer).  The three kernels
// (k_upd_hist, k_upd_collect, k_upd_select) are in particle_update.hip; every body below uses the control area they share:
// uctl doubles: [2] h  [3..38] Hinv ; as u64: [40] nan flag [42] median bin [43] rank inside
// the bin [44] collected count ; [64 .. 64+P) step norms ; then the global histogram (u32 x HB_NB).
// ---------------------------------------------------------------------------------------------
constexpr int UCTL_H = 2, UCTL_HINV = 3, UCTL_NAN = 40, UCTL_BIN = 42, UCTL_RANK = 43, UCTL_CNT = 44,
              UCTL_NORM = 64;
constexpr int HB_OCT = 48, HB_NB = HB_OCT * 256, HB_EXP0 = 1023 - 40;
constexpr int SEL_LDS_KEYS = 16384;
constexpr int COLL_CHUNK = 4096;   // pairs per collect chunk = capacity of its LDS staging buffer

__device__ __forceinline__ int key_bin(unsigned long long k) {
  const long long kb = (long long)(k >> 44) - ((long long)HB_EXP0 << 8);
  return kb < 0 ? 0 : (kb >= HB_NB ? HB_NB - 1 : (int)kb);
}
__device__ __forceinline__ unsigned int* upd_hist(double* uctl, int P) {
  return reinterpret_cast<unsigned int*>(uctl + UCTL_NORM + ((P + 7) & ~7));
}

// SVGD-ICP pieces shared by the one-workgroup kernel and the chain (defined at the end of this file)
__device__ void svgd_gradient(const UpdateArgs& a, int p, double* g6);
__device__ double svgd_step_one(const UpdateArgs& a, int p, const double* phi6, const double* xold6);

// ---- the sums-dependent half of the Stein step: k_upd_prepare ----------------------------------------------------------
// Per particle: H (+1e-6·I), b and the Newton step N = H⁻¹b (SVNICP.cpp:146-162) — in SVGD-ICP mode the first-order
// gradient goes into the N slot (SVGDICP.cpp:398-455); for the default SVN branch also the mean Hessian (summed in particle
// order) and its inverse (SVNICP.cpp:85,225).  It needs the sums and nothing else; the other half of the step (the pair
// statistics: k_upd_median or the k_upd_hist chain) needs the poses and nothing else and runs on a second stream beside the
// search and accumulate kernels.  Workgroups 0 … ceil(P/64)−1: one particle per lane of wave 0 (a 6x6 LU per lane is a long
// serial chain: 64 per workgroup spreads it over the chip); the last workgroup: the mean Hessian from ITS OWN finalisation
// of every particle (no workgroup waits for another) and the inverse.
// Measured and dropped in round 3: running this as the tail of k_reduce_partials (its last workgroup, one ticket per
// workgroup) — as one workgroup for all particles 20 us, with one reduce workgroup per particle + a ticketed mean 28 us,
// against 6 + 8 us for the two launches: a serial tail on one CU costs more than the launch it saves.
constexpr int PREP_T = 256, PREP_CH = 128, PREP_PW = 64;
struct PrepShared { double H[PREP_CH][37]; double Hmean[36]; };   // 37.3 KB

// bx: workgroup index inside the prepare part of the launch (the block may have more than PREP_T threads: the others only
// pass the barriers)
__device__ __forceinline__ void prepare_body(const UpdateArgs& a, int bx) {
  if (a.ctl[0]) return;
  __shared__ PrepShared sh;
  const int tid = threadIdx.x, P = a.P;
  Work w(a.work, P);
  const int n_pw = (P + PREP_PW - 1) / PREP_PW;
  if (bx < n_pw) {
    const int p = bx * PREP_PW + tid;
    if (tid >= PREP_PW || p >= P) return;
    if (a.svgd) {
      double g6[6];
      svgd_gradient(a, p, g6);
#pragma unroll
      for (int d = 0; d < 6; ++d) w.N[p * 6 + d] = g6[d];
      return;
    }
    double H[36], b[6], N[6];
    particle_Hb<kKeepSums>(a, p, H, b);
#pragma unroll
    for (int i = 0; i < 36; ++i) w.H[(size_t)p * 36 + i] = H[i];
    newton_step(H, b, N);
#pragma unroll
    for (int i = 0; i < 6; ++i) { w.b[p * 6 + i] = b[i]; w.N[p * 6 + i] = N[i]; }
    return;
  }
  // last workgroup (launched only for the default SVN branch): mean Hessian and its inverse
  double hsum = 0.0;                   // thread e < 36: Σ_p H_p[e], particle order
  for (int c0 = 0; c0 < P; c0 += PREP_CH) {
    const int p = c0 + tid;
    if (tid < PREP_CH && p < P) {
      double H[36], b[6];
      particle_Hb(a, p, H, b);
#pragma unroll
      for (int i = 0; i < 36; ++i) sh.H[tid][i] = H[i];
    }
    __syncthreads();
    const int cnt = P - c0 < PREP_CH ? P - c0 : PREP_CH;
    if (tid < 36)
      for (int q = 0; q < cnt; ++q) hsum += sh.H[q][tid];
    __syncthreads();
  }
  if (tid < 36) sh.Hmean[tid] = hsum / P;                     // mean over particles (SVNICP.cpp:85)
  __syncthreads();
  if (tid < 6) inverse_column(sh.Hmean, tid, a.uctl + UCTL_HINV);   // one column per lane
}

// "bin holding rank r" of a histogram of HB_NB bins, by a workgroup of T threads: a contiguous chunk of bins per thread, an
// inclusive scan of the chunk sums inside the wavefront, then the wave totals (wave_tot: T / 64 words of LDS).  The thread
// that owns the bin calls hit(bin, rank inside the bin); the caller's next barrier publishes what hit() stored.
template <int T, class Hit>
__device__ __forceinline__ void bin_of_rank(const unsigned int* hist, unsigned int rank, unsigned int* wave_tot, Hit hit) {
  constexpr int CH = HB_NB / T;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  unsigned int c[CH], tot = 0;
#pragma unroll
  for (int i = 0; i < CH; ++i) { c[i] = hist[tid * CH + i]; tot += c[i]; }
  unsigned int incl = tot;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const unsigned int v = __shfl_up(incl, off, kWave);
    if (lane >= off) incl += v;
  }
  if (lane == kWave - 1) wave_tot[wave] = incl;
  __syncthreads();
  unsigned int cum = incl - tot;
  for (int wv = 0; wv < wave; ++wv) cum += wave_tot[wv];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    if (rank >= cum && rank < cum + c[i]) hit(tid * CH + i, rank - cum);
    cum += c[i];
  }
}

// The pair statistics of the Stein step for 2 <= P <= 128, one workgroup: the exact lower median of the P² pair distances
// (torch::median over all entries incl. the diagonal's zeros, SVNICP.cpp:262) through an LDS copy of the log-binned
// histogram of the k_upd_* chain — bin the keys, find the median's bin, collect that bin (~0.4 % of the keys), rank its keys
// by counting — and with it the bandwidth h.  Needs the poses only (x = pose_particles_ = [t ; Log R], which the last pose
// update left in pose_out), so it is launched on the context's second stream at the START of an iteration and runs beside
// the search and accumulate kernels; k_upd_direction (one wavefront per particle, pose update fused) waits for it.
// Measured (debug stamps): the 8-pass LDS radix select took 60 % of the fused kernel's 63 us; this kernel takes 13.5 us.
constexpr int FRONT_BUF = 2048;  // keys of the median's bin held in LDS (+8 slack for the unrolled ranking); more (degenerate input) -> 8-pass select
template <int T>   // T: threads of the workgroup (UT in k_upd_median and k_upd_prepare_median, 256 inside the persistent small-registration kernel)
__device__ __forceinline__ void median_body(const UpdateArgs& a) {
  if (a.ctl[0]) return;
  extern __shared__ __align__(16) double dyn[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int P = a.P;
  Work w(a.work, P);
  double* lx = dyn;                                                   // [P][6]
  double* lbuf = dyn + 6 * P;                                         // [FRONT_BUF]
  unsigned int* lh = reinterpret_cast<unsigned int*>(lbuf + FRONT_BUF + 8);  // [HB_NB]
  __shared__ SelShared sel;
  __shared__ unsigned int sh_scan[T / kWave];
  __shared__ unsigned int sh_cnt;
  __shared__ int sh_bin, sh_rank, sh_nan;

  PhaseStamp stamp(a.dbg, tid == 0);   // thread-0 cycles per phase of the median workgroup
  for (int e = tid; e < HB_NB; e += T) lh[e] = 0u;
  if (tid == 0) { sh_cnt = 0u; sh_nan = 0; sh_bin = 0; sh_rank = 0; }
  for (int p = tid; p < P; p += T) {   // x = pose_particles_ (SVNICP.cpp:74-77,103-106; SVGD-ICP: as it stands, SVGDICP.cpp:106-110)
#pragma unroll
    for (int d = 0; d < 6; ++d) { const double v = a.pose_out[d * P + p]; lx[p * 6 + d] = v; w.x[p * 6 + d] = v; }
  }
  __syncthreads();
  stamp(0);

  // pass 1 over the pairs: log-binned histogram.  The matrix of pair distances is symmetric bit for bit ((a-b)² == (b-a)²)
  // with zeros on the diagonal: only the pairs i < j are binned, each with weight 2, and the P diagonal zeros go in with
  // one update — half the distance evaluations and half the LDS atomics (which pile up on a few bins: 46 % of this
  // workgroup's time went into this pass)
  const int n = P * P;
  bool nan = false;
  // the pairs i < j as a rectangle of Pe/2 rows x (Pe - 1) columns (Pe = P rounded up to even): row a holds (a, c + 1) for
  // c >= a and (Pe - 1 - a, Pe - 1 - c) for c < a — every unordered pair exactly once, so all lanes work in every step
  constexpr int KH = ((KREG + 1) / 2 + 1) * (512 / T);   // steps per thread: KH * T >= (Pe / 2)(Pe - 1) for P <= 128
  const int Pe = P + (P & 1), W = Pe - 1, npair = (Pe / 2) * W;
  const int di = T / W, dj = T - di * W;   // pair index advance per step of T entries
  double keys[KH];                           // this thread's pair distances with i < j
  const int bin0 = key_bin(0ull);            // bin of +0.0
  if (tid == 0) atomicAdd(&lh[bin0], (unsigned int)P);
  for (int p = tid; p < P; p += T) { const double sq = pair_sq(lx, p, p); if (sq != sq) nan = true; }   // a non-finite particle: inf - inf on the diagonal
  {
    int ra = tid / W, c = tid - ra * W;
#pragma unroll
    for (int k = 0; k < KH; ++k) {
      const int e = tid + k * T;
      keys[k] = -1.0;                        // "no key": the keys are non-negative, and +inf is a key (an overflowed distance)
      const int i = c >= ra ? ra : Pe - 1 - ra, j = c >= ra ? c + 1 : Pe - 1 - c;
      if (e < npair && j < P) {              // (j < P also implies i < P; only an odd P has a virtual last index)
        const double sq = pair_sq(lx, i, j);
        if (sq != sq) nan = true;
        keys[k] = sq;
        atomicAdd(&lh[key_bin((unsigned long long)__double_as_longlong(sq))], 2u);
      }
      c += dj; ra += di;
      if (c >= W) { c -= W; ++ra; }
    }
  }
  if (nan) sh_nan = 1;
  __syncthreads();
  stamp(1);
  // bin of the lower median
  bin_of_rank<T>(lh, (unsigned int)((n - 1) / 2), sh_scan, [&](int bin, unsigned int inside) { sh_bin = bin; sh_rank = (int)inside; });
  __syncthreads();
  stamp(2);
  // pass 2: the keys of that bin (one copy of each i < j pair)
  const int bstar = sh_bin;
#pragma unroll
  for (int k = 0; k < KH; ++k) {
    if (keys[k] >= 0.0 && key_bin((unsigned long long)__double_as_longlong(keys[k])) == bstar) {
      const unsigned int pos = atomicAdd(&sh_cnt, 1u);
      if (pos < FRONT_BUF) lbuf[pos] = keys[k];
    }
  }
  __syncthreads();
  stamp(3);
  const int m = (int)sh_cnt;
  double med;
  if (m <= FRONT_BUF) {
    // exact rank inside the bin by counting, every collected key standing for two matrix entries and the diagonal for P
    // zeros: the value with #less <= r < #less + #equal is the median
    const int r = sh_rank;
    const bool zin = bstar == bin0;          // the diagonal's zeros are in this bin
    for (int e = m + tid; e < ((m + 7) & ~7); e += T) lbuf[e] = __builtin_nan("");  // pad to the unroll width: neither below nor equal to any key
    __syncthreads();
    for (int e = tid; e < m; e += T) {
      const double v = lbuf[e];
      int lt = 0, eq = 0;
      for (int j0 = 0; j0 < m; j0 += 8) {  // eight broadcast reads in flight
        double u[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) u[t] = lbuf[j0 + t];
#pragma unroll
        for (int t = 0; t < 8; ++t) { lt += u[t] < v ? 1 : 0; eq += u[t] == v ? 1 : 0; }
      }
      const int LT = 2 * lt + ((zin && 0.0 < v) ? P : 0), EQ = 2 * eq + ((zin && v == 0.0) ? P : 0);
      if (LT <= r && r < LT + EQ) sel.h = v;  // every matching thread writes the same value
    }
    if (zin && tid == 0) {                    // the median may be one of the diagonal's zeros
      int eq0 = 0;
      for (int j = 0; j < m; ++j) eq0 += lbuf[j] == 0.0 ? 1 : 0;
      if (r < 2 * eq0 + P) sel.h = 0.0;
    }
    __syncthreads();
    med = sel.h;
  } else {  // degenerate distribution (most pairs in one bin): the general 8-pass select
    sel_init(&sel, lower_median_rank(P), 0ull, tid);
    __syncthreads();
    rbf_bandwidth<T>(lx, P, w.sq, &sel, tid, lane, wave);
    med = sel.h * log((double)(P + 1));  // rbf_bandwidth returns h, undo its scaling
    __syncthreads();
  }
  stamp(4);
  if (tid == 0) a.uctl[UCTL_H] = (sh_nan ? __builtin_nan("") : med) / log((double)(P + 1));  // SVNICP.cpp:262
}

// RBF kernel value of the pair (x_i, x_j) (SVNICP.cpp:257-264) and the difference df = x_i − x_j
__device__ __forceinline__ double rbf_pair(const double* xi, const double* xj, double h, double* df) {
  double sq = 0.0;
#pragma unroll
  for (int d = 0; d < 6; ++d) { df[d] = xi[d] - xj[d]; sq += df[d] * df[d]; }
  return exp(-sq / h);
}

// ---- the Stein direction of one particle, three branches ---------------------------------------------------------------
// `tpp` lanes (a power of two <= 64, neighbours in the wavefront) share particle i: lane `part` takes j = part, part + tpp, …
// and the partial sums are folded by shuffles, in which EVERY lane of the wavefront takes part — act = false marks a lane
// without a particle.  phi is the direction in lane part == 0.  x, N, b: [P][6], H: [P][36] of all particles, wherever the
// shape keeps them: LDS in the one-workgroup kernels, the work arrays in direction_body.

// default SVN branch, svgd_grad preconditioned with the mean Hessian's inverse Hinv (SVNICP.cpp:218-227)
__device__ __forceinline__ void stein_direction_default(const double* x, const double* N, const double* Hinv, int P, double h,
                                                        const double* xi, bool act, int part, int tpp, double* phi) {
  double g[6] = {0, 0, 0, 0, 0, 0}, kn[6] = {0, 0, 0, 0, 0, 0}, ks = 0.0;
  if (act)
    for (int j = part; j < P; j += tpp) {
      double df[6];
      const double k = rbf_pair(xi, x + j * 6, h, df);
#pragma unroll
      for (int d = 0; d < 6; ++d) {
        g[d] += df[d] * k;
        kn[d] += k * (-N[j * 6 + d]);
      }
      ks += k;
    }
  for (int off = tpp >> 1; off > 0; off >>= 1) {
#pragma unroll
    for (int d = 0; d < 6; ++d) { g[d] += __shfl_xor(g[d], off, kWave); kn[d] += __shfl_xor(kn[d], off, kWave); }
    ks += __shfl_xor(ks, off, kWave);
  }
#pragma unroll
  for (int d = 0; d < 6; ++d) g[d] = 2 / h * g[d];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double hg = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) hg += Hinv[6 * r + c] * g[c];
    phi[r] = (kn[r] + hg) / ks;
  }
}

// full SVN branch, svn_full_grad (SVNICP.cpp:229-252)
__device__ __forceinline__ void stein_direction_full(const double* x, const double* b, const double* H, int P, double h, double lr,
                                                     const double* xi, bool act, int part, int tpp, double* phi) {
  double Hm[36], u[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 36; ++e) Hm[e] = 0.0;
  if (act)
    for (int j = part; j < P; j += tpp) {
      double df[6], g[6];
      const double k = rbf_pair(xi, x + j * 6, h, df);
#pragma unroll
      for (int d = 0; d < 6; ++d) g[d] = 2 / h * (df[d] * k);
      const double k2 = k * k;
      const double* Hj = H + (size_t)j * 36;
#pragma unroll
      for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = 0; c < 6; ++c) Hm[6 * r + c] += k2 * Hj[6 * r + c] + g[r] * g[c];
        u[r] += k * (-b[j * 6 + r]) + g[r];
      }
    }
  for (int off = tpp >> 1; off > 0; off >>= 1) {
#pragma unroll
    for (int e = 0; e < 36; ++e) Hm[e] += __shfl_xor(Hm[e], off, kWave);
#pragma unroll
    for (int r = 0; r < 6; ++r) u[r] += __shfl_xor(u[r], off, kWave);
  }
#pragma unroll
  for (int e = 0; e < 36; ++e) Hm[e] /= P;
#pragma unroll
  for (int r = 0; r < 6; ++r) u[r] /= P;
  int piv[6];
  const bool ok = lu6(Hm, piv);
  double out[6] = {0, 0, 0, 0, 0, 0};
  // inv(Hm)·u column by column (the reference forms the inverse, then multiplies)
  for (int c = 0; c < 6; ++c) {
    double col[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) col[r] = (r == c) ? 1.0 : 0.0;
    lu6_solve(Hm, piv, col);
#pragma unroll
    for (int r = 0; r < 6; ++r) out[r] += col[r] * u[c];
  }
#pragma unroll
  for (int r = 0; r < 6; ++r) phi[r] = ok ? lr * out[r] : __builtin_nan("");
}

// SVGD-ICP, svgd_grad (SVGDICP.cpp:457-474); G = the particles' sgd gradients
__device__ __forceinline__ void stein_direction_svgd(const double* x, const double* G, int P, double h,
                                                     const double* xi, bool act, int part, int tpp, double* phi) {
  double gr[6] = {0, 0, 0, 0, 0, 0}, kg[6] = {0, 0, 0, 0, 0, 0};
  if (act)
    for (int j = part; j < P; j += tpp) {
      double df[6];
      const double k = rbf_pair(xi, x + j * 6, h, df);
#pragma unroll
      for (int d = 0; d < 6; ++d) { gr[d] += df[d] * k; kg[d] += k * (-G[j * 6 + d]); }
    }
  for (int off = tpp >> 1; off > 0; off >>= 1) {
#pragma unroll
    for (int d = 0; d < 6; ++d) { gr[d] += __shfl_xor(gr[d], off, kWave); kg[d] += __shfl_xor(kg[d], off, kWave); }
  }
#pragma unroll
  for (int d = 0; d < 6; ++d) phi[d] = (kg[d] + 2 / h * gr[d]) / P;
}

// Stein direction (SVNICP.cpp:218-252), one wavefront per particle, then that particle's pose update.
// x and the Newton steps of all particles are read from the prepare kernel's arrays (L2 resident); R/t
// of particle pi are only touched by its own wavefront.  Its step norm goes to uctl[UCTL_NORM + pi].
__device__ __forceinline__ void direction_body(const UpdateArgs& a, int bx) {
  if (a.ctl[0]) return;
  constexpr int TPP = kWave;
  const int tid = threadIdx.x;
  const int P = a.P;
  Work w(a.work, P);
  const int pi = bx * (256 / TPP) + tid / TPP, part = tid % TPP;
  if (pi >= P) return;  // whole wavefront
  const double h = a.uctl[UCTL_H];
  double xi[6], phi[6];
#pragma unroll
  for (int d = 0; d < 6; ++d) xi[d] = w.x[pi * 6 + d];
  if (a.svgd) {  // + optimizer step and pose refresh of this particle (SVGDICP.cpp:476-494, :118-121)
    stein_direction_svgd(w.x, w.N, P, h, xi, true, part, TPP, phi);
    if (part == 0) {
#pragma unroll
      for (int d = 0; d < 6; ++d) w.phi[pi * 6 + d] = phi[d];
      a.uctl[UCTL_NORM + pi] = svgd_step_one(a, pi, phi, xi);
      if (!a.check_early_stop) {  // no stop decision pending: the history row (SVGDICP.cpp:133) can go out now
        double xn[6];
#pragma unroll
        for (int d = 0; d < 6; ++d) xn[d] = a.pose_out[d * P + pi];
        history_one(a, pi, xn);
      }
    }
    return;
  }
  if (!a.full_grad) stein_direction_default(w.x, w.N, a.uctl + UCTL_HINV, P, h, xi, true, part, TPP, phi);
  else stein_direction_full(w.x, w.b, w.H, P, h, a.lr, xi, true, part, TPP, phi);
  if (part == 0) {
#pragma unroll
    for (int r = 0; r < 6; ++r) w.phi[pi * 6 + r] = phi[r];
    const PoseStep st = pose_update(a, pi, phi);
    a.uctl[UCTL_NORM + pi] = st.norm;
    if (!a.check_early_stop) history_one(a, pi, st.x);   // no stop decision pending: the history row (SVNICP.cpp:103-107) can go out now
  }
}

// The one-workgroup kernels' early-stop decision (SVNICP.cpp:95-101; SVGDICP.cpp:123-131) on the threads' step norms — a
// shuffle fold per wavefront, then the T / 64 wave totals in order (sh_norm) — and the history row (SVNICP.cpp:103-107).
// Block-wide; true: the registration stops here, finish_iter_ = iteration + 1 and the stopping epoch's row stays zero.
template <int T>
__device__ __forceinline__ bool one_workgroup_finish(const UpdateArgs& a, double my_norm, double* sh_norm) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  bool stop = false;
  if (a.check_early_stop) {  // block-uniform
    for (int off = 32; off > 0; off >>= 1) my_norm += __shfl_xor(my_norm, off, kWave);
    if (lane == 0) sh_norm[wave] = my_norm;
    __syncthreads();
    double m = 0.0;
    for (int i = 0; i < T / kWave; ++i) m += sh_norm[i];
    m /= a.P;
    // torch::lt(f64 0-dim, f32 1-dim) promotes to float32 (SVNICP.cpp:42,96-97)
    stop = (float)m < (float)a.conv_thr;
  }
  if (stop) {
    if (tid == 0) { a.ctl[0] = 1; a.ctl[1] = a.iteration + 1; }
    return true;
  }
  __syncthreads();
  for (int e = tid; e < 6 * a.P; e += T) a.history[(size_t)a.iteration * 6 * a.P + e] = (float)a.pose_out[e];
  return false;
}

// the chain's early-stop decision on a fixed-order sum (SVNICP.cpp:95-101), traces, history (SVNICP.cpp:103-107)
__device__ __forceinline__ void finish_body(const UpdateArgs& a) {
  if (a.ctl[0]) return;
  const int tid = threadIdx.x;
  const int P = a.P;
  Work w(a.work, P);
  __shared__ double sh_part[256];
  __shared__ int sh_stop;
  if (a.trH) {
    if (!a.svgd) {
      for (int e = tid; e < P * 36; e += 256) a.trH[e] = w.H[e];
      for (int e = tid; e < P * 6; e += 256) a.trb[e] = w.b[e];
    }
    for (int e = tid; e < P * 6; e += 256) { a.trN[e] = w.N[e]; a.trphi[e] = w.phi[e]; }
    if (tid == 0) *a.trh = a.uctl[UCTL_H];
  }
  if (a.check_early_stop) {
    double s = 0.0;
    for (int p = tid; p < P; p += 256) s += a.uctl[UCTL_NORM + p];
    sh_part[tid] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {  // fixed tree: every replica decides alike
      if (tid < off) sh_part[tid] += sh_part[tid + off];
      __syncthreads();
    }
    if (tid == 0) {
      const double m = sh_part[0] / P;
      const int stop = (float)m < (float)a.conv_thr;
      if (stop) { a.ctl[0] = 1; a.ctl[1] = a.iteration + 1; }
      sh_stop = stop;
    }
    __syncthreads();
    if (sh_stop) return;
  } else {
    return;  // history already written by k_upd_direction
  }
  for (int e = tid; e < 6 * P; e += 256) a.history[(size_t)a.iteration * 6 * P + e] = (float)a.pose_out[e];
}

// ---------------------------------------------------------------------------------------------
// SVGD-ICP mode (first-order sibling): replaces the tail of SVGDICP::stein_align per iteration
// (src/core/SVGDICP.cpp:106-133): sgd_grad's finalisation (:398-455, Euler partials :335-396),
// svgd_grad + rbf_kernel (:457-474), pose_update through torch::optim (:476-494, options :142-170),
// the displacement early stop (:123-131) and the particle history (:133).
// Reference quirk kept: the RBF kernel is evaluated on pose_particles_ as it stood BEFORE this
// epoch's parameters were read, i.e. at epoch 0 on the previous registration's final particles.
// ---------------------------------------------------------------------------------------------
__device__ void euler_partials(const double* R0, double roll, double pitch, double yaw, double dR[3][9]) {
  const double A = cos(yaw), Bs = sin(yaw), C = cos(pitch), D = sin(pitch), E = cos(roll), F = sin(roll);
  const double DE = D * E, DF = D * F, AC = A * C, AF = A * F, AE = A * E;
  const double ADE = A * DE, ADF = A * DF, BC = Bs * C, BE = Bs * E, BF = Bs * F, BDE = Bs * DE;
  const double pr[9] = {0, ADE + BF, BE - ADF, 0, -AF + BDE, Bs * (-DF) - AE, 0, C * E, C * (-F)};
  const double pp[9] = {A * -D, AC * F, AC * E, Bs * -D, BC * F, BC * E, -C, -DF, -DE};
  const double py[9] = {-BC, -Bs * DF - AE, AF - BDE, AC, -BE + ADF, ADE + BF, 0, 0, 0};
  mat3_mul(R0, pr, dR[0]);
  mat3_mul(R0, pp, dR[1]);
  mat3_mul(R0, py, dR[2]);
}

// sgd_grad of one particle from the raw sums (SVGDICP.cpp:398-455): Euler-angle partials, (count + 1) normalisation,
// scaled by the source size
__device__ void svgd_gradient(const UpdateArgs& a, int p, double* g6) {
  double s[kNSums];
  load_sums(a, p, s);
  const double* eu = a.eul + 6 * p;
  double dR[3][9];
  euler_partials(a.pose.R0, eu[3], eu[4], eu[5], dR);
  const double cnt1 = s[4] + 1.0;  // nonzero_count + 1
  const double* R0 = a.pose.R0;
#pragma unroll
  for (int j = 0; j < 3; ++j)      // error.sum(1).matmul(R0) / (count + 1)
    g6[j] = ((s[10] * R0[j] + s[11] * R0[3 + j] + s[12] * R0[6 + j]) / cnt1) * a.n_src;
#pragma unroll
  for (int k = 0; k < 3; ++k) {    // Σ_b e·(dR_k s) = Σ_ij dR_k[i][j]·(Σ_b e_i s_j)
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) v += dR[k][3 * i + j] * s[13 + 3 * i + j];
    g6[3 + k] = (v / cnt1) * a.n_src;
  }
}

// optimizer step of one particle (param.grad = -stein_grad, SVGDICP.cpp:476-494 with torch's defaults, :142-170), next
// epoch's R_, t_, total pose (:88-91) and pose_particles_ (:118-121); returns |new pose - xold| for the early stop (:123-131)
__device__ double svgd_step_one(const UpdateArgs& a, int p, const double* phi6, const double* xold6) {
  const int P = a.P;
  const int step = a.iteration + 1;
  double n2 = 0.0, e6[6];
#pragma unroll
  for (int d = 0; d < 6; ++d) {
    const int i = p * 6 + d;
    double g = -phi6[d];
    double v = a.eul[i];
    double* m1 = a.opt + i; double* m2 = a.opt + (size_t)6 * P + i; double* m3 = a.opt + (size_t)12 * P + i;
    switch (a.optimizer) {
      case 0: {  // Adam: betas (0.9, 0.999), eps 1e-8
        const double b1 = 0.9, b2 = 0.999, eps = 1e-8;
        const double e1 = b1 * (*m1) + (1 - b1) * g;
        const double e2 = b2 * (*m2) + (1 - b2) * g * g;
        *m1 = e1; *m2 = e2;
        const double bc1 = 1 - pow(b1, (double)step), bc2 = 1 - pow(b2, (double)step);
        v -= (a.lr / bc1) * (e1 / (sqrt(e2) / sqrt(bc2) + eps));
      } break;
      case 1: {  // RMSprop: alpha .99, eps 1e-8, weight_decay 1e-8, momentum .9
        const double alpha = 0.99, eps = 1e-8, wd = 1e-8, mom = 0.9;
        g = g + wd * v;
        const double sq = alpha * (*m1) + (1 - alpha) * g * g;
        const double buf = mom * (*m2) + g / (sqrt(sq) + eps);
        *m1 = sq; *m2 = buf;
        v -= a.lr * buf;
      } break;
      case 2: v -= a.lr * g; break;  // SGD
      default: {  // Adagrad: eps 1e-10
        const double ss = (*m3) + g * g;
        *m3 = ss;
        v -= a.lr * (g / (sqrt(ss) + 1e-10));
      } break;
    }
    a.eul[i] = v;
    e6[d] = v;
    const double df = v - xold6[d];
    n2 += df * df;
  }
  // next epoch: R_ = Euler(rx,ry,rz), t_ = (x,y,z) (SVGDICP.cpp:88-91)
  double Rm[9], Rt[9], tt[3];
  euler_to_R(e6[3], e6[4], e6[5], Rm);
  mat3_mul(a.pose.R0, Rm, Rt);
  mat3_vec(a.pose.R0, e6, tt);
#pragma unroll
  for (int i = 0; i < 9; ++i) { a.R[9 * p + i] = Rm[i]; a.Rtot[12 * p + i] = Rt[i]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) { a.t[3 * p + i] = e6[i]; a.Rtot[12 * p + 9 + i] = a.pose.t0[i] + tt[i]; }
#pragma unroll
  for (int d = 0; d < 6; ++d) a.pose_out[d * P + p] = e6[d];   // pose_particles_ (SVGDICP.cpp:118-121)
  return sqrt(n2);
}

// ---- launch arithmetic shared by the launchers and the persistent kernel ----
// workgroups of the prepare part: one per PREP_PW particles, + the mean-Hessian workgroup (only the default SVN branch
// preconditions with the mean Hessian)
__host__ __device__ inline int prepare_blocks(const UpdateArgs& a) {
  return (a.P + PREP_PW - 1) / PREP_PW + ((!a.svgd && !a.full_grad) ? 1 : 0);
}
// workgroups of direction_body: one wavefront per particle, four per workgroup
__host__ __device__ inline int direction_blocks(int P) { return (P + 3) / 4; }
// dynamic LDS of median_body: x | the median bin's keys | the log-binned histogram
inline size_t median_lds_bytes(int P) {
  return (size_t)P * 6 * sizeof(double) + (size_t)(FRONT_BUF + 8) * sizeof(double) + (size_t)HB_NB * sizeof(unsigned int);
}

}  // namespace
}  // namespace svnicp
