// particle_update.hip — the kernels of the per-iteration Stein step on the particle set and their launchers.  The device
// pieces (H, b and the Newton step, the exact median, the three Stein directions, the pose update, the early-stop decision)
// are stated once in stein_step_device.hpp; this file holds the launch shapes that compose them:
//   k_particle_update / k_particle_update_svgd   the whole step in one workgroup out of LDS (option update=fused)
//   k_upd_prepare[_median], k_upd_direction, k_upd_finish   the default chain (api.hip sequences it)
//   k_upd_median, or k_upd_hist -> k_upd_collect -> k_upd_select above 128 particles   the pair statistics on their own
// In the multi-GPU layout every GPU runs these kernels redundantly on ALL particles after the all-gather of the 22 raw sums
// per particle; identical inputs + identical code ⇒ identical state.
#include "kernels.hpp"
#include "stein_step_device.hpp"

namespace svnicp {

namespace {

// threads cooperating on one particle in the Stein-direction phase (power of two, <= 64)
__device__ __forceinline__ int threads_per_particle(int P) {
  int tpp = 1;
  while (tpp < 64 && tpp * 2 * P <= UT) tpp <<= 1;
  return tpp;
}

__global__ __launch_bounds__(UT) void k_particle_update(UpdateArgs a) {
  if (a.ctl[0]) return;
  extern __shared__ __align__(16) double dyn[];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid >> 6;
  const int P = a.P;
  Work w(a.work, P);
  double* lx = dyn;               // [P][6]  x = [t ; Log R]
  double* lN = lx + 6 * P;        // [P][6]  Newton step
  double* lb = lN + 6 * P;        // [P][6]  b
  double* lphi = lb + 6 * P;      // [P][6]  Stein direction
  const double* Hsrc = a.h_in_lds ? (lphi + 6 * P) : w.H;  // [P][36]
  double* lH = a.h_in_lds ? (lphi + 6 * P) : nullptr;
  __shared__ SelShared sel;
  __shared__ double sh_Hinv[36];
  __shared__ double sh_Hmean[36];
  __shared__ double sh_norm[UT / kWave];

  PhaseStamp stamp(a.dbg, tid == 0);
  // ---- 1. per particle: H, b, Newton step, x = [t ; Log R] ----
  for (int p = tid; p < P; p += UT) {
    double H[36], b[6], N[6];
    particle_Hb(a, p, H, b);
    if (lH) {
#pragma unroll
      for (int i = 0; i < 36; ++i) lH[p * 36 + i] = H[i];
    }
    if (!lH || a.trH) {
#pragma unroll
      for (int i = 0; i < 36; ++i) w.H[(size_t)p * 36 + i] = H[i];
    }
    newton_step(H, b, N);
#pragma unroll
    for (int i = 0; i < 6; ++i) { lb[p * 6 + i] = b[i]; lN[p * 6 + i] = N[i]; }
    double lg[3];
    so3_log(a.R + 9 * p, lg);                                 // SVNICP.cpp:74-77
#pragma unroll
    for (int i = 0; i < 3; ++i) { lx[p * 6 + i] = a.t[3 * p + i]; lx[p * 6 + 3 + i] = lg[i]; }
  }
  sel_init(&sel, lower_median_rank(P), 0ull, tid);
  __syncthreads();
  stamp(0);

  if (P > 1) {
    // ---- 2. mean Hessian (SVNICP.cpp:85) and its inverse, RBF bandwidth from the exact median ----
    if (!a.full_grad && tid < 36 * 8) {  // 8 lanes per entry, strided over particles, folded by shuffles
      const int e = tid >> 3, part = tid & 7;
      double s = 0.0;
      for (int p = part; p < P; p += 8) s += Hsrc[(size_t)p * 36 + e];
#pragma unroll
      for (int off = 4; off > 0; off >>= 1) s += __shfl_xor(s, off, 8);
      if (part == 0) sh_Hmean[e] = s / P;
    }
    __syncthreads();
    if (!a.full_grad && wave == UT / kWave - 1 && lane < 6) inverse_column(sh_Hmean, lane, sh_Hinv);   // one column per lane
    rbf_bandwidth<UT>(lx, P, w.sq, &sel, tid, lane, wave);
    stamp(1);
    const double h = sel.h;
    // ---- 3. Stein direction: tpp threads per particle split the sum over j; the pair distance is recomputed from LDS
    //         (bit-identical, cheaper than an HBM load) ----
    const int tpp = threads_per_particle(P);
    const int per_pass = UT / tpp;
    for (int base = 0; base < P; base += per_pass) {
      const int pi = base + tid / tpp, part = tid % tpp;
      const bool act = pi < P;
      double xi[6], phi[6];
#pragma unroll
      for (int d = 0; d < 6; ++d) xi[d] = act ? lx[pi * 6 + d] : 0.0;
      if (!a.full_grad) stein_direction_default(lx, lN, sh_Hinv, P, h, xi, act, part, tpp, phi);
      else stein_direction_full(lx, lb, Hsrc, P, h, a.lr, xi, act, part, tpp, phi);
      if (act && part == 0) {
#pragma unroll
        for (int r = 0; r < 6; ++r) lphi[pi * 6 + r] = phi[r];
      }
    }
  } else {
    if (tid == 0)
      for (int d = 0; d < 6; ++d) lphi[d] = -lN[d];           // SVNICP.cpp:89
  }
  __syncthreads();

  stamp(2);
  // ---- 4. traces (tests only) ----
  if (a.trH) {
    for (int e = tid; e < P * 36; e += UT) a.trH[e] = w.H[e];
    for (int e = tid; e < P * 6; e += UT) { a.trb[e] = lb[e]; a.trN[e] = lN[e]; a.trphi[e] = lphi[e]; }
    if (tid == 0) *a.trh = sel.h;
  }

  // ---- 5. pose update (SVNICP.cpp:268-279) + early stop statistic ----
  double my_norm = 0.0;
  for (int p = tid; p < P; p += UT) {
    double phi[6];
#pragma unroll
    for (int d = 0; d < 6; ++d) phi[d] = lphi[p * 6 + d];
    my_norm += pose_update(a, p, phi).norm;
  }
  stamp(3);
  if (one_workgroup_finish<UT>(a, my_norm, sh_norm)) return;
  stamp(4);
}

__global__ __launch_bounds__(PREP_T) void k_upd_prepare(UpdateArgs a) { prepare_body(a, (int)blockIdx.x); }

// pass 1 over all pairs: log-binned histogram (LDS per workgroup, merged with global atomics); the bin of the
// lower median is found at the start of k_upd_collect (a last-workgroup scan here cost 30 us of serial tail)
__global__ __launch_bounds__(256) void k_upd_hist(UpdateArgs a) {
  if (a.ctl[0]) return;
  extern __shared__ __align__(16) double dyn[];
  const int tid = threadIdx.x;
  const int P = a.P;
  Work w(a.work, P);
  double* lx = dyn;
  unsigned int* lh = reinterpret_cast<unsigned int*>(dyn + 6 * P);
  // x = pose_particles_ = [t ; Log R] as the last pose update left it (SVNICP.cpp:74-77,103-106; SVGD-ICP: as it stands,
  // SVGDICP.cpp:106-110) — this chain runs beside the stage-B kernels and must not depend on anything they produce
  for (int e = tid; e < 6 * P; e += 256) {
    const int pp = e / 6, d = e - 6 * pp;
    const double v = a.pose_out[d * P + pp];
    lx[e] = v;
    if (blockIdx.x == 0) w.x[e] = v;   // k_upd_direction reads x from here
  }
  for (int e = tid; e < HB_NB; e += 256) lh[e] = 0u;
  __syncthreads();
  unsigned long long* u = reinterpret_cast<unsigned long long*>(a.uctl);
  unsigned int* gh = upd_hist(a.uctl, P);
  const int n = P * P;
  bool nan = false;
  {
    const int stride = gridDim.x * 256;              // pair index advance per step: (di, dj) without a division per pair
    const int di = stride / P, dj = stride - di * P;
    int e = blockIdx.x * 256 + tid;
    int i = e / P, j = e - i * P;
    for (; e < n; e += stride) {
      const double s = pair_sq(lx, i, j);
      if (s != s) nan = true;
      atomicAdd(&lh[key_bin((unsigned long long)__double_as_longlong(s))], 1u);
      j += dj; i += di;
      if (j >= P) { j -= P; ++i; }
    }
  }
  if (nan) u[UCTL_NAN] = 1ull;
  __syncthreads();
  for (int e = tid; e < HB_NB; e += 256) {
    const unsigned int c = lh[e];
    if (c) atomicAdd(&gh[e], c);
  }
}

// pass 2 over all pairs: the keys of the median's bin go to work.sq (LDS staging, one global atomic per workgroup)
__global__ __launch_bounds__(256) void k_upd_collect(UpdateArgs a) {
  if (a.ctl[0]) return;
  extern __shared__ __align__(16) double dyn[];
  __shared__ unsigned int sh_cnt, sh_wsum[4];
  __shared__ int sh_bin;
  __shared__ unsigned long long sh_base;
  const int tid = threadIdx.x;
  const int P = a.P;
  Work w(a.work, P);
  double* lx = dyn;
  double* lbuf = dyn + 6 * P;  // [COLL_CHUNK]: matches of one chunk of pairs
  for (int e = tid; e < 6 * P; e += 256) { const int pp = e / 6, d = e - 6 * pp; lx[e] = a.pose_out[d * P + pp]; }
  if (tid == 0) sh_cnt = 0u;
  unsigned long long* u = reinterpret_cast<unsigned long long*>(a.uctl);
  const int n = P * P;
  // bin of the lower median: every workgroup scans the finished global histogram itself (48 plain loads per thread, L2
  // resident); workgroup 0 publishes bin and rank for k_upd_select
  bin_of_rank<256>(upd_hist(a.uctl, P), (unsigned int)((n - 1) / 2), sh_wsum, [&](int bin, unsigned int inside) {
    sh_bin = bin;
    if (blockIdx.x == 0) { u[UCTL_BIN] = (unsigned long long)bin; u[UCTL_RANK] = inside; }
  });
  __syncthreads();
  const int bstar = sh_bin;
  // the workgroup's pairs in chunks of COLL_CHUNK: a chunk cannot overflow the LDS buffer, and each chunk with
  // matches costs one global atomic
  for (int c0 = blockIdx.x * COLL_CHUNK; c0 < n; c0 += gridDim.x * COLL_CHUNK) {
    const int c1 = (c0 + COLL_CHUNK < n) ? c0 + COLL_CHUNK : n;
    {
      const int di = 256 / P, dj = 256 - di * P;
      int e = c0 + tid;
      int i = e / P, j = e - i * P;
      for (; e < c1; e += 256) {
        const double s = pair_sq(lx, i, j);
        if (key_bin((unsigned long long)__double_as_longlong(s)) == bstar) lbuf[atomicAdd(&sh_cnt, 1u)] = s;
        j += dj; i += di;
        if (j >= P) { j -= P; ++i; }
      }
    }
    __syncthreads();
    const unsigned int cnt = sh_cnt;
    if (cnt) {  // block-uniform
      if (tid == 0) sh_base = atomicAdd(&u[UCTL_CNT], (unsigned long long)cnt);
      __syncthreads();
      const unsigned long long base = sh_base;
      for (unsigned int e = tid; e < cnt; e += 256) w.sq[base + e] = lbuf[e];
      __syncthreads();
      if (tid == 0) sh_cnt = 0u;
      __syncthreads();
    }
  }
}

// exact median inside its bin -> h
__global__ __launch_bounds__(UT) void k_upd_select(UpdateArgs a) {
  if (a.ctl[0]) return;
  extern __shared__ __align__(16) double dyn[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = a.P;
  Work w(a.work, P);
  __shared__ SelShared sel;
  const unsigned long long* u = reinterpret_cast<const unsigned long long*>(a.uctl);
  const int m = (int)u[UCTL_CNT];
  const unsigned int r = (unsigned int)u[UCTL_RANK];
  const int bstar = (int)u[UCTL_BIN];
  // interior bins share the top 20 key bits: passes 7 and 6 are known
  const bool interior = bstar > 0 && bstar < HB_NB - 1;
  const unsigned long long top20 = (unsigned long long)bstar + ((unsigned long long)HB_EXP0 << 8);
  const int first_pass = interior ? 5 : 7;
  const unsigned long long prefix0 = interior ? (top20 >> 4) : 0ull;
  const bool in_lds = m <= SEL_LDS_KEYS;   // else a degenerate distribution (most pairs in one bin): the same select on the global buffer
  if (in_lds) {
    for (int e = tid; e < m; e += UT) dyn[e] = w.sq[e];
    __syncthreads();
  }
  sel_init(&sel, r, prefix0, tid);
  __syncthreads();
  const unsigned long long kmed =
      in_lds ? block_select([&](auto count) { for (int e = tid; e < m; e += UT) count((unsigned long long)__double_as_longlong(dyn[e])); },
                            first_pass, &sel, lane, wave)
             : block_select([&](auto count) { for (int e = tid; e < m; e += UT) count((unsigned long long)__double_as_longlong(w.sq[e])); },
                            first_pass, &sel, lane, wave);
  if (tid == 0) {
    const double med = u[UCTL_NAN] ? __builtin_nan("") : __longlong_as_double((long long)kmed);
    a.uctl[UCTL_H] = med / log((double)(P + 1));              // SVNICP.cpp:262
  }
  // leave the chain's global state as the next iteration's k_upd_hist expects it (svnicp_align_begin zeroes it once)
  __syncthreads();
  unsigned int* gh = upd_hist(a.uctl, P);
  for (int e = tid; e < HB_NB; e += UT) gh[e] = 0u;
  if (tid == 0) {
    unsigned long long* uw = reinterpret_cast<unsigned long long*>(a.uctl);
    uw[UCTL_NAN] = 0ull; uw[UCTL_CNT] = 0ull;
  }
}

__global__ __launch_bounds__(UT) void k_upd_median(UpdateArgs a) { median_body<UT>(a); }

// Small registrations: both halves of the Stein step's front in ONE launch on the main stream — the last workgroup runs the
// pair statistics, the others the sums-dependent half.  At the scan-to-map loop's sizes every kernel of an iteration runs
// at its launch latency, and the second stream's fork and join cost 6-8 us each: k_reduce_partials (the prepare lanes add
// the workgroups' records themselves, load_sums), k_upd_median's own launch and both event waits fall away.
__global__ __launch_bounds__(UT) void k_upd_prepare_median(UpdateArgs a) {
  if (blockIdx.x + 1 == gridDim.x) median_body<UT>(a);
  else prepare_body(a, (int)blockIdx.x);
}

__global__ __launch_bounds__(256) void k_upd_direction(UpdateArgs a) { direction_body(a, (int)blockIdx.x); }
__global__ __launch_bounds__(256) void k_upd_finish(UpdateArgs a) { finish_body(a); }

__global__ __launch_bounds__(UT) void k_particle_update_svgd(UpdateArgs a) {
  if (a.ctl[0]) return;
  extern __shared__ __align__(16) double dyn[];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid >> 6;
  const int P = a.P;
  Work w(a.work, P);
  double* lx = dyn;             // [P][6] pose_particles_ before this epoch's step
  double* lg = lx + 6 * P;      // [P][6] sgd gradient
  double* lphi = lg + 6 * P;    // [P][6] stein gradient
  __shared__ SelShared sel;
  __shared__ double sh_norm[UT / kWave];

  // ---- 1. sgd_grad from the raw sums (SVGDICP.cpp:398-455) ----
  for (int p = tid; p < P; p += UT) {
    svgd_gradient(a, p, lg + p * 6);
#pragma unroll
    for (int d = 0; d < 6; ++d) lx[p * 6 + d] = a.pose_out[d * P + p];
  }
  sel_init(&sel, lower_median_rank(P), 0ull, tid);
  __syncthreads();

  // ---- 2. svgd_grad (SVGDICP.cpp:457-474) ----
  if (P > 1) {
    rbf_bandwidth<UT>(lx, P, w.sq, &sel, tid, lane, wave);
    const double h = sel.h;
    const int tpp = threads_per_particle(P);
    const int per_pass = UT / tpp;
    for (int base = 0; base < P; base += per_pass) {
      const int pi = base + tid / tpp, part = tid % tpp;
      const bool act = pi < P;
      double xi[6], phi[6];
#pragma unroll
      for (int d = 0; d < 6; ++d) xi[d] = act ? lx[pi * 6 + d] : 0.0;
      stein_direction_svgd(lx, lg, P, h, xi, act, part, tpp, phi);
      if (act && part == 0) {
#pragma unroll
        for (int d = 0; d < 6; ++d) lphi[pi * 6 + d] = phi[d];
      }
    }
  } else {
    if (tid == 0)
      for (int d = 0; d < 6; ++d) lphi[d] = -lg[d];          // SVGDICP.cpp:112
  }
  __syncthreads();

  if (a.trN) {  // traces (tests only): newton slot carries the sgd gradient
    for (int e = tid; e < P * 6; e += UT) { a.trN[e] = lg[e]; a.trphi[e] = lphi[e]; }
    if (tid == 0) *a.trh = sel.h;
  }

  // ---- 3. optimizer step (param.grad = -stein_grad, SVGDICP.cpp:476-494), pose refresh, early stop (finish_iter_ = epoch + 1, :128) ----
  double my_norm = 0.0;
  for (int p = tid; p < P; p += UT) my_norm += svgd_step_one(a, p, lphi + p * 6, lx + p * 6);
  one_workgroup_finish<UT>(a, my_norm, sh_norm);
}

}  // namespace

size_t update_workspace_doubles(int P) { return (size_t)P * (36 + 6 * 4) + (size_t)P * P + 64; }
size_t update_uctl_doubles(int P) { return (size_t)UCTL_NORM + (size_t)((P + 7) & ~7) + (size_t)HB_NB / 2 + (size_t)36 * ((P + 127) / 128) + 8; }

// ---- the Stein step of 2 <= P particles as three pieces (api.hip sequences them) --------------------------------------
//   launch_update_median     pair statistics -> bandwidth h: needs the poses only; on the context's SECOND stream, beside the
//                            stage-B kernels of the same iteration
//   launch_update_prepare    H, b, Newton step, mean-Hessian inverse: needs the sums only
//   launch_update_direction  Stein direction + pose update per particle [+ k_upd_finish: early stop, traces, history]
hipError_t launch_update_median(const UpdateArgs& a, int num_cus, int max_p_one_workgroup, hipStream_t st) {
  const int P = a.P;
  if (P <= max_p_one_workgroup && P <= 128) {   // one workgroup, keys in registers (KREG)
    const size_t smem = median_lds_bytes(P);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_upd_median), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_upd_median, dim3(1), dim3(UT), smem, st, a);
    return hipGetLastError();
  }
  const size_t n = (size_t)P * P;
  const size_t xs = (size_t)P * 6 * sizeof(double);
  // few, fat workgroups: each one merges its LDS histogram into the global one with atomics, and those contend
  int nb = (int)((n + 1023) / 1024);
  if (nb > num_cus / 2) nb = num_cus / 2;
  if (nb < 1) nb = 1;
  const size_t lds_hist = xs + (size_t)HB_NB * sizeof(unsigned int);
  const size_t lds_coll = xs + (size_t)COLL_CHUNK * sizeof(double);
  const size_t lds_sel = (size_t)SEL_LDS_KEYS * sizeof(double);
  if (lds_hist > 150 * 1024 || lds_coll > 150 * 1024) return hipErrorInvalidValue;  // P > ~2000 on a 256-CU part
  {  // raise the dynamic-LDS cap (per device; a cheap host-side call)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_upd_hist), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_upd_collect), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_upd_select), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_sel);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_upd_hist, dim3(nb), dim3(256), lds_hist, st, a);
  hipLaunchKernelGGL(k_upd_collect, dim3(nb), dim3(256), lds_coll, st, a);
  hipLaunchKernelGGL(k_upd_select, dim3(1), dim3(UT), lds_sel, st, a);
  return hipGetLastError();
}

hipError_t launch_update_prepare(const UpdateArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_upd_prepare, dim3(prepare_blocks(a)), dim3(PREP_T), 0, st, a);
  return hipGetLastError();
}

// 2 <= P <= 128 only (the one-workgroup pair statistics)
hipError_t launch_update_prepare_median(const UpdateArgs& a, hipStream_t st) {
  const size_t smem = median_lds_bytes(a.P);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_upd_prepare_median), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_upd_prepare_median, dim3(prepare_blocks(a) + 1), dim3(UT), smem, st, a);
  return hipGetLastError();
}

hipError_t launch_update_direction(const UpdateArgs& a, hipStream_t st, bool finish) {
  hipLaunchKernelGGL(k_upd_direction, dim3(direction_blocks(a.P)), dim3(256), 0, st, a);
  if (finish && (a.check_early_stop || a.trH)) hipLaunchKernelGGL(k_upd_finish, dim3(1), dim3(256), 0, st, a);
  return hipGetLastError();
}
const double* update_step_norms(const UpdateArgs& a) { return a.uctl + UCTL_NORM; }

hipError_t launch_update(const UpdateArgs& a_in, hipStream_t st) {
  UpdateArgs a = a_in;
  const size_t base = (size_t)a.P * 24 * sizeof(double);           // x, N, b, phi
  const size_t with_h = base + (size_t)a.P * 36 * sizeof(double);  // + H
  a.h_in_lds = with_h <= 120 * 1024 ? 1 : 0;
  const size_t smem = a.h_in_lds ? with_h : base;
  if (smem > 150 * 1024) return hipErrorInvalidValue;  // P > 800: not supported by the one-workgroup update
  if (smem > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_particle_update),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_particle_update, dim3(1), dim3(UT), smem, st, a);
  return hipGetLastError();
}

hipError_t launch_update_svgd(const UpdateArgs& a, hipStream_t st) {
  const size_t smem = (size_t)a.P * 18 * sizeof(double);
  if (smem > 150 * 1024) return hipErrorInvalidValue;
  if (smem > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_particle_update_svgd),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_particle_update_svgd, dim3(1), dim3(UT), smem, st, a);
  return hipGetLastError();
}

}  // namespace svnicp
