// small_registration.hip — all iterations of a small registration in ONE cooperative launch (option chain=persistent): the
// stage-B bodies of stein_split_device.hpp and the Stein-step bodies of stein_step_device.hpp on virtual blocks, a grid
// barrier between the phases.
#include "kernels.hpp"
#include "stein_step_device.hpp"
#include "stein_split_device.hpp"

namespace svnicp {

namespace {

// ---------------------------------------------------------------------------------------------
// Small registrations, all iterations in ONE launch (svnicp_align of a context that qualifies for the small chain).
// At the scan-to-map loop's sizes an iteration is four dependent launches of 10-16 us each for a few microseconds of work
// (DESIGN.md §4.3).  k_small_registration keeps a few dozen workgroups resident for the whole registration (cooperative
// launch: the runtime refuses the grid unless every workgroup is resident at once) and runs the very same device bodies
// on virtual blocks, phase by phase, with a grid barrier between the phases:
//   A1 workgroups 0 … GS-1: search, each over its own slice of the source points;  workgroup GS: the pair statistics (it
//      only registers at the next barrier and works on through A2)
//   A2 workgroups 0 … GA-1: accumulate (the four-launch chain's partition: at most 32 records per particle)
//   B  per particle group: the workgroups' partial records added in block order, H, b, Newton step; mean Hessian + inverse
//   C  one wavefront per particle: Stein direction + pose update   [D  workgroup 0: early-stop decision, history, traces]
// The barrier is an arrival counter (four, used in turn) and a generation word in global memory: the last workgroup to
// arrive resets the counter and bumps the generation, the others poll it with s_sleep — and give up after a bounded number of polls (about a
// second), set the error word and leave, so that no wave can wait forever whatever happens to a sibling; the host then
// reports SVNICP_ERR_HIP instead of a result.  Every wave passes __threadfence() on both sides of a barrier (release of its
// own writes, invalidation of its L1 before it reads the others').  Same arithmetic, same block partition and the same
// order of additions as the four-launch small chain: bit-identical results (test_small_registration_persistent_kernel).
struct SmallArgs {
  int GS;                 // workgroups of the search phase; workgroup GS runs the pair statistics
  int GA;                 // workgroups of the accumulate phase (= records per particle in `partial`)
  int spts_per_block;     // source points per search workgroup
  int iterations;
  unsigned int* bar;      // [0] generation, [1] error word, [4 + k] arrivals of barrier k mod 4 (all zero at launch)
};

// arrive at barrier `k` (the k-th of this launch); wait = false: arrival only (the caller has nothing the others need before
// the NEXT barrier and goes on working — it still releases the barrier if it happens to be the last to arrive)
__device__ __forceinline__ bool grid_barrier(const SmallArgs& s, unsigned int& k, int nblocks, bool wait = true) {
  __shared__ int sh_ok;
  // The fences are agent-scope: on this part every XCD has its own L2, so a release writes the XCD's dirty lines back and
  // an acquire invalidates — once per WORKGROUP (thread 0, between two workgroup barriers that order the other waves'
  // accesses against it), not once per thread: 256 threads fencing on both sides cost 20 us per barrier.
  __syncthreads();
  if (threadIdx.x == 0) {
    int ok = 1;
    __threadfence();                     // release: the workgroup's writes are device-visible before the arrival
    volatile unsigned int* vb = s.bar;
    unsigned int* cnt = s.bar + 4 + (k & 3u);
    if (atomicAdd(cnt, 1u) == (unsigned int)nblocks - 1u) {
      *cnt = 0u;                         // (barrier k + 4 cannot begin before barrier k + 3 has ended, i.e. long after this)
      __threadfence();
      atomicAdd(&s.bar[0], 1u);
    } else if (wait) {
      unsigned int polls = 0u;
      while ((int)(vb[0] - (k + 1u)) < 0) {   // generation k + 1 = barrier k released
        __builtin_amdgcn_s_sleep(4);
        if (++polls > (1u << 22) || vb[1] != 0u) { atomicExch(&s.bar[1], 1u); ok = 0; break; }   // bounded: nobody waits forever
      }
    }
    __threadfence();                     // acquire: no stale line is read after the barrier
    sh_ok = ok;
  }
  __syncthreads();
  ++k;
  return sh_ok != 0;
}

template <int PW, int WP, int NRB, bool TAIL, bool SVGD>
__global__ __launch_bounds__(256) void k_small_registration(AccumArgs a, UpdateArgs u, SmallArgs s) {
  extern __shared__ __align__(16) double dyn[];
  const int bx = (int)blockIdx.x, nblocks = (int)gridDim.x;
  const int P = u.P;
  const int n_prep = prepare_blocks(u), n_dir = direction_blocks(P);
  const bool want_finish = u.check_early_stop != 0;   // (no traces here: a context that records traces runs the four-launch chain)
  UpdateArgs ub = u;                     // phase B reads the accumulate workgroups' records themselves
  ub.sums = a.partial; ub.n_ranks = s.GA; ub.sums_stride = a.Ppad * kNSums;
  AccumArgs as = a;                      // the search phase has its own, finer slices of the source points
  as.spts_per_block = s.spts_per_block;
  unsigned int k = 0u;
  PhaseStamp stamp(u.dbg, bx == 0 && threadIdx.x == 0);   // option debug: workgroup 0's cycles per phase (barrier included), summed over the iterations
  for (int it = 0; it < s.iterations; ++it) {
    if (a.ctl[0]) break;                 // early stop (uniform: read behind the last barrier's acquire)
    u.iteration = it; ub.iteration = it;
    // ---- phase A1: search on GS workgroups; workgroup GS starts the pair statistics and only REGISTERS at the barrier
    if (bx < s.GS) search_body<PW, WP, NRB, TAIL>(as, bx, 0);
    stamp(0);
    if (bx == s.GS) {
      if (!grid_barrier(s, k, nblocks, false)) return;
      median_body<256>(u);
    } else {
      if (!grid_barrier(s, k, nblocks)) return;
      stamp(1);
      // ---- phase A2: accumulate on GA workgroups
      if (bx < s.GA) accumulate_body<PW, WP, true, SVGD>(a, bx, 0, dyn);
      stamp(2);
    }
    if (!grid_barrier(s, k, nblocks)) return;
    stamp(3);
    // ---- phase B
    if (bx < n_prep) prepare_body(ub, bx);
    stamp(4);
    if (!grid_barrier(s, k, nblocks)) return;
    stamp(5);
    // ---- phase C
    if (bx < n_dir) direction_body(u, bx);
    stamp(6);
    if (!grid_barrier(s, k, nblocks)) return;
    stamp(7);
    if (want_finish) {
      if (bx == 0) finish_body(u);
      if (!grid_barrier(s, k, nblocks)) return;
    }
  }
}

}  // namespace

// ---- the persistent small-registration kernel: host side ----
namespace {
template <int PW, int WP, int NRB, bool TAIL>
hipError_t launch_small_t(const AccumArgs& a, const UpdateArgs& u, const SmallArgs& s, int grid, size_t smem, hipStream_t st) {
  const void* fn = u.svgd ? reinterpret_cast<const void*>(k_small_registration<PW, WP, NRB, TAIL, true>)
                          : reinterpret_cast<const void*>(k_small_registration<PW, WP, NRB, TAIL, false>);
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  int per_cu = 0;
  e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, smem);
  if (e != hipSuccess) return e;
  if (per_cu < 1) return hipErrorCooperativeLaunchTooLarge;
  AccumArgs aa = a; UpdateArgs uu = u; SmallArgs ss = s;
  void* args[3] = {&aa, &uu, &ss};
  return hipLaunchCooperativeKernel(fn, dim3((unsigned)grid), dim3(256), args, (unsigned int)smem, st);
}
}  // namespace

// all iterations of a small registration in one cooperative launch; `bar`: three zeroed words (arrivals, generation, error)
hipError_t launch_small_registration(const AccumPlan& plan, AccumArgs a, const UpdateArgs& u, int iterations, unsigned int* bar,
                                     int num_cus, hipStream_t st) {
  const int P = u.P;
  a.Ppad = plan.Ppad; a.pts_per_block = plan.pts_per_block; a.spts_per_block = plan.pts_per_block;   // one slice of points per workgroup, both bodies
  SmallArgs s{};
  s.GA = plan.grid_x; s.iterations = iterations; s.bar = bar;
  {  // search slices: one pass of the four waves per workgroup at least, at most num_cus - 1 workgroups
    const int pass = 4 * (64 / plan.PW);
    int64_t spb = (a.B + (num_cus - 2)) / (num_cus - 1);
    spb = (spb + pass - 1) / pass * pass;
    s.spts_per_block = (int)spb;
    s.GS = (int)((a.B + spb - 1) / spb);
  }
  if (!search_offsets_fit(a.Ppad, a.K)) return hipErrorInvalidValue;   // search_limits.hpp
  const int n_prep = prepare_blocks(u), n_dir = direction_blocks(P);
  int grid = s.GS + 1;
  if (s.GA > grid) grid = s.GA;
  if (n_prep > grid) grid = n_prep;
  if (n_dir > grid) grid = n_dir;
  if (grid > num_cus) return hipErrorCooperativeLaunchTooLarge;
  const size_t smem_median = median_lds_bytes(P);
  const size_t smem = smem_median > plan.smem ? smem_median : plan.smem;
  // small_registration_supported (registration_plan.hpp) names exactly the (PW, WP) instantiated below; NRB = 6 search row
  // blocks cover its 97 <= knn_count <= 100
  if (!small_registration_supported(plan.PW, plan.WP, plan.K)) return hipErrorInvalidValue;
  if (plan.PW == 16) return launch_small_t<16, 1, 6, true>(a, u, s, grid, smem, st);
  if (plan.PW == 32) return launch_small_t<32, 1, 6, true>(a, u, s, grid, smem, st);
  if (plan.WP == 1) return launch_small_t<64, 1, 6, true>(a, u, s, grid, smem, st);
  return launch_small_t<64, 2, 6, true>(a, u, s, grid, smem, st);
}

}  // namespace svnicp
