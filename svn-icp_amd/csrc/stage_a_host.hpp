// stage_a_host.hpp — host-only: stage A (the exact top-K search) as svnicp_ctx holds it.  The rules are in
// stage_a_plan.hpp; here are the working set, ONE sizing of it per registration, the target layout build, the dispatch
// to the four kernel families and what the getters read.  Every function reports through the owning object's error
// path (HIPCHK / fail of device_buffer.hpp), which is why they are templates on that object.
#pragma once
#include <algorithm>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "device_buffer.hpp"
#include "kernels.hpp"

namespace svnicp_host {
using namespace svnicp;

// what stage A reads of the context that owns it
struct StageAEnv {
  hipStream_t stream;
  const Tuning& tune;
  int num_cus;
  bool record_trace;
  const double* tgt;   // [M][3] as given
  int64_t B, M;        // source rows (not the query rows of a search), target rows
  const Pose0& pose0;
};

// where the select kernel of the tile family writes the split stage B's search table (registration_plan.hpp: select_writes_table)
struct TableOut { float4* rows; double* anchor; float* cmax; };

struct StageA {
  StageAPlan plan;   // of the registration begun last (begin)
  bool writes_table = false;   // … and select_writes_table of it: its whole-range search writes the search table and stores no distances
  // target SoA copies in the order plan.layout names; `held` is what they hold now (None: nothing, build at the next begin)
  TargetLayout held = TargetLayout::None;
  // registration_plan.hpp: joint_morton_sort — begin() has left the Morton layout to the registration's own search, which
  // sorts target and queries in one pass; any other search that comes first builds it on its own (ensure_layout)
  bool layout_pending = false;
  // the launch that begins the registration (k_init_particles) has put bbox, emax and fail_count at their start values for
  // the pending joint search, which then fills none of them; any search or layout build consumes the promise
  bool start_words_set = false;
  DevBuf<double> tx, ty, tz;
  DevBuf<float> txf, tyf, tzf, tile_box;
  DevBuf<float4> tile_a, tile_o;         // Morton layout: tile-local rows in MFMA A-operand order, origin | C_t per tile (knn_prefilter = mfma)
  DevBuf<int32_t> torig;
  DevBuf<unsigned long long> emax, bbox;
  DevBuf<double> cand_d2;                // the result: [rows][K], ascending by (d², index)
  DevBuf<int32_t> cand_idx;
  DevBuf<double> pool_d, sl_d, fail_tau, qrec;   // streaming kernel's pools, sliced fallback lists, proven thresholds, per-query records
  DevBuf<int32_t> pool_i, sl_i, pool2, fail_list, stat_n;
  DevBuf<int> fail_count;
  // a later search of the registration's working set (correspondence = full: one per particle and iteration; svnicp_evaluate)
  // reuses fail_list / fail_count: stage A's own are kept here, and `stage_kept` says that the getters read them
  DevBuf<int> stage_fail_count;
  DevBuf<int32_t> stage_fail_list;
  bool stage_kept = false;
  DevBuf<unsigned int> keys_a, keys_b;   // Morton sort scratch, for max(M, B) keys
  DevBuf<int32_t> vals_a, order_t, qorder;
  DevBuf<unsigned char> sort_tmp;
  size_t sort_n = 0, sort_tmp_bytes = 0;
  int sort_bits = 0;
  DevBuf<int32_t> arena, chunk_tab;      // tile kernels: overflow chunks of the survivor pools and their table
  DevBuf<unsigned long long> dbg_phase;  // option debug: per-phase wave cycles of k_knn_tiles / k_knn_brute
  static constexpr size_t kDbgPhaseWaves = 65536;   // per-wave records dbg_phase has room for, behind its 8 totals

  // Start of a registration: choose the kernel for `rows` query rows and K, size ALL scratch for it — every search of this
  // registration included, whose neighbour counts are Ks (K itself, normal_k of a normal pass, 1 of correspondence = full) —
  // and (re)build the target copies when they do not hold the layout the kernel wants.  DevBuf::ensure is a compare when
  // the buffer is large enough, so a steady state allocates nothing.
  static StageAPlan plan_for(const StageAEnv& e, int64_t rows, int K) { return plan_stage_a(rows, e.M, K, e.tune.knn, e.tune.fallback_sliced_max); }
  template <class Obj>
  int begin(Obj* o, const StageAEnv& e, int64_t rows, int K, std::initializer_list<int> Ks, bool joint_sort = false) {
    plan = plan_for(e, rows, K);
    stage_kept = false;
    layout_pending = false;
    start_words_set = false;
    const size_t Bq = (size_t)rows, B = (size_t)e.B, M = (size_t)e.M, Mp = (size_t)plan.Mp;
    size_t S = 0, slice_entries = 0;
    for (const int k : Ks) { S = std::max<size_t>(S, knn_pool_size(k)); slice_entries = std::max<size_t>(slice_entries, (size_t)knn_slice_count(k) * k); }
    HIPCHK(o, cand_idx.ensure(Bq * K));   // mini-batch: the candidates of the unique drawn rows
    HIPCHK(o, cand_d2.ensure(Bq * K));
    if (plan.kernel == KnnKernel::Stream) {
      HIPCHK(o, pool_d.ensure(Bq * S)); HIPCHK(o, pool_i.ensure(Bq * S));
    } else {
      HIPCHK(o, fail_count.ensure(1));    // svnicp_get_knn_fallbacks; the brute-force kernel has none (its word is cleared when the registration begins)
    }
    if (plan.has_fallback()) {
      if (plan.kernel == KnnKernel::Tiles) {
        HIPCHK(o, pool2.ensure(Bq * kTilesBase));
        HIPCHK(o, arena.ensure((size_t)plan.arena_cap * kTilesChunk));
        HIPCHK(o, chunk_tab.ensure(tiles_chunk_tab_words(rows)));
        if (e.record_trace) HIPCHK(o, stat_n.ensure(B));
      } else {
        HIPCHK(o, pool2.ensure(Bq * plan.S2));
      }
      HIPCHK(o, fail_list.ensure(Bq)); HIPCHK(o, fail_tau.ensure(Bq));
      HIPCHK(o, qrec.ensure(Bq * 6));  // 48-byte records
      HIPCHK(o, pool_d.ensure((size_t)kFallbackGrid * 4 * kFallbackQW * S));   // fallback rows only
      HIPCHK(o, pool_i.ensure((size_t)kFallbackGrid * 4 * kFallbackQW * S));
      if (plan.sliced_max > 0) { HIPCHK(o, sl_d.ensure((size_t)plan.sliced_max * slice_entries)); HIPCHK(o, sl_i.ensure((size_t)plan.sliced_max * slice_entries)); }
      if (e.tune.full_corr) { HIPCHK(o, stage_fail_count.ensure(1)); HIPCHK(o, stage_fail_list.ensure(B)); }
    }
    if (plan.layout == TargetLayout::None) return SVNICP_OK;
    HIPCHK(o, tx.ensure(Mp)); HIPCHK(o, ty.ensure(Mp)); HIPCHK(o, tz.ensure(Mp));
    HIPCHK(o, txf.ensure(Mp)); HIPCHK(o, tyf.ensure(Mp)); HIPCHK(o, tzf.ensure(Mp));
    HIPCHK(o, torig.ensure(Mp)); HIPCHK(o, emax.ensure(1));
    if (plan.layout == TargetLayout::Morton) {   // both clouds are sorted along the curve: the target once, the queries per search
      const bool joint = joint_sort && held != plan.layout;   // one sort of M + B pairs with 31-bit keys: order_t holds both permutations
      const size_t nmax = joint ? M + B : std::max(M, B);
      const int bits = joint ? 31 : 30;
      HIPCHK(o, keys_a.ensure(nmax)); HIPCHK(o, keys_b.ensure(nmax)); HIPCHK(o, vals_a.ensure(nmax));
      HIPCHK(o, order_t.ensure(joint ? M + B : M)); HIPCHK(o, qorder.ensure(B));
      HIPCHK(o, bbox.ensure(6)); HIPCHK(o, tile_box.ensure(6 * (Mp / kTileSlots)));
      HIPCHK(o, tile_a.ensure(Mp)); HIPCHK(o, tile_o.ensure(Mp / kTileSlots));
      if (nmax > sort_n || bits > sort_bits) {   // rocPRIM's scratch for the larger of the two sorts seen so far
        sort_n = std::max(sort_n, nmax); sort_bits = std::max(sort_bits, bits);
        sort_tmp_bytes = std::max(sort_temp_bytes(sort_n, sort_bits), sort_temp_bytes(sort_n, 30));
        HIPCHK(o, sort_tmp.ensure(sort_tmp_bytes));
      }
      if (joint) { layout_pending = true; return SVNICP_OK; }
    }
    return ensure_layout(o, e);
  }

  // the target copies in the plan's layout, built on their own when they are not held
  template <class Obj>
  int ensure_layout(Obj* o, const StageAEnv& e) {
    layout_pending = false;
    start_words_set = false;
    if (held == plan.layout || plan.layout == TargetLayout::None) return SVNICP_OK;
    if (plan.layout == TargetLayout::Hashed) {
      HIPCHK(o, launch_targets_soa2(e.tgt, e.M, plan.Mp, tx.p, ty.p, tz.p, txf.p, tyf.p, tzf.p, torig.p, emax.p, e.stream));
    } else {
      HIPCHK(o, launch_bbox(e.tgt, e.M, bbox.p, false, e.stream));
      HIPCHK(o, launch_morton_order(e.tgt, 0, e.M, 0, e.pose0, bbox.p, keys_a.p, keys_b.p, vals_a.p, order_t.p, sort_tmp.p, sort_tmp_bytes,
                                    e.tune.sort_merge != 0, nullptr, 0, e.stream));
      HIPCHK(o, launch_targets_sorted(e.tgt, e.M, plan.Mp, order_t.p, tx.p, ty.p, tz.p, txf.p, tyf.p, tzf.p, torig.p, tile_box.p, emax.p, false, tile_a.p, tile_o.p, e.stream));
    }
    held = plan.layout;
    return SVNICP_OK;
  }

  // redo the queries listed in fail_list: few -> target-sliced scan + merge, many -> one wave per two queries
  hipError_t launch_fallback(KnnArgs a, hipStream_t stream) {
    a.qlist = fail_list.p; a.qlist_count = fail_count.p; a.list_grid = kFallbackGrid; a.list_qw = kFallbackQW;
    a.slice_max_queries = plan.sliced_max; a.slices = 0;
    hipError_t e = launch_knn_topk(a, stream);  // returns at once unless the list is longer than slice_max_queries
    if (e != hipSuccess || plan.sliced_max <= 0) return e;
    a.slices = knn_slice_count(a.K);
    a.merge_n = 1;
    while (a.merge_n < a.slices * a.K) a.merge_n <<= 1;
    a.sl_d = sl_d.p; a.sl_i = sl_i.p;
    e = launch_knn_topk(a, stream);
    if (e != hipSuccess) return e;
    return launch_knn_merge_slices(a, stream);
  }

  // option debug: (allocate and) clear the totals and `waves` per-wave records for the next launch
  template <class Obj>
  int clear_dbg_phase(Obj* o, hipStream_t stream, size_t waves) {
    HIPCHK(o, dbg_phase.ensure(8 + 8 * kDbgPhaseWaves));
    HIPCHK(o, hipMemsetAsync(dbg_phase.p, 0, (8 + 8 * waves) * sizeof(unsigned long long), stream));
    return SVNICP_OK;
  }

  // download and print what the kernel just launched on `n` queries has counted (brute force or Morton tiles)
  template <class Obj>
  int print_phases(Obj* o, const StageAEnv& e, int64_t n, size_t dbg_waves) {
    std::vector<unsigned long long> h(8 + 8 * dbg_waves);
    HIPCHK(o, hipMemcpyAsync(h.data(), dbg_phase.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, e.stream));
    HIPCHK(o, hipStreamSynchronize(e.stream));
    if (plan.kernel == KnnKernel::Brute) {
      const int qb = e.tune.brute_qb > 0 ? e.tune.brute_qb : knn_brute_queries_per_block(n, e.num_cus);
      const double nwg = (double)((n + qb - 1) / qb);
      fprintf(stderr, "[svnicp] k_knn_brute (%d queries per workgroup) thread-0 cycles per workgroup: pass A %.0f, bound %.0f, pass B %.0f, general path %.0f, rank + write %.0f\n",
              qb, h[0] / nwg, h[1] / nwg, h[2] / nwg, h[3] / nwg, h[4] / nwg);
      return SVNICP_OK;
    }
    unsigned long long ranked = 0;   // tiles scored in the seed kernel's rank phase: [7] of the per-wave records
    for (size_t w = 0; w < dbg_waves; ++w) ranked += h[8 + 8 * w + 7];
    fprintf(stderr, "[svnicp] k_knn_tiles wave cycles: rank %llu seed %llu scan %llu barrier waits + hand-over %llu | counts: rank tiles scored %llu seed tiles %llu scan tiles %llu scan (query, tile) pairs %llu\n", h[0], h[1], h[2], h[3], ranked, h[4], h[5], h[6]);
    // per-wave records of k_knn_seed: [0] rank (wave 0 of a group only) [1] seed [3] barrier waits [5] tile loop [6] K-th bisection
    auto column = [&](const char* tag, int col, unsigned long long floor_) {
      std::vector<unsigned long long> v;
      for (size_t w = 0; w < dbg_waves; ++w) { const unsigned long long x = h[8 + 8 * w + col]; if (x >= floor_) v.push_back(x); }
      if (v.empty()) return;
      std::sort(v.begin(), v.end());
      fprintf(stderr, "[svnicp]   seed kernel %-12s n %6zu  p50 %8llu  p90 %8llu  p99 %8llu  max %8llu cycles\n", tag, v.size(), v[v.size() / 2],
              v[v.size() * 9 / 10], v[v.size() * 99 / 100], v.back());
    };
    column("rank", 0, 5000); column("seed", 1, 1); column("tile loop", 5, 1); column("bisection", 6, 1); column("waits", 3, 0);
    return SVNICP_OK;
  }

  // exact top-K of pose·qsrc[b_lo, b_hi) against the whole target into out_idx / out_d2 ([rows][K]).  K is the plan's for
  // stage A proper; a caller with a K of its own (normal pass, correspondence = full) asks plan.can_search(K) first and
  // words the refusal itself.  At most plan.rows query rows.  tbl (tile kernels only, writes_table): the select kernel also
  // writes these rows' search table and leaves out_d2 to the rows the fallback kernels redo.  whole_source: the
  // registration's own search over all of its source rows — the one a pending layout was left to (joint sort).
  template <class Obj>
  int search(Obj* o, const StageAEnv& e, const double* qsrc, const Pose0& pose, int K, int32_t* out_idx, double* out_d2, int64_t b_lo,
             int64_t b_hi, const TableOut* tbl = nullptr, bool whole_source = false) {
    const int64_t n = b_hi - b_lo;
    const bool joint = layout_pending && whole_source && plan.kernel == KnnKernel::Tiles && b_lo == 0 && n == e.B && n > 0;
    if (layout_pending && !joint)
      if (const int rc = ensure_layout(o, e)) return rc;
    const bool words_set = start_words_set && joint;
    start_words_set = false;
    KnnArgs a{};
    a.src = qsrc; a.pose = pose; a.tx = tx.p; a.ty = ty.p; a.tz = tz.p; a.torig = torig.p;
    a.M = e.M; a.Mp = plan.Mp; a.b_lo = b_lo; a.b_hi = b_hi; a.K = K; a.S = knn_pool_size(K);
    a.pool_d = pool_d.p; a.pool_i = pool_i.p; a.out_idx = out_idx; a.out_d2 = out_d2;
    switch (plan.kernel) {
    case KnnKernel::Brute: {
      KnnBruteArgs k{};
      k.src = qsrc; k.pose = pose; k.tgt = e.tgt; k.M = e.M; k.b_lo = b_lo; k.b_hi = b_hi; k.K = K; k.out_idx = out_idx; k.out_d2 = out_d2;
      if (e.tune.debug) {
        if (const int rc = clear_dbg_phase(o, e.stream, 0)) return rc;
        k.phase_cycles = dbg_phase.p;
      }
      HIPCHK(o, launch_knn_brute(k, e.num_cus, e.tune.brute_qb, e.stream));
      if (e.tune.debug) return print_phases(o, e, n, 0);
      return SVNICP_OK;
    }
    case KnnKernel::Tiles: {
      if (n <= 0) return SVNICP_OK;
      const int32_t* qord = qorder.p + b_lo;
      const size_t tab_words = tiles_chunk_tab_words(plan.rows);   // all -1: written by the queries' key kernel on its way
      if (joint) {   // target and queries in one sort: order_t[0, M) is the target's permutation, order_t[M, M + n) the queries'
        HIPCHK(o, launch_bbox(e.tgt, e.M, bbox.p, words_set, e.stream));
        HIPCHK(o, launch_morton_order_joint(e.tgt, e.M, qsrc, n, pose, bbox.p, keys_a.p, keys_b.p, vals_a.p, order_t.p, sort_tmp.p, sort_tmp_bytes,
                                            e.tune.sort_merge != 0, chunk_tab.p, tab_words, e.stream));
        HIPCHK(o, launch_targets_sorted(e.tgt, e.M, plan.Mp, order_t.p, tx.p, ty.p, tz.p, txf.p, tyf.p, tzf.p, torig.p, tile_box.p, emax.p, words_set, tile_a.p, tile_o.p, e.stream));
        held = plan.layout; layout_pending = false;
        qord = order_t.p + e.M;
      } else {
        HIPCHK(o, launch_morton_order(qsrc, b_lo, n, 1, pose, bbox.p, keys_a.p, keys_b.p, vals_a.p, qorder.p + b_lo, sort_tmp.p, sort_tmp_bytes,
                                      e.tune.sort_merge != 0, chunk_tab.p, tab_words, e.stream));
      }
      KnnTilesArgs k{};
      k.src = qsrc; k.pose = pose; k.qorder = qord;
      k.tx = tx.p; k.ty = ty.p; k.tz = tz.p; k.txf = txf.p; k.tyf = tyf.p; k.tzf = tzf.p;
      k.torig = torig.p; k.tile_box = tile_box.p; k.emax_bits = emax.p;
      k.tile_a = tile_a.p; k.tile_o = tile_o.p; k.prefilter_mfma = e.tune.knn_prefilter_mfma; k.seed_rank_full = e.tune.seed_rank_full;
      k.M = e.M; k.Mp = plan.Mp; k.n_tiles = (int)(plan.Mp / kTileSlots); k.b_lo = b_lo; k.b_hi = b_hi; k.K = K; k.S2 = plan.S2;
      k.pool = pool2.p; k.out_idx = out_idx; k.out_d2 = tbl ? nullptr : out_d2;
      k.tgt = e.tgt;
      if (tbl) { k.tbl_a = tbl->rows; k.tbl_anchor = tbl->anchor; k.tbl_cmax = tbl->cmax; }
      k.arena = arena.p; k.chunk_tab = chunk_tab.p; k.arena_cap = plan.arena_cap; k.tab_rows = plan.rows;
      k.scan_split = e.tune.scan_split == 4 ? 4 : 8;
      {  // a small stride coprime to n_groups: 17 sweeps over the curve (C3 1.04 -> 0.98 ms, C5 1.83 -> 1.65 ms against natural order)
        const unsigned int ng = (unsigned int)((n + 63) / 64);
        unsigned int st = e.tune.group_stride > 0 ? (unsigned int)e.tune.group_stride : 17u;
        auto gcd = [](unsigned int x, unsigned int y) { while (y) { const unsigned int t = x % y; x = y; y = t; } return x; };
        while (st > 1 && gcd(st, ng) != 1) st += 2;
        if (ng <= 2 || st >= ng) st = 1;
        k.group_stride = st;
      }
      k.fail_list = fail_list.p; k.fail_count = fail_count.p; k.fail_tau = fail_tau.p; k.qrec = qrec.p;
      a.qthr = fail_tau.p;
      if (e.record_trace) k.stat_n = stat_n.p;
      if (!words_set) HIPCHK(o, hipMemsetAsync(fail_count.p, 0, sizeof(int), e.stream));
      const size_t dbg_waves = (size_t)((n + 63) / 64) * 4;   // seed kernel: four waves per 64-query group
      const bool dbg = e.tune.debug && dbg_waves <= kDbgPhaseWaves;   // larger launches are simply not instrumented
      if (dbg) {
        if (const int rc = clear_dbg_phase(o, e.stream, dbg_waves)) return rc;
        k.phase_cycles = dbg_phase.p;
      }
      HIPCHK(o, launch_knn_tiles(k, e.stream));
      if (dbg)
        if (const int rc = print_phases(o, e, n, dbg_waves)) return rc;
      HIPCHK(o, launch_fallback(a, e.stream));
      if (tbl)   // the rows the fallback kernels rewrote: gathered from out_idx, as k_build_table3 does for every row elsewhere
        HIPCHK(o, launch_build_table3_list(out_idx, fail_list.p, fail_count.p, e.B, K, e.tgt, e.M, tbl->anchor, tbl->rows, tbl->cmax, e.stream));
      return SVNICP_OK;
    }
    case KnnKernel::SeededScan: {   // f32 pre-filter (knn_scan.hip) with knn_topk.hip as fallback
      KnnScanArgs k{};
      k.src = qsrc; k.pose = pose; k.tx = tx.p; k.ty = ty.p; k.tz = tz.p;
      k.txf = txf.p; k.tyf = tyf.p; k.tzf = tzf.p; k.torig = torig.p; k.emax_bits = emax.p;
      k.M = e.M; k.Mp = plan.Mp; k.Ms = plan.scan_Ms; k.b_lo = b_lo; k.b_hi = b_hi; k.K = K; k.S2 = plan.S2;
      k.seed_rank = plan.scan_rank; k.pool = pool2.p; k.out_idx = out_idx; k.out_d2 = out_d2;
      k.fail_list = fail_list.p; k.fail_count = fail_count.p;
      HIPCHK(o, hipMemsetAsync(fail_count.p, 0, sizeof(int), e.stream));
      HIPCHK(o, launch_knn_scan(k, e.stream));
      // redo the (rare) queries whose seeded threshold was too tight: streaming kernel, list mode
      HIPCHK(o, launch_fallback(a, e.stream));
      return SVNICP_OK;
    }
    case KnnKernel::Stream:
      HIPCHK(o, launch_knn_topk(a, e.stream));
    }
    return SVNICP_OK;
  }

  // A later search of the registration's working set: the exact top-Kq of q[0, n) (already in the target's frame: the
  // identity pose) in blocks of the rows the scratch is sized for (a mini-batch registration sizes it for fewer than B).
  // Every block writes to out_idx / out_d2 + out_step * Kq * (its first row) — out_step 1: one [n][Kq] result, 0: every
  // block into the same block_rows(n) rows, which done(first row, rows) consumes behind its search (the normal pass: [n][Kq]
  // of a whole target would be gigabytes).  The caller has asked plan.can_search(Kq).
  int64_t block_rows(int64_t n) const { return std::max<int64_t>(1, std::min<int64_t>(plan.rows, n)); }
  template <class Obj, class Done = int (*)(int64_t, int64_t)>
  int search_blocks(Obj* o, const StageAEnv& e, const double* q, int64_t n, int Kq, int32_t* out_idx, double* out_d2, int out_step,
                    Done done = [](int64_t, int64_t) { return 0; }) {
    Pose0 ident{};
    ident.R0[0] = ident.R0[4] = ident.R0[8] = 1.0;
    const int64_t rows = block_rows(n);
    for (int64_t lo = 0; lo < n; lo += rows) {
      const int64_t cnt = std::min<int64_t>(rows, n - lo), off = lo * out_step * Kq;
      if (const int rc = search(o, e, q + 3 * lo, ident, Kq, out_idx + off, out_d2 + off, 0, cnt)) return rc;
      if (const int rc = done(lo, cnt)) return rc;
    }
    return SVNICP_OK;
  }

  // svnicp_get_knn_fallbacks / _rows describe STAGE A, not a later K = 1 search through the same working set: called behind
  // stage A when such searches follow (correspondence = full), or ahead of the first one (svnicp_evaluate, unless kept already).
  // The list is copied whole, plan.rows entries whatever the count says: the count lives on the device, so a copy of only
  // the listed rows would be a kernel of its own (the same launch for at most 0.5 MB less at C3), and neither caller is on
  // the path of a default registration.
  template <class Obj>
  int keep_stage_fallbacks(Obj* o, const StageAEnv& e) {
    if (!plan.has_fallback()) return SVNICP_OK;
    HIPCHK(o, stage_fail_count.ensure(1)); HIPCHK(o, stage_fail_list.ensure((size_t)plan.rows));
    HIPCHK(o, hipMemcpyAsync(stage_fail_count.p, fail_count.p, sizeof(int), hipMemcpyDeviceToDevice, e.stream));
    HIPCHK(o, hipMemcpyAsync(stage_fail_list.p, fail_list.p, (size_t)plan.rows * sizeof(int32_t), hipMemcpyDeviceToDevice, e.stream));
    stage_kept = true;
    return SVNICP_OK;
  }
  // what the getters read: the count of stage A's fallback rows (nullptr: the streaming kernel has no such notion), the rows
  // themselves, the survivor counts of the tile kernels' pre-filter (nullptr: not recorded)
  const int* fallback_count() const {
    if (plan.kernel == KnnKernel::Stream) return nullptr;
    return stage_kept ? stage_fail_count.p : fail_count.p;
  }
  const int32_t* fallback_rows() const { return stage_kept ? stage_fail_list.p : fail_list.p; }
  const int32_t* survivors(bool record_trace) const { return plan.kernel == KnnKernel::Tiles && record_trace ? stat_n.p : nullptr; }
};

}  // namespace svnicp_host
