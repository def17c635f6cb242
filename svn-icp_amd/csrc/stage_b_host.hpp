// stage_b_host.hpp — host-only: stage B (nearest of K, the 22 sums) as svnicp_ctx holds it.  The rules are in
// registration_plan.hpp; here are the tables and per-iteration scratch, ONE sizing of them per registration and the table
// build.  Reports through the owning object's error path, like stage_a_host.hpp.
#pragma once
#include <algorithm>
#include <cstdio>
#include <string>

#include "device_buffer.hpp"
#include "kernels.hpp"

namespace svnicp_host {
using namespace svnicp;

struct StageB {
  AccumPlan plan{};    // of the registration begun last (begin)
  DevBuf<double> table, anchor, sums, partial;   // sums [P][kNSums] follows the particles (svnicp_set_particles)
  DevBuf<float4> tablef, tablea;
  DevBuf<float> cmaxb;
  DevBuf<uint8_t> kbest;
  DevBuf<int32_t> kidx;
  DevBuf<int> ambig;   // [0] wave steps with an undecided lane, [1] undecided (point, particle) pairs (cleared when the registration begins)
  DevBuf<double> full_q, full_d2;      // correspondence = full: one particle's transformed source, its nearest distances
  DevBuf<int32_t> full_idx;            // … and the nearest target of every (particle of the shard, source point): [P][B]

  // Start of a registration: complete the plan for this device and size everything for it — tables of r.Bt rows, scratch of
  // r.Bi rows per iteration, and correspondence = full's buffers when the shard is not empty.
  template <class Obj>
  int begin(Obj* o, const RegistrationFacts& f, const Tuning& t, const RegistrationRows& r, const AccumPlan& shape, int num_cus) {
    const size_t Bt = (size_t)r.Bt, Bi = (size_t)r.Bi, K = (size_t)f.K;
    plan = shape;
    HIPCHK(o, cmaxb.ensure(Bt));
    HIPCHK(o, ambig.ensure(2));
    if (f.nshard() > 0) {
      plan = plan_accumulate(shape, r.Bi, num_cus, t);
      if (t.debug)
        fprintf(stderr, "[svnicp] stage-B plan: mode=%d PW=%d WP=%d TP=%d grid=%dx%d tiles/block=%d smem=%zu sgrid=%d pts/block=%d/%d\n", plan.f32,
                plan.PW, plan.WP, plan.TP, plan.grid_x, plan.grid_y, plan.tiles_per_block, plan.smem, plan.sgrid_x, plan.spts_per_block,
                plan.pts_per_block);
      if (plan.smem > 160u * 1024)   // K > 128 runs the LDS-tile VALU search: its smallest tile must fit one CU's LDS
        return fail(o, SVNICP_ERR_INVALID, "svnicp_align: knn_count " + std::to_string(f.K) + " needs " + std::to_string(plan.smem) +
                    " bytes of LDS per workgroup (limit 163840): the candidate count is too large for this particle count");
      HIPCHK(o, partial.ensure((size_t)std::max(plan.grid_x, f.P == 1 ? single_particle_grid(r.Bi) : 0) * plan.Ppad * kNSums));
      if (t.full_corr) {
        HIPCHK(o, full_q.ensure((size_t)f.B * 3)); HIPCHK(o, full_d2.ensure((size_t)f.B));
        HIPCHK(o, full_idx.ensure((size_t)f.P * f.B));
      }
    }
    if (plan.f32 == 3) {   // the split variant gathers from the target cloud
      HIPCHK(o, tablea.ensure(Bt * 128)); HIPCHK(o, anchor.ensure(Bt * 3));
      HIPCHK(o, kbest.ensure(Bi * plan.Ppad)); HIPCHK(o, kidx.ensure(Bi * plan.Ppad));
    } else {
      HIPCHK(o, table.ensure(Bt * K * 3)); HIPCHK(o, tablef.ensure(Bt * K));
    }
    return SVNICP_OK;
  }

  // the candidate table of `rows` rows from stage A's indices cand [rows][K]
  template <class Obj>
  int build_table(Obj* o, const int32_t* cand, int64_t rows, int K, const double* tgt, int64_t M, hipStream_t stream) {
    if (plan.f32 == 3)
      HIPCHK(o, launch_build_table3(cand, rows, K, tgt, M, nullptr, anchor.p, tablea.p, cmaxb.p, stream));
    else
      HIPCHK(o, launch_build_table2(cand, rows, K, tgt, M, table.p, tablef.p, cmaxb.p, stream));
    return SVNICP_OK;
  }
};

}  // namespace svnicp_host
