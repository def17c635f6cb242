"""What a registration decides behind stage A, case by case (no GPU needed).

svn-icp_amd/csrc/registration_plan.hpp states as pure functions: the row counts of a (mini-batch) registration, what
svnicp_align_begin refuses and with which words, the stage-B variant and shape of a particle shard, whether the
registration is a small one, which launches carry its Stein step and how svnicp_align drives the iterations.  This test
compiles the header on the host, evaluates every case in one probe and compares.  The expectations were worked out by
hand from the rules (DESIGN.md sections 4.2, 4.3, 4.5, 4.8, 4.9), not taken from the header's output.

A case is (C++ statements that change the base facts `f` / options `t`, the expression to print, the expected text).
The base is a plain registration: P = 16 particles (the whole shard), K = 100, B = 1100 rows, M = 20000, 12 iterations,
SVN mode, no early stop, every option at its default.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svn-icp_amd", "csrc")

CHAINS = ("OneKernel", "SmallChain", "InlineMedian", "SideStream")
MB = "svnicp_align: mini-batch mode (svnicp_set_minibatch) is not available here: "
PLANE = "svnicp_align: the point-to-plane residual (svnicp_set_residual) is not available here: "

PROBE = r"""
#include <cstdio>
#include <string>
#include "registration_plan.hpp"
using namespace svnicp;
static void particles(RegistrationFacts& f, int P) { f.P = P; f.p_lo = 0; f.p_hi = P; }
static RegistrationFacts base() { RegistrationFacts f; particles(f, 16); f.K = 100; f.I = 12; f.B = 1100; f.M = 20000; return f; }
static std::string shape(const AccumPlan& p) { char b[96]; std::snprintf(b, sizeof b, "%d %d %d %d %d", p.PW, p.WP, p.grid_y, p.Ppad, p.RS); return b; }
static std::string rows(const RegistrationRows& r) { char b[96]; std::snprintf(b, sizeof b, "%d %lld %lld %lld", (int)r.mb, (long long)r.Bq, (long long)r.Bt, (long long)r.Bi); return b; }
static std::string msg(const char* prefix, const char* why) { return why ? std::string(prefix) + why : std::string("-"); }
static std::string num(long long v) { return std::to_string(v); }
// the registration as svnicp_align_begin plans it: stage-B plan (Bi rows per iteration), step, drive
static AccumPlan stage_b(const RegistrationFacts& f, const Tuning& t) { return plan_stage_b(f, t, registration_rows(f.batch, f.I, f.B).Bi); }
static StepPlan step(const RegistrationFacts& f, const Tuning& t) { return plan_step(f, t, stage_b(f, t)); }
static DrivePlan drive(const RegistrationFacts& f, const Tuning& t, bool blocking) { return plan_drive(f, t, stage_b(f, t), step(f, t), blocking); }
// a split-variant shape with one row of workgroups, for the rules no whole registration reaches
static AccumPlan split_row() { AccumPlan p{}; p.f32 = 3; p.grid_y = 1; p.PW = 16; p.WP = 1; return p; }
int main() {
@CASES@
  return 0;
}
"""

CASES = []


def case(name, setup, expr, expected):
    CASES.append((name, setup, expr, str(expected)))


# ---- shape: PW from 16 (split) or 8 (fused) doubling up to 64 and the shard; WP = ceil(n / 64) once PW = 64, 3 -> 4;
# grid_y = ceil(n / (PW WP)); Ppad = grid_y PW WP; RS = 3 K | 1 = 301 for K = 100
SHAPES = {  # nshard: (split, fused)
    1: ("16 1 1 16", "8 1 1 8"), 8: ("16 1 1 16", "8 1 1 8"), 9: ("16 1 1 16", "16 1 1 16"), 16: ("16 1 1 16", "16 1 1 16"),
    17: ("32 1 1 32", "32 1 1 32"), 33: ("64 1 1 64", "64 1 1 64"), 64: ("64 1 1 64", "64 1 1 64"), 65: ("64 2 1 128", "64 2 1 128"),
    128: ("64 2 1 128", "64 2 1 128"), 129: ("64 4 1 256", "64 4 1 256"), 192: ("64 4 1 256", "64 4 1 256"),
    257: ("64 4 2 512", "64 4 2 512"),
}
for n, (split, fused) in SHAPES.items():
    case("shape-split-%d" % n, "", "shape(stage_b_shape(3, %d, 100))" % n, split + " 301")
    case("shape-fused-%d" % n, "", "shape(stage_b_shape(1, %d, 100))" % n, fused + " 301")
case("shape-f64-9", "", "shape(stage_b_shape(0, 9, 100))", "16 1 1 16 301")
case("shape-row-stride-K4", "", "shape(stage_b_shape(1, 4, 4))", "8 1 1 8 13")        # 12 | 1
case("shape-empty", "", "shape(stage_b_shape(1, 0, 100))", "0 0 0 0 0")               # a variant and no grid

# ---- variant: (accum, K, nshard, full_corr, plane)
for name, args, v in [
        ("K128", "3, 128, 16, false, false", 3), ("K129", "3, 129, 16, false, false", 1),
        ("n8", "3, 100, 8, false, false", 1), ("n9", "3, 100, 9, false, false", 3),
        ("n4-full", "3, 100, 4, true, false", 3), ("n4-plane", "3, 100, 4, false, true", 3), ("n4-full-K129", "3, 129, 4, true, false", 1),
        ("f64", "0, 100, 16, false, false", 0), ("valu", "1, 100, 16, false, false", 1), ("f64-n4-full", "0, 100, 4, true, false", 0),
        ("empty-split", "3, 100, 0, false, false", 1), ("empty-split-full", "3, 100, 0, true, false", 1),
        ("empty-f64", "0, 100, 0, false, false", 0), ("empty-valu", "1, 100, 0, false, false", 1)]:
    case("variant-" + name, "", "num(stage_b_variant(%s))" % args, v)
case("variant-of-plan", "particles(f, 4); f.plane = true;", "num(stage_b(f, t).f32)", 3)
case("variant-of-plan-empty", "f.p_lo = f.p_hi = 5;", "num(stage_b(f, t).f32) + ' ' + shape(stage_b(f, t))", "1 0 0 0 0 0")

# ---- small: 16 particles x 32768 rows = 2^19 pairs; 3 x 174763 = 2^19 + 1
assert 16 * 32768 == 2 ** 19 and 128 * 4096 == 2 ** 19 and 3 * 174763 == 2 ** 19 + 1
SMALL = "num(stage_b(f, t).small)"
case("small-base", "", SMALL, 1)
case("small-pairs-2^19", "f.B = 32768;", SMALL, 1)
case("small-pairs-above", "f.B = 32769;", SMALL, 0)
case("small-pairs-2^19+1", "particles(f, 3);", "num(small_registration(split_row(), f, t, 174763))", 0)
case("small-pairs-2^19-2", "particles(f, 3);", "num(small_registration(split_row(), f, t, 174762))", 1)
case("small-minibatch-rows", "f.B = 40000; f.batch = 1000;", SMALL, 1)              # Bi = batch: 16000 pairs per iteration
case("small-P128", "particles(f, 128); f.B = 4096;", SMALL, 1)
case("small-P129", "particles(f, 129); f.B = 100;", SMALL, 0)
# the 128 of the prepare kernel's one-workgroup pair statistics is a bound of its own: option fused_update_max_p goes up to 700
case("small-P128-max-p-700", "particles(f, 128); f.B = 4096; t.fused_update_max_p = 700;", SMALL, 1)
case("small-P129-max-p-700", "particles(f, 129); f.B = 100; t.fused_update_max_p = 700;", SMALL, 0)
case("small-P2", "particles(f, 2);", "num(small_registration(split_row(), f, t, 1100))", 1)
case("small-P1", "particles(f, 1);", "num(small_registration(split_row(), f, t, 1100))", 0)
case("small-P8-fused-variant", "particles(f, 8);", SMALL, 0)
case("small-max-p-below", "t.fused_update_max_p = 15;", SMALL, 0)
case("small-max-p-equal", "t.fused_update_max_p = 16;", SMALL, 1)
case("small-chain-general", "t.small_chain = 0;", SMALL, 0)
case("small-update-fused", "t.update_fused = 1;", SMALL, 0)
case("small-row-shard", "f.row_world = 2;", SMALL, 0)
case("small-partial-shard", "f.shard_set = true; f.p_hi = 12;", SMALL, 0)
case("small-full-corr", "t.full_corr = 1;", SMALL, 0)
case("small-plane", "f.plane = true;", SMALL, 0)
case("small-accum-valu", "t.accum = 1;", SMALL, 0)
case("small-K129", "f.K = 129;", SMALL, 0)
case("small-two-rows-of-workgroups", "AccumPlan p = split_row(); p.grid_y = 2;", "num(small_registration(p, f, t, 1100))", 0)

# ---- chain
CHAIN = "num((int)step(f, t).chain)"


def chain(name, setup, expected):
    case("chain-" + name, setup, CHAIN, CHAINS.index(expected))


chain("P1", "particles(f, 1);", "OneKernel")
chain("P2", "particles(f, 2);", "InlineMedian")                          # <= 8 particles: fused variant, never small
chain("P16", "", "SmallChain")
chain("P128", "particles(f, 128);", "SmallChain")                        # 140800 pairs
chain("P129", "particles(f, 129);", "SideStream")
chain("P129-max-p-700", "particles(f, 129); t.fused_update_max_p = 700;", "SideStream")              # few pairs, yet not small
chain("P129-max-p-700-large", "particles(f, 129); f.B = 40000; t.fused_update_max_p = 700;", "SideStream")  # nor inline
chain("P128-max-p-700-large", "particles(f, 128); f.B = 40000; t.fused_update_max_p = 700;", "InlineMedian")
chain("update-fused", "t.update_fused = 1;", "OneKernel")
chain("update-fused-max-p-below", "t.update_fused = 1; t.fused_update_max_p = 15;", "SideStream")
chain("update-fused-max-p-equal", "t.update_fused = 1; t.fused_update_max_p = 16;", "OneKernel")
chain("general", "t.small_chain = 0;", "InlineMedian")
chain("median-stream-small", "t.median_inline = 0;", "SmallChain")       # stays on the small chain
chain("general-median-stream", "t.small_chain = 0; t.median_inline = 0;", "SideStream")
chain("large-default", "f.B = 40000;", "InlineMedian")
chain("large-median-stream", "f.B = 40000; t.median_inline = 0;", "SideStream")
chain("large-median-inline", "f.B = 40000; t.median_inline = 1;", "InlineMedian")
chain("max-p-below", "t.fused_update_max_p = 15;", "SideStream")
chain("plane", "f.plane = true;", "InlineMedian")
# svnicp_set_option after a begin: the stored plan's `small` holds, the new options decide the rest
case("chain-rerun-keeps-small", "const AccumPlan p = stage_b(f, t); t.small_chain = 0;", "num((int)plan_step(f, t, p).chain)", 1)

# ---- single_fused: P = 1, SVN, one row rank, shard [0, 1), fast correspondence, option single=fused, fused f32 variant, no plane
SINGLE = "num(step(f, t).single_fused)"
case("single-base", "particles(f, 1);", SINGLE, 1)
case("single-P2", "particles(f, 2);", SINGLE, 0)
case("single-svgd", "particles(f, 1); f.svgd = true;", SINGLE, 0)
case("single-row-shard", "particles(f, 1); f.row_world = 2;", SINGLE, 0)
case("single-empty-shard", "particles(f, 1); f.shard_set = true; f.p_hi = 0;", SINGLE, 0)
case("single-shard-1-1-of-one", "particles(f, 1); f.shard_set = true; f.p_lo = 1;", SINGLE, 0)   # the empty shard [1, 1)
case("single-full-corr", "particles(f, 1); t.accum = 1; t.full_corr = 1;", SINGLE, 0)      # accum=valu: the variant stays 1
case("single-option-split", "particles(f, 1); t.single_fused = 0;", SINGLE, 0)
case("single-f64", "particles(f, 1); t.accum = 0;", SINGLE, 0)
case("single-valu", "particles(f, 1); t.accum = 1;", SINGLE, 1)
case("single-plane", "particles(f, 1); t.accum = 1; f.plane = true;", SINGLE, 0)

# ---- drive
for K, ok in ((96, 0), (97, 1), (100, 1), (101, 0)):
    for (PW, WP), inst in (((16, 1), 1), ((64, 2), 1), ((64, 4), 0)):
        case("supported-%d-%d-%d" % (PW, WP, K), "", "num(small_registration_supported(%d, %d, %d))" % (PW, WP, K), ok & inst)
    case("persistent-P16-K%d" % K, "f.K = %d; t.persistent = 1;" % K, "num(drive(f, t, true).persistent_try)", ok)
    case("persistent-P100-K%d" % K, "particles(f, 100); f.K = %d; t.persistent = 1;" % K, "num(drive(f, t, false).persistent_try)", ok)
case("persistent-64x4", "t.persistent = 1; AccumPlan p = split_row(); p.PW = 64; p.WP = 4; p.small = 1; StepPlan s; s.chain = StepChain::SmallChain;",
     "num(plan_drive(f, t, p, s, true).persistent_try)", 0)
case("persistent-off", "", "num(drive(f, t, true).persistent_try)", 0)
case("persistent-trace", "t.persistent = 1; f.record_trace = true;", "num(drive(f, t, true).persistent_try)", 0)
case("persistent-profiling", "t.persistent = 1; f.profiling = true;", "num(drive(f, t, true).persistent_try)", 0)
case("persistent-no-iterations", "t.persistent = 1; f.I = 0;", "num(drive(f, t, true).persistent_try)", 0)
case("persistent-general-chain", "t.persistent = 1; f.B = 40000;", "num(drive(f, t, true).persistent_try)", 0)
DEFER = "num(drive(f, t, true).defer_fin)"
case("defer-base", "f.check_early_stop = true;", DEFER, 1)
case("defer-async", "f.check_early_stop = true;", "num(drive(f, t, false).defer_fin)", 1)
case("defer-no-early-stop", "", DEFER, 0)
case("defer-trace", "f.check_early_stop = true; f.record_trace = true;", DEFER, 0)
case("defer-fused-variant", "f.check_early_stop = true; t.accum = 1;", DEFER, 0)
case("defer-full-corr", "f.check_early_stop = true; t.full_corr = 1;", DEFER, 0)
case("defer-one-kernel", "f.check_early_stop = true; t.update_fused = 1;", DEFER, 0)
case("follow-I8", "f.check_early_stop = true; f.I = 8;", "num(drive(f, t, true).follow)", 0)
case("follow-I9", "f.check_early_stop = true; f.I = 9;", "num(drive(f, t, true).follow)", 1)
case("follow-async", "f.check_early_stop = true; f.I = 9;", "num(drive(f, t, false).follow)", 0)
case("follow-no-early-stop", "f.I = 9;", "num(drive(f, t, true).follow)", 0)

# ---- refusals
MBR = "msg(kMinibatchRefusal, minibatch_refusal(f, t))"
case("mb-off", "t.full_corr = 1;", MBR, "-")
case("mb-fine", "f.batch = 100;", MBR, "-")
case("mb-negative", "f.batch = -1;", MBR, MB + "batch_size must be positive")
case("mb-partial-shard", "f.batch = 100; f.shard_set = true; f.p_lo = 4;", MBR, MB + "a partial particle shard (svnicp_set_shard) is set")
case("mb-whole-shard-set", "f.batch = 100; f.shard_set = true;", MBR, "-")
case("mb-row-shard", "f.batch = 100; f.row_world = 2;", MBR, MB + "a source-row shard (svnicp_set_row_shard) is set")
case("mb-full-corr", "f.batch = 100; t.full_corr = 1;", MBR, MB + "option correspondence=full is set")
case("mb-persistent", "f.batch = 100; t.persistent = 1;", MBR, MB + "option chain=persistent is set")
case("mb-rows-2^22", "f.batch = 1 << 20; f.I = 4;", MBR, "-")
case("mb-rows-above", "f.batch = (1 << 20) + 1; f.I = 4;", MBR,
     MB + "iterations * batch_size exceeds 2^22 table rows (about 2.5 KB of tables per row)")
case("mb-table-iterations", "f.batch = 100; f.explicit_tab = true; f.tab_I = 11;", MBR,
     MB + "the explicit index table's iteration count differs from params.iterations")
case("mb-table-fine", "f.batch = 100; f.explicit_tab = true; f.tab_I = 12;", MBR, "-")
case("mb-first-of-two", "f.batch = -1; t.full_corr = 1;", MBR, MB + "batch_size must be positive")
PLR = "msg(kPlaneRefusal, plane_refusal(f, t))"
case("plane-off", "f.svgd = true;", PLR, "-")
case("plane-fine", "f.plane = true;", PLR, "-")
case("plane-svgd", "f.plane = true; f.svgd = true;", PLR, PLANE + "SVGD mode has no Hessian to put the plane residual in")
case("plane-partial-shard", "f.plane = true; f.shard_set = true; f.p_hi = 8;", PLR, PLANE + "a partial particle shard (svnicp_set_shard) is set")
case("plane-row-shard", "f.plane = true; f.row_world = 2;", PLR,
     PLANE + "a source-row shard (svnicp_set_row_shard) is set: the rank exchange carries the 22 point-to-point sums")
case("plane-minibatch", "f.plane = true; f.batch = 100;", PLR, PLANE + "mini-batch mode (svnicp_set_minibatch) is set")
case("plane-full-corr", "f.plane = true; t.full_corr = 1;", PLR, PLANE + "option correspondence=full is set")
case("plane-persistent", "f.plane = true; t.persistent = 1;", PLR, PLANE + "option chain=persistent is set")
case("plane-accum", "f.plane = true; t.accum = 1;", PLR,
     PLANE + "option accum is not split: the plane kernel consumes the search kernel's winner index")
case("plane-K129", "f.plane = true; f.K = 129;", PLR,
     PLANE + "knn_count exceeds 128: the plane kernel consumes the matrix-pipe search kernel's winner index")
case("plane-few-targets", "f.plane = true; f.M = 15;", PLR, PLANE + "the target has fewer points than normal_k and no normals were supplied")
case("plane-few-targets-supplied", "f.plane = true; f.M = 15; f.normals_supplied = true;", PLR, "-")
case("plane-first-of-two", "f.plane = true; f.svgd = true; t.accum = 0;", PLR, PLANE + "SVGD mode has no Hessian to put the plane residual in")
FULL_SPLIT = "correspondence = full needs the split stage B (accum = split, more than 8 particles or knn_count <= 128)"
FULL_K1 = "correspondence = full needs knn_count <= 128 (Morton-tile stage A) or knn = v1"
case("full-off", "", 'msg("", full_corr_refusal(f, t, 1, false))', "-")
case("full-fine", "t.full_corr = 1;", 'msg("", full_corr_refusal(f, t, 3, true))', "-")
case("full-variant", "t.full_corr = 1;", 'msg("", full_corr_refusal(f, t, 1, true))', FULL_SPLIT)
case("full-stage-a", "t.full_corr = 1;", 'msg("", full_corr_refusal(f, t, 3, false))', FULL_K1)
case("full-first-of-two", "t.full_corr = 1;", 'msg("", full_corr_refusal(f, t, 0, false))', FULL_SPLIT)
case("full-empty-shard", "t.full_corr = 1; f.shard_set = true; f.p_lo = f.p_hi = 3;", 'msg("", full_corr_refusal(f, t, 1, false))', "-")
# the registration of test_full_correspondence_mode_refusals: 4 particles, K = 200
case("full-P4-K200", "particles(f, 4); f.K = 200; t.full_corr = 1;", 'msg("", full_corr_refusal(f, t, stage_b(f, t).f32, false))', FULL_SPLIT)

# ---- row counts: mb, stage-A rows, table rows, rows per iteration
case("rows-plain", "", "rows(registration_rows(0, 12, 1000))", "0 1000 1000 1000")
case("rows-table-below-B", "", "rows(registration_rows(100, 5, 1000))", "1 500 500 100")
case("rows-table-above-B", "", "rows(registration_rows(100, 5, 300))", "1 300 500 100")
case("rows-no-iterations", "", "rows(registration_rows(100, 0, 1000))", "0 1000 1000 1000")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("registration_plan")
    lines = "\n".join('  { RegistrationFacts f = base(); Tuning t; (void)f; (void)t; %s std::printf("%d|%%s\\n", std::string(%s).c_str()); }'
                      % (setup, i, expr.replace("'", '"')) for i, (_, setup, expr, _) in enumerate(CASES))
    (d / "probe.cpp").write_text(PROBE.replace("@CASES@", lines))
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)
    out = subprocess.run([str(d / "probe")], check=True, capture_output=True, text=True).stdout
    return dict((int(i), v) for i, v in (l.split("|", 1) for l in out.splitlines()))


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_registration_plan(probe, i):
    name, setup, expr, expected = CASES[i]
    assert probe[i] == expected, (name, setup, expr)


def test_header_needs_no_hip():
    """the header includes the standard library and stage_a_plan.hpp, nothing of HIP"""
    inc = [l.split()[1] for l in open(os.path.join(CSRC, "registration_plan.hpp")) if l.startswith("#include")]
    assert inc and all(i in ("<cstddef>", "<cstdint>", "<initializer_list>", '"stage_a_plan.hpp"') for i in inc), inc
