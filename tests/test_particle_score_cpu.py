"""Score and weight the particles (include/svnicp_hip.h), the part that needs no GPU: the numpy
restatement on hand-made cases, the ABI declarations and bindings, the refusal ladders of registration_plan.hpp compiled on
the host, and the preconditions of what tests/test_particle_score_gpu.py compares exactly (on the CPU oracle's candidates and
poses: if a cloud fails one, change its seed in tests/particle_score_cases.py, not the bound)."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import particle_score_cases as pc
import particle_score_reference as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svn-icp_amd", "csrc")
IDENTITY = np.r_[np.eye(3).ravel(), 0.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------------ the restatement alone
def test_cost_by_hand_on_three_points():
    src = np.array([[0.0, 0, 0], [1, 0, 0], [5, 5, 5]])
    tgt = np.array([[0.1, 0, 0], [1, 0.2, 0], [9, 9, 9]])
    cand = np.array([[0, 1], [0, 1], [2, 0]], np.int32)
    nrm = np.array([[1.0, 0, 0], [0, 0, 0], [0, 1, 0]])
    # row 0: candidates at d2 0.01 and 1.04 -> 0.01, inlier, normal (1, 0, 0): r = -0.1.  row 1: 0.81 and 0.04 -> 0.04, inlier,
    # zero normal.  row 2: 48 and 73.01 -> 48, beyond the gate 0.5^2.  cost = (0.05 + 1 * 0.25) / 3 = 0.1
    got = ps.score(src, tgt, cand, IDENTITY[None], 0.5, normals=nrm)[0]
    assert got[:3].tolist() == [3.0, 2.0, 1.0]
    assert np.allclose(got[3:], [0.05, 0.01, 0.1], rtol=1e-15, atol=0)
    assert ps.score(src, tgt, cand, IDENTITY[None], 0.5)[0].tolist()[:3] == [3.0, 2.0, 0.0]
    # strict '<' from candidate 0: a tie keeps the first, a NaN first distance is never replaced, indices are clamped
    tie = ps.pairs(np.zeros((1, 3)), np.array([[1.0, 0, 0], [0, 1.0, 0]]), np.array([[1, 0]]), IDENTITY[None])
    assert tie.idx[0, 0] == 1 and tie.second[0, 0] == 1.0
    nan0 = ps.score(np.zeros((2, 3)), np.array([[np.nan, 0, 0], [0.1, 0, 0]]), np.array([[0, 1], [7, -3]]), IDENTITY[None], 1.0)[0]
    assert nan0.tolist()[:3] == [1.0, 1.0, 0.0] and not np.isnan(nan0).any()        # row 1: 7 -> 1 (d2 0.01), -3 -> 0 (NaN)
    # a 1e160 row is evaluated (d2 = +inf) and never an inlier; a NaN source row is not evaluated; both cost the gate
    bad = ps.score(np.array([[1e160, 0, 0], [np.nan, 0, 0]]), tgt, cand[:2], IDENTITY[None], 0.5, normals=nrm)[0]
    assert bad.tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 0.25]


def test_weights_sum_to_one_and_flatten_with_temperature():
    cost = np.array([0.031, 0.030, 0.0345, 0.05, 0.030001])
    w = ps.weights(cost, 1e-3)
    assert abs(w.sum() - 1.0) < 1e-15 and w.argmax() == 1 and (np.diff(w[np.argsort(cost)]) <= 0).all()
    assert np.abs(ps.weights(cost, 1e9) - 0.2).max() < 1e-11                         # temperature -> large: uniform
    cold = ps.weights(cost, 1e-9)                                                     # the cold case: second best is 1e-6 away
    assert cold[1] == 1.0 and np.count_nonzero(cold) == 1


def test_weighted_stats_with_equal_weights_are_the_oracle_s(pkg, orc):
    src, tgt = pc.clouds(pkg, "random")
    init = pc.particles(pkg, 16)
    o = orc.Solver(init, iterations=3, lr=pc.LR, max_dist=1.0, knn_count=16, svn_full_grad=False)
    o.add_cloud(src, tgt, init)
    o.stein_align()
    mean, var, cov = ps.weighted_stats(o.get_particles(), np.full(16, 1.0 / 16))
    assert np.abs(mean - o.get_transformation()).max() < 1e-12 and np.abs(var - o.get_distribution()).max() < 1e-12
    assert np.abs(cov.reshape(36) - o.get_cov_matrix()).max() < 1e-12
    x = np.arange(12.0)                                     # [6, 2]: rows (0, 1), (2, 3), ...
    m, v, c = ps.weighted_stats(x, [0.25, 0.75])
    assert np.allclose(m, x.reshape(6, 2) @ [0.25, 0.75]) and np.allclose(v, 0.1875) and np.allclose(c, 0.1875)


# ------------------------------------------------------------------------------------------------ ABI and bindings
def test_abi_declares_and_exports_the_scoring_entry_points(pkg):
    names = pkg.declared_symbols()
    L = pkg.load_library()
    for n in ("svnicp_score_particles", "svnicp_set_particle_weighting", "svnicp_get_particle_scores"):
        assert n in names and hasattr(L, n), n
    dp = C.POINTER(C.c_double)
    assert L.svnicp_score_particles.argtypes == [C.c_void_p, C.c_double, dp, dp]
    assert L.svnicp_set_particle_weighting.argtypes == [C.c_void_p, C.c_int, C.c_double, C.c_double]
    assert L.svnicp_get_particle_scores.argtypes == [C.c_void_p, dp, dp]
    hdr = open(os.path.join(ROOT, "include", "svnicp_hip.h")).read()
    for macro, value in (("SVNICP_SCORE_FIELDS", 6), ("SVNICP_WEIGHT_UNIFORM", 0), ("SVNICP_WEIGHT_SOFTMIN", 1), ("SVNICP_ABI_VERSION", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), hdr), macro
    assert pkg.abi_version() == 1 and C.sizeof(pkg.binding.Params) == 56            # svnicp_params is unchanged
    # a NULL context is refused, not dereferenced
    assert L.svnicp_score_particles(None, 0.3, None, None) == -1
    assert L.svnicp_set_particle_weighting(None, 1, 0.3, 1e-3) == -1 and L.svnicp_get_particle_scores(None, None, None) == -1


def test_host_mirrors_carry_the_option(pkg):
    w = pkg.ParticleWeightOpt()
    assert dataclasses.asdict(w) == dict(use_weight_mean=False, weight_dist=0.0, temperature=0.0)
    assert "inert" in pkg.ParticleWeightOpt.__doc__
    assert callable(pkg.SVNICP.score_particles) and callable(pkg.SVNICP.get_particle_scores)
    assert [f.name for f in dataclasses.fields(pkg.ParticleScores)] == list(ps.FIELDS) + ["poses"]
    cfg = pkg.pipeline.PipelineConfig()
    assert cfg.weight_dist == 0.0 and cfg.weight_temperature == 0.0
    for bad in (dict(weight_dist=-1.0), dict(weight_dist=float("nan")), dict(weight_dist=0.3), dict(weight_dist=0.3, weight_temperature=float("inf"))):
        with pytest.raises(ValueError):
            pkg.pipeline.PipelineConfig(**bad)
    assert pkg.pipeline.PipelineConfig(weight_dist=0.3, weight_temperature=1e-3).weight_dist == 0.3
    sm = pkg.stein_msgs
    prm = pkg.SteinICPParam(iterations=7, lr=0.5)
    for opt, want in ((None, False), (pkg.ParticleWeightOpt(True), False), (pkg.ParticleWeightOpt(False, 0.3, 1e-3), False),
                      (pkg.ParticleWeightOpt(True, 0.3, 1e-3), True)):
        m = sm.decode("stein_msgs/SteinParameters", sm.encode(sm.fill_parameters(prm, opt, 1.5, particle_count=9, voxel_size=0.5)))
        assert m["weight_mean"] is want and m["iterations"] == 7 and m["particle_count"] == 9 and m["voxel_size"] == 0.5
    shim = open(os.path.join(ROOT, "svn-icp_amd", "host", "svnicp_hip_shim.hpp")).read()
    for needle in ("weight_dist", "temperature", "score_particles", "get_particle_scores", "SVNICP_WEIGHT_SOFTMIN"):
        assert needle in shim, needle
    host = open(os.path.join(ROOT, "svn-icp_amd", "host", "registration_pipeline.hpp")).read()
    assert "weight_dist" in host and "weight_temperature" in host


# ------------------------------------------------------------------------------------------------ the refusal ladders
WEIGHTING = "svnicp_align: particle weighting (svnicp_set_particle_weighting) is not available here: "
SCORING = "svnicp_score_particles: the last registration cannot be scored: "
LADDER_CASES = [   # (statements on the base facts f / options t, expression, expected text)
    ("", "msg(kWeightingRefusal, weighting_refusal(f, t))", "-"),                        # uniform: nothing is refused …
    ("f.svgd = true; f.batch = 8;", "msg(kWeightingRefusal, weighting_refusal(f, t))", "-"),   # … whatever else is set
    ("f.weighting = 1;", "msg(kWeightingRefusal, weighting_refusal(f, t))", "-"),
    ("f.weighting = 1; f.plane = true; f.K = 330; f.check_early_stop = true;", "msg(kWeightingRefusal, weighting_refusal(f, t))", "-"),
    ("f.weighting = 2;", "msg(kWeightingRefusal, weighting_refusal(f, t))", WEIGHTING + "unknown weighting kind"),
    ("f.weighting = -1; f.svgd = true;", "msg(kWeightingRefusal, weighting_refusal(f, t))", WEIGHTING + "unknown weighting kind"),
    ("f.weighting = 1; f.svgd = true;", "msg(kWeightingRefusal, weighting_refusal(f, t))",
     WEIGHTING + "SVGD mode: the weight option belongs to SVNICP's constructor only"),
    ("f.weighting = 1; f.shard_set = true; f.p_hi = 8;", "msg(kWeightingRefusal, weighting_refusal(f, t))",
     WEIGHTING + "a partial particle shard (svnicp_set_shard) is set"),
    ("f.weighting = 1; f.shard_set = true;", "msg(kWeightingRefusal, weighting_refusal(f, t))", "-"),       # the whole shard
    ("f.weighting = 1; f.row_world = 2;", "msg(kWeightingRefusal, weighting_refusal(f, t))",
     WEIGHTING + "a source-row shard (svnicp_set_row_shard) is set: this context holds a part of the scan"),
    ("f.weighting = 1; f.batch = 64;", "msg(kWeightingRefusal, weighting_refusal(f, t))",
     WEIGHTING + "mini-batch mode (svnicp_set_minibatch) is set: its candidate tables are per drawn position"),
    ("f.weighting = 1; t.full_corr = 1;", "msg(kWeightingRefusal, weighting_refusal(f, t))",
     WEIGHTING + "option correspondence=full is set: the iterations did not search the candidate table"),
    ("f.weighting = 1; f.svgd = true; f.batch = 64;", "msg(kWeightingRefusal, weighting_refusal(f, t))",     # the first that holds
     WEIGHTING + "SVGD mode: the weight option belongs to SVNICP's constructor only"),
    ("", "msg(kScoringRefusal, scoring_refusal(f, t))", "-"),
    ("f.svgd = true; f.plane = true; f.K = 600; t.accum = 1; t.small_chain = 0;", "msg(kScoringRefusal, scoring_refusal(f, t))", "-"),
    ("f.shard_set = true; f.p_lo = 8;", "msg(kScoringRefusal, scoring_refusal(f, t))", SCORING + "a partial particle shard (svnicp_set_shard) is set"),
    ("f.row_world = 4;", "msg(kScoringRefusal, scoring_refusal(f, t))",
     SCORING + "a source-row shard (svnicp_set_row_shard) is set: this context holds a part of the scan"),
    ("f.batch = 1;", "msg(kScoringRefusal, scoring_refusal(f, t))",
     SCORING + "mini-batch mode (svnicp_set_minibatch) is set: its candidate tables are per drawn position"),
    ("t.full_corr = 1;", "msg(kScoringRefusal, scoring_refusal(f, t))",
     SCORING + "option correspondence=full is set: the iterations did not search the candidate table"),
    ("f = RegistrationFacts{};", "std::to_string(f.weighting + (int)t.full_corr)", "0"),                           # the one new field, defaulted
]
PROBE = r"""
#include <cstdio>
#include <string>
#include "registration_plan.hpp"
using namespace svnicp;
static RegistrationFacts base() { RegistrationFacts f; f.P = 16; f.p_lo = 0; f.p_hi = 16; f.K = 100; f.I = 12; f.B = 1100; f.M = 20000; return f; }
static std::string msg(const char* prefix, const char* why) { return why ? std::string(prefix) + why : std::string("-"); }
int main() {
@CASES@
  return 0;
}
"""


def test_refusal_ladders_compiled_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    body = "\n".join('  { RegistrationFacts f = base(); Tuning t; %s std::printf("%%s\\n", std::string(%s).c_str()); }' % (setup, expr)
                     for setup, expr, _ in LADDER_CASES)
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE.replace("@CASES@", body))
    exe = tmp_path / "probe"
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    assert len(out) == len(LADDER_CASES)
    for (setup, expr, want), got in zip(LADDER_CASES, out):
        assert got == want, (setup, expr)


# ------------------------------------------------------------------------------------------------ preconditions of the GPU cases
_ORACLE = {}


def _oracle_run(pkg, orc, cloud, P, K, iterations):
    """(source, target, candidates, total poses [P, 12]) of the CPU oracle's registration of a parity case (SVN mode)."""
    key = (cloud, P, K, iterations)
    if key not in _ORACLE:
        src, tgt = pc.clouds(pkg, cloud)
        init, T0 = pc.particles(pkg, P), pc.initial_mean(pkg)
        o = orc.Solver(init, iterations=iterations, lr=pc.LR, max_dist=1.0, knn_count=K, svn_full_grad=False)
        o.add_cloud(src, tgt, init)
        o.set_initial_mean(T0[:3, :3], T0[:3, 3])
        o.stein_align()
        poses = pc.total_poses(lambda w: orc.so3_exp(w)[0], o.get_particles(), T0)
        _ORACLE[key] = (src, tgt, o.candidates(), poses)
    return _ORACLE[key]


@pytest.mark.parametrize("K", pc.KS)
@pytest.mark.parametrize("P", pc.PS)
def test_no_pair_of_the_parity_cases_sits_on_a_gate_or_a_tie(pkg, orc, P, K):
    src, tgt, cand, poses = _oracle_run(pkg, orc, pc.cloud_of(P, K), P, K, pc.iterations_of(P, K))
    pr = ps.pairs(src, tgt, cand, poses)
    for gate in pc.GATES:
        near_gate, tie = ps.preconditions(pr, gate)
        assert near_gate.size == 0 and tie.size == 0, (gate, near_gate[:4], tie[:4])
    # the case says something: most rows are inliers at the wide gate, fewer at the narrow one, and the particles differ
    wide, narrow = ps.score(src, tgt, cand, poses, 1.0, pr=pr), ps.score(src, tgt, cand, poses, 0.3, pr=pr)
    assert (wide[:, 0] == pc.B_).all() and (wide[:, 1] > 0.5 * pc.B_).all() and (narrow[:, 1] <= wide[:, 1]).all()
    if P > 1:
        assert np.unique(narrow[:, 5]).size > 1


@pytest.mark.parametrize("cloud", pc.CLOUDS)
def test_the_cold_case_has_one_best_particle(pkg, orc, cloud):
    src, tgt, cand, poses = _oracle_run(pkg, orc, cloud, pc.WEIGHT_P, pc.WEIGHT_K, 3)
    cost = np.sort(ps.score(src, tgt, cand, poses, pc.WEIGHT_GATE)[:, 5])
    assert cost[1] - cost[0] >= 1e-6, cost[:3]
    w = ps.weights(cost, pc.COLD_T)
    assert w[0] == 1.0 and not w[1:].any()
    assert ps.weights(cost, pc.WEIGHT_T).min() > 0.0          # the warm temperature spreads the weight over every particle
