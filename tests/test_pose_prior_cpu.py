"""The Gaussian pose prior on the correction without a GPU (include/svnicp_hip.h "pose prior").

1. the contract's gradient J^T Lambda e against the central difference of 1/2 e^T Lambda e along the right perturbation, in mpmath;
2. the planning rules and the refusal ladder of registration_plan.hpp with the prior on, compiled on the host;
3. svnicp::pose_prior::validate through tests/pose_prior_driver.cpp, built with the address and undefined-behaviour sanitizers;
4. the two symbols and the unchanged parameter block;
5. the degenerate scene (a plane seen from above) through the oracle's split-phase Stein step: with the prior the one particle
   lands on the prior's mean, without it it stays where it started; 64 particles contract to the prior's width.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import pose_prior_cases as cases
import pose_prior_reference as pref
import stein_step_reference as ss
import test_registration_plan_cpu as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svn-icp_amd", "csrc")
PRIOR = "svnicp_align: the pose prior (svnicp_set_pose_prior) is not available here: "


# ---------------- 1. gradient against the central difference, 60 digits, h = 1e-20 ----------------
GRAD_CASES = [   # (name, rotation vector of R_p, t_p, mean6, Lambda)
    ("e_r_zero", [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], np.zeros(6), "full"),
    ("e_t_only", [0.0, 0.0, 0.0], [0.3, -0.1, 0.2], np.zeros(6), "full"),
    ("below_series_threshold", [3e-3, -4e-3, 0.0], [0.1, 0.2, -0.3], np.zeros(6), "full"),
    ("above_series_threshold", [0.0, 1.2e-2, 1.6e-2], [0.1, 0.2, -0.3], np.zeros(6), "full"),
    ("theta_2.5", [1.5, -2.0, 0.0], [0.1, 0.2, -0.3], np.zeros(6), "full"),
    ("mean_nonzero", [0.3, 0.1, -0.2], [0.1, 0.2, -0.3], cases.MU_NONZERO, "full"),
    ("mean_nonzero_diag", [0.3, 0.1, -0.2], [0.1, 0.2, -0.3], cases.MU_NONZERO, "diag"),
    ("rank1", [0.3, 0.1, -0.2], [0.1, 0.2, -0.3], cases.MU_NONZERO, "rank1"),
    ("huge", [0.03, 0.01, -0.02], [0.1, 0.2, -0.3], cases.MU_NONZERO, "huge"),
]


@pytest.mark.parametrize("name,rvec,tp,mean6,lam", GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_gradient_is_the_derivative_of_the_cost(name, rvec, tp, mean6, lam):
    """J^T Lambda e equals d/d(delta) 1/2 e^T Lambda e at R_p Exp(delta_r), t_p + R_p delta_t.  Central difference with
    h = 1e-20 at 60 digits: truncation O(h^2) = 1e-40, rounding 1e-60 / 1e-20 = 1e-40 of the cost: 1e-15 of the gradient's
    largest entry is loose by 20 orders (an absolute floor of 1e-30 max|Lambda| covers e = 0, where both are 0)."""
    A = ss.MP()
    m = A.m
    L = [float(v) for v in cases.LAMBDAS[lam]().reshape(36)]
    Rp = pref.exp_host(A, [A.c(v) for v in rvec], guard=0)
    tpc = [A.c(v) for v in tp]
    g, G = pref.prior_terms(A, Rp, tpc, pref.exp_host(A, mean6[3:6]), [A.c(v) for v in mean6[:3]], [A.c(v) for v in L])
    h = m.mpf(10) ** -20
    D = ss.MP()                       # the differences need the exact Log: so3_log's |sin| <= 1e-12 branch returns 0 for a step of 1e-20
    D.V = frozenset({"no_guards"})
    fd = []
    for k in range(6):
        d = [m.mpf(0)] * 6
        d[k] = h
        X = D if k >= 3 else A
        cp = pref.cost(X, *pref.perturbed(X, Rp, tpc, d), mean6, L)
        d[k] = -h
        cm = pref.cost(X, *pref.perturbed(X, Rp, tpc, d), mean6, L)
        fd.append((cp - cm) / (2 * h))
    scale = max(max(abs(v) for v in g), m.mpf(1e-15) * max(abs(v) for v in L))
    err = max(abs(fd[k] - g[k]) for k in range(6))
    print("%s: max |fd - g| = %s, max |g| = %s" % (name, m.nstr(err, 5), m.nstr(max(abs(v) for v in g), 5)))
    assert err <= m.mpf(1e-15) * scale
    # J^T Lambda J is the Gauss-Newton Hessian of the same cost: symmetric, and positive semi-definite like Lambda
    Gm = np.array([[float(G[6 * i + j]) for j in range(6)] for i in range(6)])
    assert np.array_equal(Gm, Gm.T)
    assert np.linalg.eigvalsh(Gm).min() >= -1e-9 * max(np.abs(Gm).max(), 1e-300)


def test_prior_does_not_see_the_initial_mean():
    """J_t = R_p, not R0 R_p: the terms added to a record are the same for every initial mean (the data term's translation
    tangent t_tot += R0 R_p dt is t += R_p dt of the correction)."""
    A = ss.F64()
    x = cases.particles(8)
    L = cases.lam_full().reshape(36)
    sums = cases.sums(8)
    R0 = cases.far_mean()[:3, :3].reshape(9)
    eye = np.eye(3).reshape(9)
    for p in range(8):
        Rp, _ = ss.so3_exp(A, [np.float64(v) for v in x[3:, p]])
        with np.errstate(all="ignore"):
            Ha, ba = pref.record(A, sums[p], eye, Rp, x[:3, p], cases.MU_NONZERO, L)
            H0, b0 = pref.record(A, sums[p], eye, Rp, x[:3, p], cases.MU_NONZERO, None)
            Hb, bb = pref.record(A, sums[p], R0, Rp, x[:3, p], cases.MU_NONZERO, L)
            H1, b1 = pref.record(A, sums[p], R0, Rp, x[:3, p], cases.MU_NONZERO, None)
        assert np.allclose(np.array(Ha) - np.array(H0), np.array(Hb) - np.array(H1), rtol=0, atol=1e-9 * np.abs(Ha).max())
        assert np.allclose(np.array(ba) - np.array(b0), np.array(bb) - np.array(b1), rtol=0, atol=1e-9 * np.abs(ba).max())
        assert not np.allclose(b0, b1)


def test_restatement_agrees_with_mpmath_on_the_kernel_cases():
    """The float64 restatement against the mpmath one on the particle sets of the GPU test: E_f64 of the bar stays small (the
    two are different programs: series against closed form, host Rodrigues against the exact one)."""
    F, M = ss.F64(), ss.MP()
    x = cases.particles(8)
    sums = cases.sums(8)
    eye = np.eye(3).reshape(9)
    R = []
    for p in range(8):
        Rp, _ = ss.so3_exp(F, [np.float64(v) for v in x[3:, p]])
        R.append([float(v) for v in Rp])
    for lam in ("diag", "full", "rank1", "zero", "huge"):
        L = cases.LAMBDAS[lam]().reshape(36)
        Hf, bf = pref.records(F, sums, eye, R, x[:3].T, cases.MU_NONZERO, L)
        Hm, bm = pref.records(M, sums, eye, R, x[:3].T, cases.MU_NONZERO, L)
        for p in range(8):
            eh, eb = pref.rel_err(Hf[p], Hm[p]), pref.rel_err(bf[p], bm[p])
            assert eh is not None and eb is not None
            assert eh < 1e-13 and eb < 1e-12, (lam, p, eh, eb)
        assert np.array_equal(Hf, Hf.reshape(8, 6, 6).transpose(0, 2, 1).reshape(8, 36)), "H must stay exactly symmetric"


# ---------------- 2. planning and refusals ----------------
PLAN_CASES = []


def case(name, setup, expr, expected):
    PLAN_CASES.append((name, "f.prior = true; " + setup, expr, str(expected)))


# the base registration (16 particles, 1100 rows) is a small one: with the prior it is not, and runs the inline chain
case("small-off", "", rp.SMALL, 0)
case("small-P128", "particles(f, 128); f.B = 4096;", rp.SMALL, 0)
case("small-direct", "particles(f, 3);", "num(small_registration(split_row(), f, t, 1100))", 0)
case("chain-P16", "", rp.CHAIN, rp.CHAINS.index("InlineMedian"))
case("chain-P128", "particles(f, 128);", rp.CHAIN, rp.CHAINS.index("InlineMedian"))
case("chain-P129", "particles(f, 129);", rp.CHAIN, rp.CHAINS.index("SideStream"))
case("chain-P1", "particles(f, 1);", rp.CHAIN, rp.CHAINS.index("OneKernel"))
case("chain-update-fused", "t.update_fused = 1;", rp.CHAIN, rp.CHAINS.index("OneKernel"))
case("chain-median-stream", "t.median_inline = 0;", rp.CHAIN, rp.CHAINS.index("SideStream"))
case("chain-plane", "f.plane = true;", rp.CHAIN, rp.CHAINS.index("InlineMedian"))
case("single-base", "particles(f, 1);", rp.SINGLE, 0)
case("single-valu", "particles(f, 1); t.accum = 1;", rp.SINGLE, 0)
# the stage-B variant is chosen as ever
case("variant-P16", "", "num(stage_b(f, t).f32)", 3)
case("variant-P8", "particles(f, 8);", "num(stage_b(f, t).f32)", 1)
case("variant-P4-plane", "particles(f, 4); f.plane = true;", "num(stage_b(f, t).f32)", 3)
case("shape-P16", "", "shape(stage_b(f, t))", "16 1 1 16 301")
case("rows-minibatch", "f.batch = 100;", "rows(registration_rows(f.batch, f.I, f.B))", "1 1100 1200 100")
case("persistent-never-tried", "f.K = 100;", "num(drive(f, t, true).persistent_try)", 0)
case("defer-base", "f.check_early_stop = true;", "num(drive(f, t, true).defer_fin)", 1)
PRR = "msg(kPriorRefusal, prior_refusal(f, t))"
case("refusal-fine", "", PRR, "-")
case("refusal-svgd", "f.svgd = true;", PRR, PRIOR + "SVGD mode: its gradient does not pass through the H | b record the prior is added to")
case("refusal-partial-shard", "f.shard_set = true; f.p_hi = 8;", PRR, PRIOR + "a partial particle shard (svnicp_set_shard) is set")
case("refusal-whole-shard-set", "f.shard_set = true;", PRR, "-")
case("refusal-row-shard", "f.row_world = 2;", PRR, PRIOR + "a source-row shard (svnicp_set_row_shard) is set")
case("refusal-persistent", "t.persistent = 1;", PRR, PRIOR + "option chain=persistent is set")
case("refusal-first-of-two", "f.svgd = true; t.persistent = 1;", PRR,
     PRIOR + "SVGD mode: its gradient does not pass through the H | b record the prior is added to")
case("allowed-minibatch", "f.batch = 100;", PRR + " + msg(kMinibatchRefusal, minibatch_refusal(f, t))", "--")
case("allowed-plane", "f.plane = true;", PRR + " + msg(kPlaneRefusal, plane_refusal(f, t))", "--")
case("allowed-full-corr", "t.full_corr = 1;", PRR, "-")
case("allowed-update-fused", "t.update_fused = 1;", PRR, "-")
case("allowed-weighting", "f.weighting = 1;", PRR + " + msg(kWeightingRefusal, weighting_refusal(f, t))", "--")
case("allowed-P1", "particles(f, 1);", PRR, "-")
PLAN_CASES.append(("off-is-no-refusal", "f.svgd = true; t.persistent = 1; f.row_world = 2;", PRR, "-"))
PLAN_CASES.append(("off-default-false", "", "num(f.prior)", "0"))
# an initialiser that names no prior (the struct's last member) leaves it off
PLAN_CASES.append(("off-aggregate", "RegistrationFacts g{16, 100, 12}; f = g;", "num(f.prior) + num(f.weighting)", "00"))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    d = tmp_path_factory.mktemp("pose_prior_plan")
    lines = "\n".join('  { RegistrationFacts f = base(); Tuning t; (void)f; (void)t; %s std::printf("%d|%%s\\n", std::string(%s).c_str()); }'
                      % (setup, i, expr.replace("'", '"')) for i, (_, setup, expr, _) in enumerate(PLAN_CASES))
    (d / "probe.cpp").write_text(rp.PROBE.replace("@CASES@", lines))
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)
    out = subprocess.run([str(d / "probe")], check=True, capture_output=True, text=True).stdout
    return dict((int(i), v) for i, v in (l.split("|", 1) for l in out.splitlines()))


@pytest.mark.parametrize("i", range(len(PLAN_CASES)), ids=[c[0] for c in PLAN_CASES])
def test_plan_with_prior(probe, i):
    name, setup, expr, expected = PLAN_CASES[i]
    assert probe[i] == expected, (name, setup, expr)


def test_prior_is_the_last_fact():
    """RegistrationFacts::prior is the struct's last data member, so existing positional initialisers stay valid."""
    txt = open(os.path.join(CSRC, "registration_plan.hpp")).read()
    body = txt[txt.index("struct RegistrationFacts {"):txt.index("int nshard() const")]
    members = [l.strip() for l in body.splitlines() if l.strip() and not l.strip().startswith("//")]
    assert members[-1].startswith("bool prior = false;"), members[-1]


# ---------------- 3. validation, under the sanitizers ----------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    d = tmp_path_factory.mktemp("pose_prior_driver")
    exe = str(d / "pose_prior_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "pose_prior_driver.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict((l.split("|")[0], l.split("|")[1:]) for l in r.stdout.splitlines())


ACCEPTED = ("identity", "zero", "huge", "rank1", "asymmetric_within_tolerance", "eigenvalue_-1e-13_relative", "mean_rotation_3.1", "mean_general")
REFUSED = {"asymmetric": "the information matrix is not symmetric", "nan_entry": "the information matrix holds a non-finite entry",
           "inf_entry": "the information matrix holds a non-finite entry", "nan_mean": "the mean holds a non-finite entry",
           "negative_diagonal": "the information matrix has a negative diagonal entry",
           "eigenvalue_-1e-6": "the information matrix has a negative eigenvalue",
           "mean_rotation_pi": "the mean's rotation vector is not shorter than pi", "null": "null argument"}


@pytest.mark.parametrize("name", ACCEPTED)
def test_validation_accepts(driver, name):
    rc, why, asym, orth = driver[name]
    assert (rc, why) == ("0", "-")
    assert float(asym) == 0.0, "the stored matrix is symmetrised"
    assert float(orth) < 1e-15 * 4, "R_mu is a rotation"


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_validation_refuses(driver, name):
    rc, why = driver[name][:2]
    assert rc == "-1" and why == REFUSED[name]


def test_header_needs_no_hip():
    inc = [l.split()[1] for l in open(os.path.join(CSRC, "pose_prior.hpp")) if l.startswith("#include")]
    assert inc == ["<cmath>", '"information_solve.hpp"'], inc


# ---------------- 4. ABI ----------------
def test_symbols_are_declared_exported_and_bound(pkg):
    from svnicp_amd.binding import Params
    L = pkg.load_library()
    dp = C.POINTER(C.c_double)
    for n in ("svnicp_set_pose_prior", "svnicp_get_pose_prior", "svnicp_particle_pose_devptr"):
        assert n in pkg.declared_symbols() and hasattr(L, n)
    assert L.svnicp_set_pose_prior.argtypes == [C.c_void_p, dp, dp]
    assert L.svnicp_get_pose_prior.argtypes == [C.c_void_p, C.POINTER(C.c_int), dp, dp]
    assert L.svnicp_set_pose_prior(None, None, None) == -1 and L.svnicp_get_pose_prior(None, None, None, None) == -1
    assert L.svnicp_particle_pose_devptr(None, 0) is None
    assert C.sizeof(Params) == 56 and pkg.abi_version() == 1
    assert callable(pkg.SVNICP.set_pose_prior) and callable(pkg.SVNICP.pose_prior) and callable(pkg.SVGDICP.set_pose_prior)


# ---------------- 5. the degenerate scene through the oracle's Stein step ----------------
@pytest.fixture(scope="module")
def scene_runs(orc):
    src, tgt, nrm = cases.plane_scene()
    out = {}
    for P in (1, 64):
        init = cases.scene_particles(P)
        for prior in (True, False):
            out[P, prior] = pref.run_scene(orc, src, tgt, nrm, init, cases.SCENE_K, cases.SCENE_ITERS, 1.0, float("inf"),
                                           cases.SCENE_MU if prior else None, cases.scene_lambda() if prior else None)
    return out


def test_scene_one_particle_lands_on_the_mean(scene_runs):
    x = scene_runs[1, True].particles.reshape(6)
    print("P = 1 with prior: pose - mu =", x - cases.SCENE_MU)
    assert np.abs(x - cases.SCENE_MU).max() < 1e-6


def test_scene_without_prior_stays_where_it_started(scene_runs):
    x = scene_runs[1, False].particles.reshape(6)
    print("P = 1 without prior: (x, y) =", x[:2])
    assert np.linalg.norm(x[:2] - cases.SCENE_MU[:2]) > 0.1


def test_scene_particles_contract_to_the_prior(scene_runs):
    sx = scene_runs[64, True].particles.reshape(6, 64)[0].std(ddof=1)
    s0 = scene_runs[64, False].particles.reshape(6, 64)[0].std(ddof=1)
    print("P = 64: std of x with prior %.4f, without %.4f" % (sx, s0))
    assert sx < 0.5 * s0
