"""The plane and GICP forms of the particle scores without a GPU: pins tests/particle_score_objective_reference.py (the numpy
float64 restatement the GPU tests compare the device against) on its own — against the point restatement, against closed forms,
against mpmath and against the solver's own gradient — and the presence of the new interface in the host layers."""
import os

import numpy as np
import pytest

from conftest import so3_exp_np

import gicp_reference as gr
import particle_score_cases as pc
import particle_score_objective_cases as oc
import particle_score_objective_mp_reference as pm
import particle_score_objective_reference as po
import particle_score_reference as ps
import plane_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
INF = float("inf")
_CASES = {}


def _case(pkg, orc, cloud, P=16, K=16):
    """(src, tgt, nt, ns, cand, poses [P, 12], pairs): the shared clouds with unit normals of both, the oracle's candidates at the
    initial mean and the total poses of the particle prior — what a scoring sees before the first iteration."""
    key = (cloud, P, K)
    if key not in _CASES:
        src, tgt = pc.clouds(pkg, cloud)
        nt = pr.normals(orc, tgt, 16)[0]
        ns = gr.normalise_supplied(oc.source_normals(orc, src, cloud), src)
        T0 = pc.initial_mean(pkg)
        cand, _ = orc.knn_topk(orc.transform(src, T0[:3, :3], T0[:3, 3]), tgt, K)
        poses = pc.total_poses(so3_exp_np, pc.particles(pkg, P), T0)
        _CASES[key] = (src, tgt, nt, ns, cand, poses, ps.pairs(src, tgt, cand, poses))
    return _CASES[key]


ALL = [(c, P, K) for c in pc.CLOUDS for P, K in ((16, 16), (4, 1), (25, 128))]


@pytest.mark.parametrize("cloud,P,K", ALL)
def test_plane_form_without_robust_weight_is_the_point_restatement_bitwise(pkg, orc, cloud, P, K):
    src, tgt, nt, ns, cand, poses, pairs = _case(pkg, orc, cloud, P, K)
    for gate in oc.GATES:
        point = ps.score(src, tgt, cand, poses, gate, normals=nt, pr=pairs)
        plane = po.score(po.PLANE, src, tgt, cand, poses, gate, normals=nt, delta=INF, pr=pairs)
        assert plane[:, 2].min() > 0
        assert plane[:, :5].tobytes() == point[:, :5].tobytes()            # sum_h == sum_r2 and the four fields before it


@pytest.mark.parametrize("cloud,P,K", ALL)
def test_gicp_closed_forms(pkg, orc, cloud, P, K):
    """epsilon = 1: W = I exactly (S = 2 I, cofactors 4, det 8, k = 2 / 8), so rho2 is |Rt^T e|^2 and differs from d2 = |e|^2 by
    the rounding of the rotation alone: 8 u |e|^2.  n_s = m: S = 2 C(m), rho2 = (1 - eps) r^2 + eps |e|^2; at epsilon = 1 to the
    same bound, and for smaller epsilon to that bound times cond(S) = 1 / eps, the accuracy a closed-form inverse has
    (tests/gicp_mp_reference.py states why)."""
    src, tgt, nt, ns, cand, poses, pairs = _case(pkg, orc, cloud, P, K)
    gate = max(oc.GATES)
    R = poses[:, :9]
    t = po.terms(po.GICP, pairs, poses, gate, nt, ns, INF, 1.0)
    a = t.accepted
    assert a.any()
    e2 = (pairs.e ** 2).sum(axis=2)
    err = np.abs(t.x2 - pairs.d2)[a] / e2[a]
    print(f"{cloud} P {P} K {K}: eps = 1: max |rho2 - d2| / |e|^2 = {err.max() / U:.2f} u over {a.sum()} pairs")
    assert err.max() <= 8 * U
    n = np.where(a[..., None], nt[pairs.idx], 0.0)
    ez = np.where(a[..., None], pairs.e, 0.0)
    u, m = po.rotate_back(R, ez), po.rotate_back(R, n)
    r = (n * ez).sum(axis=2)
    for eps in (1.0, 0.5, 1e-3):
        rho2, _ = po.gicp_rho2(u, m, m, np.float64(eps))
        want = (1.0 - eps) * r * r + eps * e2
        err = np.abs(rho2 - want)[a] / e2[a]
        print(f"{cloud} P {P} K {K}: n_s = m, eps {eps}: max |rho2 - ((1 - eps) r^2 + eps |e|^2)| / |e|^2 = {err.max() / U:.2f} u, bound {8 / eps:.0f} u")
        assert err.max() <= 8 * U / eps


@pytest.mark.parametrize("cloud,P,K", ALL)
def test_no_accepted_pair_costs_more_than_the_cap(pkg, orc, cloud, P, K):
    src, tgt, nt, ns, cand, poses, pairs = _case(pkg, orc, cloud, P, K)
    for form in (po.PLANE, po.GICP):
        for gate in oc.GATES:
            for delta in oc.DELTAS:
                for eps in ((oc.EPS, 1e-6, 1.0) if form == po.GICP else (oc.EPS,)):
                    t = po.terms(form, pairs, poses, gate, nt, ns, delta, eps)
                    cap = po.cap(gate, delta)
                    assert t.accepted.any() and (t.h[t.accepted] <= cap).all() and (t.h[~t.accepted] == 0.0).all()
                    assert (t.x[t.accepted] < gate).all()                 # x <= |e| < gate: |n| = 1, W's eigenvalues in [eps, 1]
                    sc = po.score(form, src, tgt, cand, poses, gate, normals=nt, src_normals=ns, delta=delta, eps=eps, pr=pairs)
                    assert (sc[:, 5] <= cap).all() and (sc[:, 5] > 0).all() and np.isfinite(sc).all()


@pytest.mark.parametrize("form", [po.PLANE, po.GICP])
@pytest.mark.parametrize("cloud", pc.CLOUDS)
def test_sum_h_against_mpmath(pkg, orc, cloud, form):
    """Three particles of the 16: the float64 sum within 300 u of the mpmath sum in units of the yardstick (300 additions of
    terms each known to a few u of its yardstick entry; particle_score_objective_mp_reference.py)."""
    src, tgt, nt, ns, cand, poses, pairs = _case(pkg, orc, cloud)
    for gate, delta in ((0.3, 0.05), (1.0, INF)):
        f64 = po.score(form, src, tgt, cand, poses, gate, normals=nt, src_normals=ns, delta=delta, eps=oc.EPS, pr=pairs)[:, 4]
        particles = (0, 7, 15)
        val, mag = pm.sum_h_mp(form, pairs, poses, gate, nt, ns, delta, oc.EPS, particles)
        import mpmath
        for p, v, g in zip(particles, val, mag):
            err = float(abs(v - mpmath.mpf(float(f64[p]))) / g)
            print(f"{cloud} form {form} gate {gate} delta {delta} particle {p}: |f64 - mp| / mag = {err / U:.2f} u")
            assert err <= 300 * U


# ------------------------------------------------------------------------------------------------ it is the objective the solver minimised
def _exp(w):
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if a == 0:
        return np.eye(3), np.eye(3)
    return (np.eye(3) + np.sin(a) / a * K + (1 - np.cos(a)) / a ** 2 * K @ K,
            np.eye(3) + (1 - np.cos(a)) / a ** 2 * K + (a - np.sin(a)) / a ** 3 * K @ K)      # R, left Jacobian


@pytest.mark.parametrize("form", [po.PLANE, po.GICP])
def test_the_cost_is_the_objective_the_solver_minimised(pkg, orc, form):
    """make_pair(2048, 8192) with supplied normals, max_corr_dist = sqrt(max_dist) (the solver gates the SQUARED distance against
    max_dist): the central difference of B * cost / 2 = sum h / 2 + constant along the six right-perturbation axes is b of
    tests/plane_reference.py resp. tests/gicp_reference.py (W frozen at the linearisation pose, as the solver has it).  The pairs
    are held fixed: asserted, no pair crosses the gate, delta or its runner-up within the step, so the rejected rows' constant
    cancels exactly and sum_h is differenced itself.

    Tolerance from the step h alone, as tests/test_plane_cpu.py derives it.  Plane: |r'|, |r''|, |r'''| <= L := 1 + |s|, the
    third derivative of a pair's term is at most 3 L^2 + delta L.  GICP: the solver freezes the metric Rt W Rt^T of a pair in
    the target frame, so the frozen cost is h(|y|) with y = W^(1/2) Rt^T e(xi), Rt and W taken at xi = 0 and e at the perturbed
    pose; e is the vector of the plane form and |W| <= 1, so |y'|, |y''|, |y'''| <= L with the same L.  Inside delta the term
    y.y / 2 has third derivative <= 3 L^2 + L, beyond it delta |y| with |y| > delta has <= delta (L + 3 L^2 / delta + 3 L^3 / delta^2).
    The central difference is off by h^2 / 6 of the sum; round-off: two sums of N terms, N eps sum / h."""
    p = pkg.scans.make_pair(2048, 8192)
    src, tgt = p.source, p.target
    nt = pr.normals(orc, tgt, 16)[0]
    ns = pr.normals(orc, src, 16)[0]
    K, delta, max_dist, h, eps = 8, 0.05, 0.25, 1e-6, oc.EPS
    gate = float(np.sqrt(max_dist))
    assert gate * gate == max_dist
    R0, t0 = _exp(np.array([0.002, 0.001, -0.003]))[0], np.array([0.01, 0.02, -0.01])
    x6 = np.array([0.1, 0.05, -0.03, -0.003, 0.005, 0.008])      # a pose at which the preconditions asserted below hold
    Rt, tt = pr.total_pose(orc, x6, R0, t0)
    cand, _ = orc.knn_topk(orc.transform(src, R0, t0), tgt, K)
    if form == po.PLANE:
        rec, slot, stats, res = pr.record_one(src, tgt, nt, cand, Rt, tt, max_dist, delta)
    else:
        rec, slot, stats, res = gr.record_one(src, tgt, nt, ns, cand, Rt, tt, max_dist, delta, eps)
    b = rec[36:]

    def pose12(xi):
        dR, J = _exp(xi[3:])
        return np.concatenate([(Rt @ dR).reshape(9), tt + Rt @ (J @ xi[:3])])[None]

    pose0 = pose12(np.zeros(6))
    base = ps.pairs(src, tgt, cand, pose0)
    t0_ = po.terms(form, base, pose0, gate, nt, ns, delta, eps)
    acc = t0_.accepted[0]
    assert acc.sum() == stats[0] and 0 < acc.sum() < len(src), "the scoring's accepted pairs are the solver's; the gate rejects some"
    out = t0_.x[0][acc] > delta
    assert 0.05 <= out.mean() <= 0.95, f"{out.mean():.3f} of the accepted pairs lie outside delta"
    W0 = None
    if form == po.GICP:     # W of every pair at the linearisation pose, [B, 6]
        W0 = np.stack(po.gicp_weight(po.rotate_back(pose0[:, :9], np.where(acc[None, :, None], nt[base.idx], 0.0)),
                                     np.where(acc[None, :, None], ns[None], 0.0), np.float64(eps)), axis=-1)[0]

    def sum_h(xi):
        """(sum h over the pairs accepted at xi = 0, the pairs of xi): the metric Rt W Rt^T frozen for the GICP form."""
        pose = pose12(xi)
        prs = ps.pairs(src, tgt, cand, pose)
        t = po.terms(form, prs, pose, gate, nt, ns, delta, eps)
        if form == po.PLANE:
            return t.h[0].sum(), prs, t
        u = po.rotate_back(pose0[:, :9], np.where(acc[None, :, None], prs.e, 0.0))[0]
        v = np.stack([W0[:, 0] * u[:, 0] + W0[:, 1] * u[:, 1] + W0[:, 2] * u[:, 2], W0[:, 1] * u[:, 0] + W0[:, 3] * u[:, 1] + W0[:, 4] * u[:, 2],
                      W0[:, 2] * u[:, 0] + W0[:, 4] * u[:, 1] + W0[:, 5] * u[:, 2]], axis=1)
        rho2 = np.maximum((u * v).sum(axis=1), 0.0)
        return po.h(np.sqrt(rho2), rho2, np.float64(delta))[acc].sum(), prs, t

    s = src[acc]
    L = 1.0 + np.linalg.norm(s, axis=1)
    third = 3 * L * L + delta * L if form == po.PLANE else np.where(out, delta * L + 3 * L * L + 3 * L ** 3 / delta, 3 * L * L + L)
    f0 = sum_h(np.zeros(6))[0]
    tol = (h * h / 6.0) * third.sum() + acc.sum() * np.finfo(float).eps * (f0 / 2) / h
    g = np.zeros(6)
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        (fp, pp, tp), (fm, pm_, tm) = sum_h(d), sum_h(-d)
        for prs, t in ((pp, tp), (pm_, tm)):        # the pairs are held fixed: nothing crosses the gate, delta or its runner-up
            assert np.array_equal(prs.kb, base.kb) and np.array_equal(t.accepted, t0_.accepted) and np.array_equal(t.inlier, t0_.inlier), k
            assert np.array_equal(t.x[0][acc] > delta, out), k
        g[k] = (fp - fm) / (4 * h)                  # B * cost / 2 = sum_h / 2 + the rejected rows' constant
    err = np.abs(g - b).max()
    print(f"form {form}: {acc.sum()} pairs, {out.sum()} beyond delta; max |central difference - b| = {err:.3e}, bound {tol:.3e}, |b| max {np.abs(b).max():.3e}")
    assert err <= tol
    assert tol < 1e-3 * np.abs(b).max(), "the bound must be far below b itself, or the check shows nothing"


# ------------------------------------------------------------------------------------------------ the recorded weights case
def test_the_recorded_case_ranks_differently_under_the_two_costs(pkg, orc):
    """particle_score_objective_cases.RANKS_DIFFERENTLY on the CPU: the GICP registration of the weights case through the oracle
    (tests/gicp_reference.py with the cases' prior), both costs by the restatements at its final poses.  The argmins are the
    recorded ones, they differ, and each leads its runner-up by more than 1e-6 m^2 — a thousand times what separates the device's
    poses from the oracle's can move a cost."""
    cloud, K = oc.RANKS_DIFFERENTLY
    src, tgt, nt, ns, _, _, _ = _case(pkg, orc, cloud)
    T0 = pc.initial_mean(pkg)
    ref = gr.run(orc, src, tgt, nt, ns, pc.particles(pkg, pc.WEIGHT_P), K, 3, 1.0, oc.SOLVER_DELTA, oc.EPS, lr=pc.LR, svn_full_grad=False,
                 R0=T0[:3, :3], t0=T0[:3, 3], prior=(oc.PRIOR_MEAN, oc.PRIOR_LAMBDA))
    poses = pc.total_poses(so3_exp_np, ref.particles, T0)
    cand, _ = orc.knn_topk(orc.transform(src, T0[:3, :3], T0[:3, 3]), tgt, K)
    pairs = ps.pairs(src, tgt, cand, poses)
    gicp = po.score(po.GICP, src, tgt, cand, poses, pc.WEIGHT_GATE, normals=nt, src_normals=ns, delta=oc.SOLVER_DELTA, eps=oc.EPS, pr=pairs)[:, 5]
    point = ps.score(src, tgt, cand, poses, pc.WEIGHT_GATE, normals=nt, pr=pairs)[:, 5]
    og, op = np.argsort(gicp), np.argsort(point)
    print(f"{cloud} K {K}: argmin under the GICP cost {og[0]} (leads by {gicp[og[1]] - gicp[og[0]]:.3e}), under the point cost {op[0]} "
          f"(leads by {point[op[1]] - point[op[0]]:.3e})")
    assert (int(og[0]), int(op[0])) == oc.ARGMIN[cloud, K] and og[0] != op[0]
    assert gicp[og[1]] - gicp[og[0]] > 1e-6 and point[op[1]] - point[op[0]] > 1e-6


# ------------------------------------------------------------------------------------------------ the host layers
def test_host_layers_carry_the_objective(pkg):
    import ctypes as C
    B = pkg.binding
    assert (B.SCORE_AS_SOLVED, B.SCORE_POINT, B.SCORE_PLANE, B.SCORE_GICP) == (-1, 0, 1, 2)
    assert [f[0] for f in B.ScoreObjectiveStruct._fields_] == ["struct_size", "form", "max_corr_dist", "huber_delta", "epsilon"]
    assert C.sizeof(B.ScoreObjectiveStruct) == 40
    for name in ("svnicp_score_particles_objective", "svnicp_set_particle_weighting_objective", "svnicp_get_score_objective"):
        assert name in B.declared_symbols() and hasattr(B.load_library(), name)
    w = pkg.ParticleWeightOpt()
    assert w.weight_cost == "point" and pkg.ParticleWeightOpt(True, 0.3, 1e-3, "solved").weight_cost == "solved"
    sc = pkg.ParticleScores(*([np.zeros(1)] * 7))
    assert sc.form == "point" and sc.accepted is sc.plane_inliers and sc.sum_h is sc.sum_r2
    cfg = pkg.pipeline.PipelineConfig()
    assert cfg.weight_cost == "point"
    for bad in (dict(weight_cost="solved"), dict(weight_cost="gicp", weight_dist=0.3, weight_temperature=1.0)):
        with pytest.raises(ValueError):
            pkg.pipeline.PipelineConfig(**bad)
    assert pkg.pipeline.PipelineConfig(weight_dist=0.3, weight_temperature=1e-3, weight_cost="solved").weight_cost == "solved"
    shim = open(os.path.join(ROOT, "svn-icp_amd", "host", "svnicp_hip_shim.hpp")).read()
    for needle in ("weight_cost", "score_particles_objective", "set_particle_weighting_objective", "get_score_objective", "SVNICP_SCORE_AS_SOLVED"):
        assert needle in shim, needle
    host = open(os.path.join(ROOT, "svn-icp_amd", "host", "registration_pipeline.hpp")).read()
    assert "weight_cost" in host and "weight_cost" in open(os.path.join(ROOT, "svn-icp_amd", "host", "pipeline_drive.cpp")).read()


# ------------------------------------------------------------------------------------------------ the pair's arithmetic under the sanitizers
def test_pair_cost_driver_under_the_sanitizers(tmp_path):
    """tests/particle_score_objective_driver.cpp: gicp_pair_cost beside gicp_pair_sums on the host, compiled with the address and
    undefined-behaviour sanitizers the way tests/gicp_accum_driver.cpp is; the program checks itself."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "particle_score_objective_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-I", os.path.join(ROOT, "svn-icp_amd", "csrc"), os.path.join(ROOT, "tests", "particle_score_objective_driver.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok (0 findings)" in r.stdout and "adversarial pairs: 144 checked" in r.stdout


# ------------------------------------------------------------------------------------------------ the refusals, stated once
WEIGHTING = "svnicp_align: particle weighting (svnicp_set_particle_weighting) is not available here: "
PLANE_T = "form PLANE needs normals of the current target in the context (svnicp_set_target_normals, or a registration that estimated them)"
GICP_T = "form GICP needs normals of the current target in the context (svnicp_set_target_normals, or a registration that estimated them)"
GICP_S = ("form GICP needs normals of the current source in the context (svnicp_set_source_normals, or a registration in generalized-ICP mode "
          "that estimated them)")
LADDER_CASES = [   # (statements on the objective o / the base facts f, expression, expected text)
    ("o.gate = 0.3;", "msg(score_objective_refusal(o, 1e-6))", "-"),
    ("o.form = -1; o.gate = 0.3; o.delta = 1.0 / 0.0; o.eps = 1.0;", "msg(score_objective_refusal(o, 1e-6))", "-"),
    ("o.form = 2; o.gate = 0.3; o.eps = 1e-6;", "msg(score_objective_refusal(o, 1e-6))", "-"),
    ("o.form = 3; o.gate = 0.0;", "msg(score_objective_refusal(o, 1e-6))", "unknown form (SVNICP_SCORE_AS_SOLVED, _POINT, _PLANE or _GICP)"),
    ("o.form = -2; o.gate = 0.3;", "msg(score_objective_refusal(o, 1e-6))", "unknown form (SVNICP_SCORE_AS_SOLVED, _POINT, _PLANE or _GICP)"),
    ("o.gate = 0.0;", "msg(score_objective_refusal(o, 1e-6))", "max_corr_dist must be finite and positive"),
    ("o.gate = 1.0 / 0.0;", "msg(score_objective_refusal(o, 1e-6))", "max_corr_dist must be finite and positive"),
    ("o.gate = 0.0 / 0.0;", "msg(score_objective_refusal(o, 1e-6))", "max_corr_dist must be finite and positive"),
    ("o.gate = 0.3; o.delta = -0.1;", "msg(score_objective_refusal(o, 1e-6))", "huber_delta must be positive (+inf: no robust weight) or 0 (the solver's own)"),
    ("o.gate = 0.3; o.delta = 0.0 / 0.0;", "msg(score_objective_refusal(o, 1e-6))", "huber_delta must be positive (+inf: no robust weight) or 0 (the solver's own)"),
    ("o.gate = 0.3; o.eps = 2.0;", "msg(score_objective_refusal(o, 1e-6))", "epsilon must be 0 (the solver's own) or in [1e-6, 1]"),
    ("o.gate = 0.3; o.eps = 1e-7;", "msg(score_objective_refusal(o, 1e-6))", "epsilon must be 0 (the solver's own) or in [1e-6, 1]"),
    # resolution: form | delta | eps
    ("o.form = -1; o.gate = 0.3; o.delta = 9; o.eps = 0.5;", "show(resolve_score_objective(o, false, false, 0.1, 1e-3))", "0 0 0"),
    ("o.form = -1; o.gate = 0.3; o.delta = 9; o.eps = 0.5;", "show(resolve_score_objective(o, true, false, 0.1, 1e-3))", "1 0.1 0"),
    ("o.form = -1; o.gate = 0.3; o.delta = 9; o.eps = 0.5;", "show(resolve_score_objective(o, true, true, 0.1, 1e-3))", "2 0.1 0.001"),
    ("o.form = 1; o.gate = 0.3;", "show(resolve_score_objective(o, false, false, 0.1, 1e-3))", "1 0.1 0"),
    ("o.form = 2; o.gate = 0.3; o.delta = 0.05;", "show(resolve_score_objective(o, true, false, 0.1, 1e-3))", "2 0.05 0.001"),
    ("o.form = 2; o.gate = 0.3; o.delta = 0.05; o.eps = 0.25;", "show(resolve_score_objective(o, true, true, 0.1, 1e-3))", "2 0.05 0.25"),
    ("o.form = 0; o.gate = 0.3; o.delta = 0.05; o.eps = 0.25;", "show(resolve_score_objective(o, true, true, 0.1, 1e-3))", "0 0 0"),
    # the normals a resolved form reads
    ("", "msg(score_normals_refusal(0, false, false))", "-"),
    ("", "msg(score_normals_refusal(1, true, false))", "-"),
    ("", "msg(score_normals_refusal(2, true, true))", "-"),
    ("", "msg(score_normals_refusal(1, false, true))", PLANE_T),
    ("", "msg(score_normals_refusal(2, false, false))", GICP_T),
    ("", "msg(score_normals_refusal(2, true, false))", GICP_S),
    # … and the weighting's ladder carries them behind its own
    ("f.weighting = 1; f.weighting_form = 1;", "msg(weighting_refusal(f, t), kWeightingRefusal)", WEIGHTING + PLANE_T),
    ("f.weighting = 1; f.weighting_form = 1; f.target_normals = true;", "msg(weighting_refusal(f, t), kWeightingRefusal)", "-"),
    ("f.weighting = 1; f.weighting_form = 2; f.target_normals = true;", "msg(weighting_refusal(f, t), kWeightingRefusal)", WEIGHTING + GICP_S),
    ("f.weighting = 1; f.weighting_form = 2; f.svgd = true;", "msg(weighting_refusal(f, t), kWeightingRefusal)",
     WEIGHTING + "SVGD mode: the weight option belongs to SVNICP's constructor only"),
    ("f.weighting = 0; f.weighting_form = 2;", "msg(weighting_refusal(f, t), kWeightingRefusal)", "-"),
]
PROBE = r"""
#include <cstdio>
#include <string>
#include "registration_plan.hpp"
using namespace svnicp;
static RegistrationFacts base() { RegistrationFacts f; f.P = 16; f.p_lo = 0; f.p_hi = 16; f.K = 100; f.I = 12; f.B = 1100; f.M = 20000; return f; }
static std::string msg(const char* why, const char* prefix = "") { return why ? std::string(prefix) + why : std::string("-"); }
static std::string show(const ScoreObjective& o) { char b[96]; std::snprintf(b, sizeof b, "%d %g %g", o.form, o.delta, o.eps); return b; }
int main() {
@CASES@
  return 0;
}
"""


def test_objective_refusals_and_resolution_compiled_on_the_host(tmp_path):
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    body = "\n".join('  { RegistrationFacts f = base(); Tuning t; ScoreObjective o; (void)f; (void)t; (void)o; %s std::printf("%%s\\n", std::string(%s).c_str()); }'
                     % (setup, expr) for setup, expr, _ in LADDER_CASES)
    src = tmp_path / "probe.cpp"
    src.write_text(PROBE.replace("@CASES@", body))
    exe = tmp_path / "probe"
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-Wno-div-by-zero", "-I", os.path.join(ROOT, "svn-icp_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).splitlines()
    assert len(out) == len(LADDER_CASES)
    for (setup, expr, want), got in zip(LADDER_CASES, out):
        assert got == want, (setup, expr)
