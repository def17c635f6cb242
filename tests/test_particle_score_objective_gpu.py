"""Score and weight the particles in the plane and generalized-ICP objectives (csrc/particle_score.hip)
against tests/particle_score_objective_reference.py, the numpy restatement of include/svnicp_hip.h "score and weight the
particles in the objective the solver minimised".  The clouds are those of tests/particle_score_cases.py (300 source, 3000 target
points); the restatement is fed the device's own candidates, the normals the context holds and the poses the scoring returned.

Tolerances, as in tests/test_particle_score_gpu.py and for its reason: the three counts are exact (every case checks on the returned
poses that no pair sits within 1e-12 of the gate or of its runner-up; h is continuous, so delta needs no precondition); d2, r,
rho2 and h are the same unfused float64 expressions on both sides, the sums differ by the order of 300 additions and the cost by
that of its sum: TIGHT = 1e-9 relative.  The weights are one exp and one division away from the restatement applied to the
returned costs (1e-12), the weighted statistics follow within 1e-12 * max|pose|."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from helpers import TIGHT

import nonfinite_reference as nf
import particle_score_cases as pc
import particle_score_objective_cases as oc
import particle_score_objective_reference as po
import particle_score_reference as ps
import plane_reference as pr

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
INF = float("inf")
FORM_ID = {"point": po.POINT, "plane": po.PLANE, "gicp": po.GICP}
_CLOUDS = {}


def _clouds(hip, orc, name):
    """(source, target, target normals, source normals with a tenth of the rows zeroed) of a shared cloud: once per session."""
    if name not in _CLOUDS:
        src, tgt = pc.clouds(hip, name)
        _CLOUDS[name] = (src, tgt, pr.normals(orc, tgt, 16)[0], oc.source_normals(orc, src, name))
    return _CLOUDS[name]


def _solver(hip, src, tgt, P, K, residual="point", iterations=3, svgd=False, weight=None, nt=None, ns=None, delta=oc.SOLVER_DELTA,
            eps=oc.EPS, prior=None, **kw):
    """prior=None: the cases' pose prior in plane and GICP mode (particle_score_objective_cases.PRIOR_LAMBDA says why), none in point mode."""
    init = pc.particles(hip, P)
    prm = hip.SteinICPParam(iterations=iterations, lr=pc.LR, max_dist=1.0, KNN_count=K, SVN_full_grad=False, residual=residual,
                            huber_delta=delta, gicp_epsilon=eps, **kw)
    s = (hip.SVGDICP if svgd else hip.SVNICP)(prm, init, weight or hip.ParticleWeightOpt())
    s.add_cloud(src, tgt, init)
    s.set_initial_mean(pc.initial_mean(hip))
    _normals(s, nt, ns)
    if residual != "point" if prior is None else prior:
        s.set_pose_prior(oc.PRIOR_MEAN, oc.PRIOR_LAMBDA)
    return s


def _normals(s, nt, ns):
    if nt is not None:
        s.set_target_normals(nt)
    if ns is not None:
        s.set_source_normals(ns)


def _registered(hip, *a, **kw):
    s = _solver(hip, *a, **kw)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    return s


def _fields(sc):
    return np.stack([sc.evaluated, sc.inliers, sc.accepted, sc.sum_d2, sc.sum_h, sc.cost], axis=1).astype(np.float64)


def _poses12(sc):
    return np.concatenate([sc.poses[:, :, :3].reshape(-1, 9), sc.poses[:, :, 3]], axis=1)


def _want(s, form, src, tgt, got, gate, delta, eps=oc.EPS, pairs=None):
    """The restatement at the returned poses, on what the context holds."""
    ns = s.get_source_normals() if form == "gicp" else None
    return po.score(FORM_ID[form], src, tgt, s.get_candidates(), _poses12(got), gate, normals=s.get_target_normals(), src_normals=ns,
                    delta=delta, eps=eps, pr=pairs)


def _check(got, want, label, pairs=None, gate=None):
    g = _fields(got)
    rel = [np.abs(g[:, i] - want[:, i]).max() / max(np.abs(want[:, i]).max(), 1e-300) for i in (3, 4, 5)]
    print(f"{label}: evaluated {g[:, 0].min():.0f}..{g[:, 0].max():.0f} inliers {g[:, 1].min():.0f}..{g[:, 1].max():.0f} accepted "
          f"{g[:, 2].min():.0f}..{g[:, 2].max():.0f} | max rel diff sum_d2 {rel[0]:.3e} sum_h {rel[1]:.3e} cost {rel[2]:.3e}")
    if pairs is not None:
        near_gate, tie = ps.preconditions(pairs, gate)
        assert near_gate.size == 0 and tie.size == 0, label
    assert not np.isnan(g).any(), label
    assert np.array_equal(g[:, :3], want[:, :3]), label
    assert np.allclose(g[:, 3:], want[:, 3:], rtol=TIGHT, atol=0), label


def _score_all(s, form, src, tgt, label, solver_form=None):
    """Both gates x both deltas of one form on one registration, each against the restatement; where delta is the solver's and the
    registration ran in this form, "solved" must give the explicit form's bits."""
    eps = oc.EPS if form == "gicp" else None
    pairs, out = None, {}
    for gate in oc.GATES:
        for delta in oc.DELTAS:
            got = s.score_particles(gate, form=form, huber_delta=delta, gicp_epsilon=eps)
            assert got.form == form and got.max_corr_dist == gate and got.huber_delta == delta and got.gicp_epsilon == (oc.EPS if form == "gicp" else 0.0)
            assert got.poses.shape[1:] == (3, 4) and np.isfinite(got.poses).all()
            if pairs is None:
                pairs = ps.pairs(src, tgt, s.get_candidates(), _poses12(got))
            _check(got, _want(s, form, src, tgt, got, gate, delta, pairs=pairs), f"{label} form {form} gate {gate} delta {delta}", pairs, gate)
            again = s.get_particle_scores()
            assert _fields(again).tobytes() == _fields(got).tobytes() and again.poses.tobytes() == got.poses.tobytes() and again.form == form
            if solver_form == form and delta == oc.SOLVER_DELTA:
                solved = s.score_particles(gate, form="solved")
                assert solved.form == form and solved.huber_delta == oc.SOLVER_DELTA and solved.gicp_epsilon == got.gicp_epsilon
                assert _fields(solved).tobytes() == _fields(got).tobytes() and solved.poses.tobytes() == got.poses.tobytes()
            out[gate, delta] = got
    return out


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("form", oc.FORMS)
@pytest.mark.parametrize("K", oc.KS)
@pytest.mark.parametrize("P", oc.PS)
def test_objective_scores_agree_with_the_restatement(hip, orc, P, K, form):
    """Every particle geometry against every K the two modes accept, after a registration in the mode whose form is scored;
    B = 300 = 4 * 64 + 44 rows: a partial workgroup and a partial tile.  A tenth of the source rows have no normal."""
    cloud = oc.cloud_of(P, K, form)
    src, tgt, nt, ns = _clouds(hip, orc, cloud)
    I = oc.iterations_of(P, K)
    s = _registered(hip, src, tgt, P, K, residual=form, iterations=I, nt=nt, ns=ns)
    got = _score_all(s, form, src, tgt, f"{cloud} P {P} K {K} I {I}", solver_form=form)
    for sc in got.values():
        assert (sc.evaluated == pc.B_).all() and (sc.accepted > 0).all() and (sc.accepted <= sc.inliers).all()
    if form == "gicp":    # the zeroed source rows: fewer pairs than the plane form accepts at the same poses
        plane = s.score_particles(oc.GATES[0], form="plane", huber_delta=INF)
        assert (got[oc.GATES[0], INF].accepted < plane.accepted).all()


@pytest.mark.parametrize("P", oc.K150_PS)
def test_objective_scores_with_lower_tiles(hip, orc, P):
    """K = 150: tiles lower than the workgroup's row slots and the seeded scan.  The plane and GICP residuals refuse K > 128, so
    the registration runs in point mode; the normals come afterwards and the forms are the caller's choice."""
    src, tgt, nt, ns = _clouds(hip, orc, "sheets")
    s = _registered(hip, src, tgt, P, 150)
    _normals(s, nt, ns)
    for form in oc.FORMS:
        _score_all(s, form, src, tgt, f"sheets P {P} K 150 after a point-mode registration")


@pytest.mark.parametrize("B,M", [(1, 1), (70, 64)])
def test_objective_score_edges(hip, B, M):
    src, tgt = hip.scans.random_clouds(B, M, seed=7)
    nt, ns = oc.random_unit_normals(M, 21, 0.0 if M == 1 else 0.1), oc.random_unit_normals(B, 22, 0.0 if B == 1 else 0.1)
    for P, K in ((4, 16), (9, 1)):
        s = _registered(hip, src, tgt, P, K)
        _normals(s, nt, ns)
        for form in oc.FORMS:
            for delta in oc.DELTAS:
                got = s.score_particles(1.0, form=form, huber_delta=delta, gicp_epsilon=oc.EPS if form == "gicp" else None)
                _check(got, _want(s, form, src, tgt, got, 1.0, delta), f"B {B} M {M} P {P} K {K} form {form} delta {delta}")
                assert (got.evaluated == B).all()


# ------------------------------------------------------------------------------------------------ 2. what is bitwise the point scoring
@pytest.mark.parametrize("P,K", [(4, 16), (130, 128), (64, 150)])
def test_plane_form_without_robust_weight_is_the_point_scoring_bit_for_bit(hip, orc, P, K):
    src, tgt, nt, _ = _clouds(hip, orc, "random")
    s = _registered(hip, src, tgt, P, K)
    s.set_target_normals(nt)
    for gate in oc.GATES:
        point = s.score_particles(gate)
        assert point.form == "point" and point.huber_delta == 0.0
        plane = s.score_particles(gate, form="plane", huber_delta=INF)
        assert (plane.accepted > 0).all()
        assert _fields(plane)[:, :5].tobytes() == _fields(point)[:, :5].tobytes()


@pytest.mark.parametrize("normals", [False, True])
def test_solved_after_a_point_registration_is_score_particles(hip, orc, normals):
    src, tgt, nt, ns = _clouds(hip, orc, "sheets")
    s = _registered(hip, src, tgt, 25, 16)
    if normals:
        _normals(s, nt, ns)
    for gate in oc.GATES:
        point = s.score_particles(gate)
        solved = s.score_particles(gate, form="solved")
        assert solved.form == "point" and solved.huber_delta == 0.0 and solved.gicp_epsilon == 0.0 and solved.max_corr_dist == gate
        assert _fields(solved).tobytes() == _fields(point).tobytes() and solved.poses.tobytes() == point.poses.tobytes()
        explicit = s.score_particles(gate, form="point", huber_delta=0.1)      # checked, not used
        assert _fields(explicit).tobytes() == _fields(point).tobytes()


# ------------------------------------------------------------------------------------------------ 3. non-finite rows
@pytest.mark.parametrize("nan_target_0", [False, True])
def test_objective_score_with_nonfinite_and_huge_rows(hip, orc, nan_target_0):
    """The rows of tests/test_particle_score_gpu.py's case: a NaN source row, a 1e160 source row, NaN / inf target rows and a NaN
    target row 0, after a plane-mode registration (the context then holds estimated target normals); the source normals are
    supplied.  No NaN in any field, the counts as in the restatement."""
    src, tgt, _, ns = _clouds(hip, orc, "random")
    src_rows, tgt_rows = [3, 64, 65, 299], [5, 511, 2999]
    src_b, tgt_b = nf.poison(src, src_rows, ("nan1", "big64", "nan3", "big64")), nf.poison(tgt, tgt_rows, ("nan1", "+inf", "nan3"))
    if nan_target_0:
        tgt_b = nf.poison(tgt_b, [0], "nan1")
    s = _registered(hip, src_b, tgt_b, 9, 16, residual="plane", delta=0.1, prior=False)   # that test's registration
    s.set_source_normals(ns)
    for form in oc.FORMS:
        for gate in oc.GATES:
            for delta in oc.DELTAS:
                got = s.score_particles(gate, form=form, huber_delta=delta, gicp_epsilon=oc.EPS if form == "gicp" else None)
                assert np.isfinite(got.poses).all()
                _check(got, _want(s, form, src_b, tgt_b, got, gate, delta), f"non-finite target0 {nan_target_0} form {form} gate {gate} delta {delta}")
                assert (got.evaluated == len(src) - 2).all() and (got.inliers <= len(src) - 4).all() and (got.inliers > 0).all()
                assert (got.accepted > 0).all() or form == "gicp"
                assert np.isfinite(_fields(got)).all()


# ------------------------------------------------------------------------------------------------ 4. weights
def _weighted(hip, orc, cloud, temperature, residual="gicp", cost="solved", K=pc.WEIGHT_K, **kw):
    src, tgt, nt, ns = _clouds(hip, orc, cloud)
    w = hip.ParticleWeightOpt(True, pc.WEIGHT_GATE, temperature, cost)
    return _registered(hip, src, tgt, pc.WEIGHT_P, K, residual=residual, weight=w, nt=nt, ns=ns, **kw)


@pytest.mark.parametrize("cloud", pc.CLOUDS)
def test_weights_follow_the_objective_cost(hip, orc, cloud):
    src, tgt, _, _ = _clouds(hip, orc, cloud)
    s = _weighted(hip, orc, cloud, pc.WEIGHT_T)
    sc = s.get_particle_scores()                                  # the registration's own scoring, no further GPU work
    assert sc.form == "gicp" and sc.max_corr_dist == pc.WEIGHT_GATE and sc.huber_delta == oc.SOLVER_DELTA and sc.gicp_epsilon == oc.EPS
    _check(sc, _want(s, "gicp", src, tgt, sc, pc.WEIGHT_GATE, oc.SOLVER_DELTA), f"{cloud} weighted GICP registration")
    w = s.get_particle_weight()
    want_w = ps.weights(sc.cost, pc.WEIGHT_T)
    print(f"{cloud}: weights {w.min():.3e}..{w.max():.3e} sum - 1 = {w.sum() - 1.0:.3e} max rel diff {np.abs(w / want_w - 1).max():.3e}")
    assert np.allclose(w, want_w, rtol=1e-12, atol=0) and abs(w.sum() - 1.0) <= 1e-12
    x = s.get_particles()
    mean, var, cov = ps.weighted_stats(x, w)
    tol = 1e-12 * np.abs(x).max()
    got = (s.get_transformation(), s.get_distribution(), s.get_cov_matrix())
    print(f"{cloud}: |mean| {np.abs(got[0] - mean).max():.3e} |var| {np.abs(got[1] - var).max():.3e} |cov| {np.abs(got[2] - cov.reshape(36)).max():.3e} tol {tol:.3e}")
    assert np.abs(got[0] - mean).max() <= tol and np.abs(got[1] - var).max() <= tol and np.abs(got[2] - cov.reshape(36)).max() <= tol
    # a scoring by hand in the same objective gives the registration's scores bit for bit; the point cost is another
    assert _fields(s.score_particles(pc.WEIGHT_GATE, form="solved")).tobytes() == _fields(sc).tobytes()
    assert _fields(s.score_particles(pc.WEIGHT_GATE)).tobytes() != _fields(sc).tobytes()
    assert np.array_equal(s.get_particle_weight(), w)            # scoring changes no result
    # the same through the setter on a plane-mode context: "solved" resolves at svnicp_align_begin, to the plane form there
    p = _weighted(hip, orc, cloud, pc.WEIGHT_T, residual="plane")
    psc = p.get_particle_scores()
    assert psc.form == "plane" and psc.huber_delta == oc.SOLVER_DELTA and psc.gicp_epsilon == 0.0
    _check(psc, _want(p, "plane", src, tgt, psc, pc.WEIGHT_GATE, oc.SOLVER_DELTA), f"{cloud} weighted plane registration")
    assert np.allclose(p.get_particle_weight(), ps.weights(psc.cost, pc.WEIGHT_T), rtol=1e-12, atol=0)


_ARGMIN = {}


@pytest.mark.parametrize("cloud,K", oc.WEIGHT_CASES)
def test_cold_weights_pick_the_best_particle_of_the_objective(hip, orc, cloud, K):
    s = _weighted(hip, orc, cloud, pc.COLD_T, K=K)
    cost = s.get_particle_scores().cost
    order = np.argsort(cost)
    print(f"{cloud}: best GICP cost {cost[order[0]]!r}, second {cost[order[1]]!r}")
    assert cost[order[1]] - cost[order[0]] >= 1e-6
    w, x = s.get_particle_weight(), s.get_particles().reshape(6, -1)
    assert w[order[0]] == 1.0 and np.count_nonzero(w) == 1
    assert np.array_equal(s.get_transformation(), x[:, order[0]])
    modes = s.particle_modes(10.0, 10.0)                          # one mode of all particles: its best is the argmin
    assert modes.has_scores and modes.n_modes == 1 and int(modes.best[0]) == order[0] and modes.cost_min[0] == cost[order[0]]
    point = s.score_particles(pc.WEIGHT_GATE).cost
    print(f"{cloud}: argmin under the GICP cost {order[0]}, under the point cost {int(np.argmin(point))}")
    _ARGMIN[cloud, K] = (int(order[0]), int(np.argmin(point)))


def test_the_objective_ranks_differently_from_the_point_cost(hip, orc):
    """On the sheet-dominated cloud the particle the GICP cost ranks first is not the one the point cost does (the case is recorded
    in tests/particle_score_objective_cases.py, chosen on the restatement: tests/test_particle_score_objective_cpu.py)."""
    case = oc.RANKS_DIFFERENTLY
    if case not in _ARGMIN:
        test_cold_weights_pick_the_best_particle_of_the_objective(hip, orc, *case)
    print(f"{case}: argmin under the GICP cost {_ARGMIN[case][0]}, under the point cost {_ARGMIN[case][1]}; recorded {oc.ARGMIN[case]}")
    assert _ARGMIN[case] == oc.ARGMIN[case] and _ARGMIN[case][0] != _ARGMIN[case][1]


# ------------------------------------------------------------------------------------------------ 5. isolation
def _snapshot(s):
    d = dict(transformation=s.get_transformation(), distribution=s.get_distribution(), cov=s.get_cov_matrix(),
             particles=s.get_particles(), weights=s.get_particle_weight(), history=s.get_particle_history(),
             candidates=s.get_candidates(), cand_d2=s.get_candidate_dist2(), fallbacks=np.array(s.get_knn_fallbacks()),
             ambiguous=np.array(s.get_ambiguous_pairs()), iterations=np.array(s.get_iterations_run()))
    for k, v in s.get_trace().items():
        d["trace_" + k] = v
    return d


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


@pytest.mark.parametrize("P,K,residual", [(16, 16, "gicp"), (130, 128, "plane")])
def test_objective_scoring_and_weighting_change_nothing_else(hip, orc, P, K, residual):
    """The snapshot pattern of test_uniform_weighting_changes_nothing: after objective scoring and weighting, then back to uniform,
    a registration is bitwise that of a fresh context; a following svnicp_set_particle_weighting restores the point cost bitwise."""
    src, tgt, nt, ns = _clouds(hip, orc, "random")
    kw = dict(record_trace=True, residual=residual, nt=nt, ns=ns)

    def again(s):
        s.add_cloud(src, tgt, pc.particles(hip, P))
        _normals(s, nt, ns)
        assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
        return _snapshot(s)

    f = _registered(hip, src, tgt, P, K, **kw)                    # the context that never sets, scores or weights
    fresh = _snapshot(f)
    s = _solver(hip, src, tgt, P, K, **kw)                        # set and reset
    s.set_particle_weighting("softmin", 0.3, 1e-3, cost="solved")
    s.set_particle_weighting("uniform", cost="solved")
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    _same(fresh, _snapshot(s))
    s.set_particle_weighting("softmin", 0.3, 1e-3, cost="solved")  # a weighted registration …
    weighted, fresh = again(s), again(f)
    assert weighted["weights"].tobytes() != fresh["weights"].tobytes() and s.get_particle_scores().form == residual
    for k in ("particles", "history", "candidates", "cand_d2", "trace_H", "trace_corr", "iterations"):   # the iterations do not see the weights
        assert weighted[k].tobytes() == fresh[k].tobytes(), k
    s.set_particle_weighting("uniform")                           # … and the uniform one after it
    _same(again(f), again(s))
    fresh = _snapshot(f)
    one = s.score_particles(0.3, form="solved")                   # after a scoring: nothing a getter returns has changed …
    _same(fresh, _snapshot(s))
    two = s.score_particles(0.3, form=residual, huber_delta=oc.SOLVER_DELTA, gicp_epsilon=oc.EPS if residual == "gicp" else None)
    assert _fields(one).tobytes() == _fields(two).tobytes() and one.poses.tobytes() == two.poses.tobytes()
    _same(again(f), again(s))                                     # … and the next registration is that of the untouched context
    # the point weighting after the objective weighting is the point weighting of a context that never knew the other
    s.set_particle_weighting("softmin", 0.3, 1e-3, cost="solved")
    s.set_particle_weighting("softmin", 0.3, 1e-3)
    f.set_particle_weighting("softmin", 0.3, 1e-3)
    a, b = again(s), again(f)
    _same(a, b)
    assert a["weights"].tobytes() != fresh["weights"].tobytes()
    assert s.get_particle_scores().form == "point" and _fields(s.get_particle_scores()).tobytes() == _fields(f.get_particle_scores()).tobytes()


# ------------------------------------------------------------------------------------------------ 6. refusals
def _err(s):
    return s._L.svnicp_last_error(s.handle).decode()


def _raw_score(s, form, gate=0.3, delta=0.0, eps=0.0, size=None):
    obj = hip_binding(s).ScoreObjectiveStruct(C.sizeof(hip_binding(s).ScoreObjectiveStruct) if size is None else size, form, gate, delta, eps)
    out = np.zeros((s._P, 6))
    return s._L.svnicp_score_particles_objective(s.handle, C.byref(obj), out.ctypes.data_as(C.POINTER(C.c_double)), None)


def hip_binding(s):
    import sys
    return sys.modules[type(s).__module__].binding


def test_objective_scoring_refusals(hip, orc):
    src, tgt, nt, ns = _clouds(hip, orc, "random")
    P, K = 16, 16
    s = _solver(hip, src, tgt, P, K)
    assert _raw_score(s, po.PLANE) == ERR_INVALID and "no finished registration" in _err(s)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    assert _raw_score(s, po.PLANE) == ERR_INVALID and "form PLANE needs normals of the current target" in _err(s)
    assert _raw_score(s, po.GICP) == ERR_INVALID and "form GICP needs normals of the current target" in _err(s)
    s.set_target_normals(nt)
    assert _raw_score(s, po.PLANE, delta=INF) == 0
    assert _raw_score(s, po.GICP) == ERR_INVALID and "form GICP needs normals of the current source" in _err(s)
    s.set_source_normals(ns)
    assert _raw_score(s, po.GICP) == 0
    assert _raw_score(s, po.GICP, size=8) == ERR_INVALID and "struct_size mismatch" in _err(s)
    assert s._L.svnicp_score_particles_objective(s.handle, None, None, None) == ERR_INVALID and "null svnicp_score_objective" in _err(s)
    for form in (-2, 3, 7):
        assert _raw_score(s, form) == ERR_INVALID and "unknown form" in _err(s), form
    for gate in (0.0, -1.0, float("nan"), INF):
        for form in (-1, 0, 1, 2):
            assert _raw_score(s, form, gate=gate) == ERR_INVALID and "max_corr_dist must be finite and positive" in _err(s), (form, gate)
    for delta in (-0.1, float("nan"), -INF):
        assert _raw_score(s, po.PLANE, delta=delta) == ERR_INVALID and "huber_delta" in _err(s), delta
    for eps in (2.0, 1e-9, -1e-3, float("nan")):
        assert _raw_score(s, po.GICP, eps=eps) == ERR_INVALID and "epsilon" in _err(s), eps
    # the refusals of svnicp_score_particles, word for word
    s.set_k(K)
    assert _raw_score(s, po.GICP) == ERR_INVALID and "register again" in _err(s)
    s.set_option("correspondence", "full")
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    assert _raw_score(s, po.GICP) == ERR_INVALID and "correspondence=full" in _err(s)
    s.set_option("correspondence", "fast")
    s.set_minibatch(64, 1)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    assert _raw_score(s, po.AS_SOLVED) == ERR_INVALID and "mini-batch" in _err(s)
    s.set_minibatch(0)
    # the refused context stays usable
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    got = s.score_particles(0.3, form="gicp", huber_delta=0.05, gicp_epsilon=1e-3)
    _check(got, _want(s, "gicp", src, tgt, got, 0.3, 0.05), "after the refusals")
    # before any scoring there is no objective to return
    t = _solver(hip, src, tgt, P, K)
    obj = hip_binding(t).ScoreObjectiveStruct(C.sizeof(hip_binding(t).ScoreObjectiveStruct))
    assert t._L.svnicp_get_score_objective(t.handle, C.byref(obj)) == ERR_INVALID and "no scoring yet" in _err(t)


def test_objective_weighting_refusals(hip, orc):
    src, tgt, nt, ns = _clouds(hip, orc, "random")
    P, K = 16, 16

    def refused(s, needle):
        rc = s._L.svnicp_align_begin(s.handle)
        assert rc == ERR_INVALID and "particle weighting" in _err(s) and needle in _err(s), (rc, _err(s))

    def setter(s, kind, form, gate=0.3, delta=0.0, eps=0.0, T=1e-3):
        B = hip_binding(s)
        obj = B.ScoreObjectiveStruct(C.sizeof(B.ScoreObjectiveStruct), form, gate, delta, eps)
        return s._L.svnicp_set_particle_weighting_objective(s.handle, kind, C.byref(obj), T)

    g = _solver(hip, src, tgt, P, K, svgd=True)
    g.set_particle_weighting("softmin", 0.3, 1e-3, cost="solved")
    refused(g, "SVGD")
    s = _solver(hip, src, tgt, P, K)
    assert setter(s, 1, 5) == ERR_INVALID and "unknown form" in _err(s)
    assert setter(s, 1, -1, gate=0.0) == ERR_INVALID and "max_corr_dist" in _err(s)
    assert setter(s, 1, 1, delta=-1.0) == ERR_INVALID and "huber_delta" in _err(s)
    assert setter(s, 1, 2, eps=3.0) == ERR_INVALID and "epsilon" in _err(s)
    for T in (0.0, -1.0, float("nan"), INF):
        assert setter(s, 1, -1, T=T) == ERR_INVALID and "temperature" in _err(s), T
    assert setter(s, 2, -1) == 0
    refused(s, "unknown weighting kind")
    # a form whose normals neither the context holds nor this registration estimates: refused before anything runs
    assert setter(s, 1, po.PLANE) == 0
    refused(s, "form PLANE needs normals of the current target")
    s.set_target_normals(nt)
    assert setter(s, 1, po.GICP) == 0
    refused(s, "form GICP needs normals of the current source")
    s.set_source_normals(ns)
    assert setter(s, 1, -1) == 0
    assert s._L.svnicp_set_shard(s.handle, 0, 8) == 0
    refused(s, "particle shard")
    assert s._L.svnicp_set_shard(s.handle, 0, P) == 0
    assert s._L.svnicp_set_row_shard(s.handle, 0, 2, 2 * len(src)) == 0
    refused(s, "row shard")
    assert s._L.svnicp_set_row_shard(s.handle, 0, 1, 0) == 0
    s.set_minibatch(64, 1)
    refused(s, "mini-batch")
    s.set_minibatch(0)
    s.set_option("correspondence", "full")
    refused(s, "correspondence=full")
    s.set_option("correspondence", "fast")
    # the refused context stays usable: point mode, so "solved" is the point cost of svnicp_set_particle_weighting
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    fresh = _registered(hip, src, tgt, P, K, weight=hip.ParticleWeightOpt(True, 0.3, 1e-3), nt=nt, ns=ns)
    assert np.array_equal(s.get_particle_weight(), fresh.get_particle_weight()) and s.get_particle_scores().form == "point"
    assert _fields(s.get_particle_scores()).tobytes() == _fields(fresh.get_particle_scores()).tobytes()


# ------------------------------------------------------------------------------------------------ 7. the pipelines
def test_pipelines_weight_in_the_solved_objective(hip, tmp_path):
    """weight_cost="solved" with the GICP residual on the synthetic drive of tests/test_pipeline_gpu.py: the C++ and the Python
    pipeline agree to 1e-9 in pose, and the weighted poses stay within 1e-3 of the unweighted run.  As in
    test_pipeline_with_weighted_particles the temperature makes that bound follow from the contract: the costs lie in [0, cap],
    cap = h(gate) = delta (2 gate - delta) = 0.09 m^2 at gate 0.5 m and the solver's delta 0.1 m, so with A = cap / temperature
    sum |w_p - 1/P| <= e^A - 1 and a coordinate of the mean moves by at most (e^A - 1) R, R = 0.6 m the width of the prior."""
    from test_pipeline_gpu import _build_pipeline_drive
    pl, sc = hip.pipeline, hip.scans
    root = os.path.dirname(os.path.dirname(hip.library_path()))
    exe = _build_pipeline_drive(root)
    P, I, K, voxel, n_scans = 24, 12, 40, 0.5, 4
    gate, temperature, delta = 0.5, 400.0, 0.1
    cap = po.cap(gate, delta)
    assert cap == delta * (2 * gate - delta) and np.expm1(cap / temperature) * 0.6 <= 5e-4
    scene = sc.make_scene()
    rng = np.random.default_rng(11)
    scans, parts = [], []
    for k in range(n_scans):
        t = np.array([0.0, 0.0, 0.05 * k]); R = sc.rot_zyx(0.0, 0.0, np.radians(0.3 * k))
        scans.append((0.1 * k, sc.lidar_scan(scene, R, t, 16384, stream=700 + k).astype(np.float32)))
        parts.append(hip.initialize_particles(P, pl.PRIOR_UB, pl.PRIOR_LB, rng))
    with open(tmp_path / "scans.bin", "wb") as f:
        f.write(struct.pack("<i", n_scans))
        for stamp, pts in scans:
            f.write(struct.pack("<di", stamp, pts.shape[0])); f.write(np.ascontiguousarray(pts[:, :3], np.float32).tobytes())
    with open(tmp_path / "particles.bin", "wb") as f:
        for p in parts:
            f.write(np.ascontiguousarray(p, np.float64).tobytes())
    # gpu_map 1, deskew 0, segment 0, map_normals 2 (GICP), eval 0, information off, modes off, clear 0, no seed grid, no prior, the weights
    args = ["1", "0", "0", "2", "0", "off", "off", "0", "0", "0"] + ["0"] * 7 + ["0"] * 7 + [str(gate), str(temperature), "solved"]
    r = subprocess.run([exe, str(tmp_path / "scans.bin"), str(tmp_path / "out.bin"), str(P), str(I), str(K), str(voxel),
                        str(tmp_path / "particles.bin")] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    off = 0

    def take(dtype, n):
        nonlocal off
        a = np.frombuffer(raw, dtype, n, off); off += a.nbytes
        return a
    cpp = []
    for k in range(n_scans):
        aligned = int(take("<i4", 1)[0])
        pose = take("<f8", 12)
        take("<f8", 12 + 6 + 6 + 36)
        B, M = (int(v) for v in take("<i8", 2))
        take("<f8", 3 * B + 3 * M + 6 * P)
        if aligned:
            take("<i8", 1)
        T = np.eye(4); T[:3, :3] = pose[:9].reshape(3, 3); T[:3, 3] = pose[9:]
        cpp.append(T)
    assert off == len(raw)
    runs = {}
    for name, kw in (("uniform", {}), ("solved", dict(weight_dist=gate, weight_temperature=temperature, weight_cost="solved"))):
        cfg = pl.PipelineConfig(min_range=1.0, max_range=80.0, voxel_size=voxel, map_voxel_size=voxel, map_voxel_max_points=20,
                                map_range=100.0, particle_count=P, gpu_map=True, map_normals=True,
                                solver=hip.SteinICPParam(iterations=I, lr=1.0, max_dist=1.0, KNN_count=K, SVN_full_grad=False,
                                                         residual="gicp", huber_delta=delta), **kw)
        pipe = pl.RegistrationPipeline(cfg, device=0)
        it = iter(parts)
        pipe._particles = lambda it=it: next(it)
        runs[name] = [pipe.process_scan(pts, stamp) for stamp, pts in scans]
        if name == "solved":
            o = pipe._solver.get_score_objective()
            assert (o.form, o.max_corr_dist, o.huber_delta, o.epsilon) == (po.GICP, gate, delta, 1e-3)
    uniform = np.float64(np.float32(1.0) / np.float32(P))
    for k in range(n_scans):
        u, w = runs["uniform"][k], runs["solved"][k]
        assert np.allclose(w.pose, cpp[k], rtol=0, atol=1e-9), k
        if k == 0:
            continue
        assert w.state == int(hip.SteinICPState.ALIGN_SUCCESS)
        assert abs(w.weights.sum() - 1.0) <= 1e-12 and (w.weights >= 0).all() and not np.array_equal(w.weights, u.weights)
        assert np.array_equal(u.weights, np.full(P, uniform))
        print(f"scan {k}: |pose - unweighted pose| = {np.abs(w.pose - u.pose).max():.3e} (weights {w.weights.min():.6e}..{w.weights.max():.6e})")
        assert np.abs(w.pose - u.pose).max() <= 1e-3
    with pytest.raises(ValueError, match="weight_cost"):
        pl.PipelineConfig(weight_cost="solved")
    with pytest.raises(ValueError, match="weight_cost"):
        pl.PipelineConfig(weight_dist=0.3, weight_temperature=1.0, weight_cost="plane")
