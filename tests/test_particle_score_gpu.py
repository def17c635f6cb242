"""Score and weight the particles on the device (csrc/particle_score.hip) against
tests/particle_score_reference.py, the numpy restatement of include/svnicp_hip.h "score and weight the particles".  The clouds
are 300 source and 3000 target points (tests/particle_score_cases.py); the restatement is fed the device's own candidates
(svnicp_get_candidates) and the poses the scoring returned.

Tolerances: the three counts are exact (tests/test_particle_score_cpu.py checks on the oracle's poses, and every case here on
the returned ones, that no pair sits within 1e-12 of a gate or of its runner-up); d2 and r are the same unfused float64
expressions on both sides, the sums differ by the order of 300 additions and the cost by that of its sum: TIGHT = 1e-9
relative.  The weights are one exp and one division away from the restatement applied to the returned costs (1e-12), and the
weighted statistics follow from get_particles() and get_particle_weight() within 1e-12 * max|pose|."""
import ctypes as C

import numpy as np
import pytest

from conftest import so3_exp_np
from helpers import TIGHT

import nonfinite_reference as nf
import particle_score_cases as pc
import particle_score_reference as ps
import plane_reference as pr

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
_CASES = {}


def _case(hip, orc, name):
    """(source, target, unit normals of the target) of a shared cloud: computed once per session."""
    if name not in _CASES:
        src, tgt = pc.clouds(hip, name)
        _CASES[name] = (src, tgt, pr.normals(orc, tgt, 16)[0])
    return _CASES[name]


def _solver(hip, src, tgt, P, K, iterations=3, svgd=False, weight=None, options=(), T0=None, init=None, **kw):
    init = pc.particles(hip, P) if init is None else init
    prm = hip.SteinICPParam(iterations=iterations, lr=pc.LR, max_dist=1.0, KNN_count=K, SVN_full_grad=False, **kw)
    s = (hip.SVGDICP if svgd else hip.SVNICP)(prm, init, weight or hip.ParticleWeightOpt())
    for name, value in options:
        s.set_option(name, value)
    s.add_cloud(src, tgt, init)
    s.set_initial_mean(pc.initial_mean(hip) if T0 is None else T0)
    return s


def _registered(hip, *a, **kw):
    s = _solver(hip, *a, **kw)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    return s


def _fields(sc):
    return np.stack([sc.evaluated, sc.inliers, sc.plane_inliers, sc.sum_d2, sc.sum_r2, sc.cost], axis=1).astype(np.float64)


def _check(got, want, label, pairs=None, gate=None):
    """got: ParticleScores; want: [P, 6] of the restatement at got's poses."""
    g = _fields(got)
    print(f"{label}: evaluated {g[:, 0].min():.0f}..{g[:, 0].max():.0f} inliers {g[:, 1].min():.0f}..{g[:, 1].max():.0f} plane "
          f"{g[:, 2].min():.0f}..{g[:, 2].max():.0f} | max rel diff sum_d2 {np.abs(g[:, 3] - want[:, 3]).max() / max(want[:, 3].max(), 1e-300):.3e} "
          f"sum_r2 {np.abs(g[:, 4] - want[:, 4]).max() / max(want[:, 4].max(), 1e-300):.3e} cost {np.abs(g[:, 5] - want[:, 5]).max() / want[:, 5].max():.3e}")
    if pairs is not None:
        near_gate, tie = ps.preconditions(pairs, gate)
        assert near_gate.size == 0 and tie.size == 0, label
    assert not np.isnan(g).any(), label
    assert np.array_equal(g[:, :3], want[:, :3]), label
    assert np.allclose(g[:, 3:], want[:, 3:], rtol=TIGHT, atol=0), label


def _poses12(sc):
    return np.concatenate([sc.poses[:, :, :3].reshape(-1, 9), sc.poses[:, :, 3]], axis=1)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("early_stop", [False, True])
@pytest.mark.parametrize("svgd", [False, True])
@pytest.mark.parametrize("K", pc.KS)
@pytest.mark.parametrize("P", pc.PS)
def test_scores_agree_with_the_restatement(hip, orc, P, K, svgd, early_stop):
    """Every particle geometry (16 / 32 / 64 lanes, 1 / 2 / 4 waves along the particles) against every K: tiles as high as
    the workgroup's row slots and lower ones (K = 128, 150), B = 300 = 4 * 64 + 44 rows: a partial workgroup and a partial
    tile.  Two gates, without and with supplied normals, on one registration."""
    cloud = pc.cloud_of(P, K)
    src, tgt, nrm = _case(hip, orc, cloud)
    I = pc.iterations_of(P, K)
    kw = dict(check_early_stop=True, convergence_threshold=10.0) if early_stop else {}
    s = _registered(hip, src, tgt, P, K, iterations=I, svgd=svgd, **kw)
    if early_stop and I > 1 and P > 1:
        assert s.get_iterations_run() < I
    cand = s.get_candidates()
    pairs = None
    for normals in (None, nrm):
        if normals is not None:
            s.set_target_normals(normals)
        for gate in pc.GATES:
            got = s.score_particles(gate)
            assert got.poses.shape == (P, 3, 4) and np.isfinite(got.poses).all()
            if pairs is None:
                pairs = ps.pairs(src, tgt, cand, _poses12(got))
            else:
                assert np.array_equal(_poses12(got), pairs_poses)       # the same registration: the same poses every time
            pairs_poses = _poses12(got)
            want = ps.score(src, tgt, cand, pairs_poses, gate, normals=normals, pr=pairs)
            _check(got, want, f"{cloud} P {P} K {K} I {I} svgd {svgd} stop {early_stop} gate {gate} normals {normals is not None}", pairs, gate)
            assert (got.evaluated == pc.B_).all() and (got.plane_inliers > 0).all() == (normals is not None)
            again = s.get_particle_scores()
            assert _fields(again).tobytes() == _fields(got).tobytes() and again.poses.tobytes() == got.poses.tobytes()


# ------------------------------------------------------------------------------------------------ 2. the poses
@pytest.mark.parametrize("P,K", [(4, 16), (130, 128), (9, 150)])
def test_scored_poses_are_the_particles_total_poses(hip, orc, P, K):
    src, tgt, _ = _case(hip, orc, "random")
    T0 = pc.initial_mean(hip)
    for kw in ({}, dict(check_early_stop=True, convergence_threshold=10.0)):
        s = _registered(hip, src, tgt, P, K, **kw)
        got = _poses12(s.score_particles(0.3))
        want = pc.total_poses(so3_exp_np, s.get_particles(), T0)
        print(f"P {P} K {K} {kw}: max |pose - T0 * Pose(Exp r, t)| = {np.abs(got - want).max():.3e}")
        assert np.abs(got - want).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ 3. edges
@pytest.mark.parametrize("B,M", [(1, 1), (70, 64)])
def test_score_edges(hip, B, M):
    src, tgt = hip.scans.random_clouds(B, M, seed=7)
    for P, K in ((4, 16), (9, 1)):
        s = _registered(hip, src, tgt, P, K)
        got = s.score_particles(1.0)
        _check(got, ps.score(src, tgt, s.get_candidates(), _poses12(got), 1.0), f"B {B} M {M} P {P} K {K}")
        assert (got.evaluated == B).all()


@pytest.mark.parametrize("nan_target_0", [False, True])
def test_score_with_nonfinite_and_huge_rows(hip, orc, nan_target_0):
    """A NaN source row, a 1e160 source row, NaN / inf target rows, and a NaN target row 0: the candidate 0 (the contract's
    filler) of every row without an eligible target.  Plane mode: a non-finite pair is rejected there, so the particles stay
    finite (in point mode it turns the sums, and with them every pose, into NaN) — and the context holds estimated normals."""
    src, tgt, _ = _case(hip, orc, "random")
    src_rows, tgt_rows = [3, 64, 65, 299], [5, 511, 2999]
    src_b, tgt_b = nf.poison(src, src_rows, ("nan1", "big64", "nan3", "big64")), nf.poison(tgt, tgt_rows, ("nan1", "+inf", "nan3"))
    if nan_target_0:
        tgt_b = nf.poison(tgt_b, [0], "nan1")
    s = _registered(hip, src_b, tgt_b, 9, 16, residual="plane")
    cand, nrm = s.get_candidates(), s.get_target_normals()
    if nan_target_0:
        assert (cand[[3, 65]] == 0).all()
    for gate in pc.GATES:
        got = s.score_particles(gate)
        assert np.isfinite(got.poses).all()
        want = ps.score(src_b, tgt_b, cand, _poses12(got), gate, normals=nrm)
        _check(got, want, f"non-finite target0 {nan_target_0} gate {gate}")
        # the NaN rows are not evaluated; the 1e160 rows are (d2 = +inf) and are never inliers
        assert (got.evaluated == len(src) - 2).all() and (got.inliers <= len(src) - 4).all() and (got.plane_inliers > 0).all()
        assert np.isfinite(_fields(got)).all()


# ------------------------------------------------------------------------------------------------ 4. weights
def _weighted(hip, src, tgt, temperature, **kw):
    w = hip.ParticleWeightOpt(True, pc.WEIGHT_GATE, temperature)
    return _registered(hip, src, tgt, pc.WEIGHT_P, pc.WEIGHT_K, weight=w, **kw)


@pytest.mark.parametrize("cloud", pc.CLOUDS)
def test_weights_and_weighted_statistics(hip, orc, cloud):
    src, tgt, _ = _case(hip, orc, cloud)
    s = _weighted(hip, src, tgt, pc.WEIGHT_T)
    sc = s.get_particle_scores()                                  # the registration's own scoring, no further GPU work
    _check(sc, ps.score(src, tgt, s.get_candidates(), _poses12(sc), pc.WEIGHT_GATE), f"{cloud} weighted registration")
    w = s.get_particle_weight()
    want_w = ps.weights(sc.cost, pc.WEIGHT_T)
    print(f"{cloud}: weights {w.min():.3e}..{w.max():.3e} sum - 1 = {w.sum() - 1.0:.3e} max rel diff {np.abs(w / want_w - 1).max():.3e}")
    assert np.allclose(w, want_w, rtol=1e-12, atol=0) and abs(w.sum() - 1.0) <= 1e-12
    assert w.max() > 2.0 / pc.WEIGHT_P                            # not the uniform weights in disguise
    x = s.get_particles()
    mean, var, cov = ps.weighted_stats(x, w)
    tol = 1e-12 * np.abs(x).max()
    got = (s.get_transformation(), s.get_distribution(), s.get_cov_matrix())
    print(f"{cloud}: |mean| {np.abs(got[0] - mean).max():.3e} |var| {np.abs(got[1] - var).max():.3e} |cov| {np.abs(got[2] - cov.reshape(36)).max():.3e} tol {tol:.3e}")
    assert np.abs(got[0] - mean).max() <= tol and np.abs(got[1] - var).max() <= tol and np.abs(got[2] - cov.reshape(36)).max() <= tol
    # what builds on the mean follows: evaluate(NULL, NULL) is taken at the weighted mean
    ev = s.evaluate(0.3)
    assert np.allclose(ev.pose, pc.initial_mean(hip) @ hip.pipeline.correction_to_pose(got[0]), rtol=0, atol=TIGHT)
    # a scoring by hand at the same gate gives the registration's scores bit for bit; another gate replaces them
    assert _fields(s.score_particles(pc.WEIGHT_GATE)).tobytes() == _fields(sc).tobytes()
    assert _fields(s.score_particles(1.0)).tobytes() == _fields(s.get_particle_scores()).tobytes() != _fields(sc).tobytes()
    assert np.array_equal(s.get_particle_weight(), w)            # scoring changes no result
    # asynchronous registration + synchronize: the pinned result block carries the weighted figures
    a = _solver(hip, src, tgt, pc.WEIGHT_P, pc.WEIGHT_K, weight=hip.ParticleWeightOpt(True, pc.WEIGHT_GATE, pc.WEIGHT_T))
    a.stein_align_async()
    a.synchronize()
    assert np.array_equal(a.get_particle_weight(), w) and np.array_equal(a.get_transformation(), got[0]) and np.array_equal(a.get_cov_matrix(), got[2])


@pytest.mark.parametrize("cloud", pc.CLOUDS)
def test_cold_weights_pick_the_best_particle(hip, orc, cloud):
    src, tgt, _ = _case(hip, orc, cloud)
    s = _weighted(hip, src, tgt, pc.COLD_T)
    cost = s.get_particle_scores().cost
    order = np.argsort(cost)
    print(f"{cloud}: best cost {cost[order[0]]!r}, second {cost[order[1]]!r}")
    assert cost[order[1]] - cost[order[0]] >= 1e-6
    w, x = s.get_particle_weight(), s.get_particles().reshape(6, -1)
    assert w[order[0]] == 1.0 and np.count_nonzero(w) == 1
    assert np.array_equal(s.get_transformation(), x[:, order[0]])
    assert np.array_equal(s.get_distribution(), np.zeros(6)) and np.array_equal(s.get_cov_matrix(), np.zeros(36))


def test_use_weight_mean_alone_is_inert(hip, orc):
    src, tgt, _ = _case(hip, orc, "random")
    plain = _registered(hip, src, tgt, pc.WEIGHT_P, pc.WEIGHT_K)
    flag = _registered(hip, src, tgt, pc.WEIGHT_P, pc.WEIGHT_K, weight=hip.ParticleWeightOpt(True))
    assert np.array_equal(plain.get_particle_weight(), flag.get_particle_weight())
    assert np.array_equal(plain.get_particle_weight(), np.full(pc.WEIGHT_P, np.float64(np.float32(1.0) / np.float32(pc.WEIGHT_P))))
    assert np.array_equal(plain.get_transformation(), flag.get_transformation())
    rc = flag._L.svnicp_get_particle_scores(flag.handle, None, None)
    assert rc == ERR_INVALID and "no scoring yet" in flag._L.svnicp_last_error(flag.handle).decode()


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


@pytest.mark.parametrize("P,K", [(16, 16), (130, 128), (4, 150)])
def test_uniform_weighting_changes_nothing(hip, orc, P, K):
    src, tgt, _ = _case(hip, orc, "random")
    kw = dict(record_trace=True)

    def again(s):
        s.add_cloud(src, tgt, pc.particles(hip, P))
        assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
        return _snapshot(s)

    f = _registered(hip, src, tgt, P, K, **kw)                    # the context that never sets, scores or weights: its n-th
    fresh = _snapshot(f)                                          # registration is what the other's n-th must equal
    s = _solver(hip, src, tgt, P, K, **kw)                        # set and reset
    s.set_particle_weighting("softmin", 0.3, 1e-3)
    s.set_particle_weighting("uniform")
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    _same(fresh, _snapshot(s))
    s.set_particle_weighting("softmin", 0.3, 1e-3)                # a weighted registration …
    weighted, fresh = again(s), again(f)
    assert weighted["weights"].tobytes() != fresh["weights"].tobytes()
    for k in ("particles", "history", "candidates", "cand_d2", "trace_H", "trace_corr", "iterations"):   # the iterations do not see the weights
        assert weighted[k].tobytes() == fresh[k].tobytes(), k
    s.set_particle_weighting("uniform")                           # … and the uniform one after it
    _same(again(f), again(s))
    fresh = _snapshot(f)
    one = s.score_particles(0.3)                                  # after a scoring: nothing a getter returns has changed …
    _same(fresh, _snapshot(s))
    two = s.score_particles(0.3)                                  # … two scorings give identical bits …
    assert _fields(one).tobytes() == _fields(two).tobytes() and one.poses.tobytes() == two.poses.tobytes()
    _same(again(f), again(s))                                     # … and the next registration is that of the untouched context


# ------------------------------------------------------------------------------------------------ 6. refusals
def _err(s):
    return s._L.svnicp_last_error(s.handle).decode()


def _align_refused(s, needle):
    rc = s._L.svnicp_align_begin(s.handle)
    assert rc == ERR_INVALID and "particle weighting" in _err(s) and needle in _err(s), (rc, _err(s))


def _score_refused(s, needle):
    out = np.zeros((s._P, 6))
    rc = s._L.svnicp_score_particles(s.handle, 0.3, out.ctypes.data_as(C.POINTER(C.c_double)), None)
    assert rc == ERR_INVALID and needle in _err(s), (rc, _err(s))


def _split_phase(s, iterations):
    L, h = s._L, s.handle
    assert L.svnicp_align_begin(h) == 0, _err(s)
    assert L.svnicp_stage_candidates(h, 0, s._B) == 0 and L.svnicp_build_candidate_table(h) == 0, _err(s)
    for it in range(iterations):
        assert L.svnicp_iter_accumulate(h, it) == 0 and L.svnicp_iter_update(h, it) == 0, _err(s)
    assert L.svnicp_finish(h) == 0 and L.svnicp_synchronize(h) == 0, _err(s)


def test_weighting_refusals(hip, orc):
    src, tgt, _ = _case(hip, orc, "random")
    P, K = 16, 16
    s = _solver(hip, src, tgt, P, K)
    for args in ((1, 0.0, 1e-3), (1, -0.3, 1e-3), (1, float("nan"), 1e-3), (1, float("inf"), 1e-3), (2, 0.0, 0.0)):
        assert s._L.svnicp_set_particle_weighting(s.handle, *args) == ERR_INVALID and "max_corr_dist" in _err(s), args
    for args in ((1, 0.3, 0.0), (1, 0.3, -1.0), (1, 0.3, float("nan")), (1, 0.3, float("inf"))):
        assert s._L.svnicp_set_particle_weighting(s.handle, *args) == ERR_INVALID and "temperature" in _err(s), args
    assert s._L.svnicp_set_particle_weighting(s.handle, 2, 0.3, 1e-3) == 0
    _align_refused(s, "unknown weighting kind")
    s.set_particle_weighting("softmin", 0.3, 1e-3)
    assert s._L.svnicp_set_shard(s.handle, 0, 8) == 0
    _align_refused(s, "particle shard")
    assert s._L.svnicp_set_shard(s.handle, 0, P) == 0
    assert s._L.svnicp_set_row_shard(s.handle, 0, 2, 2 * len(src)) == 0
    _align_refused(s, "row shard")
    assert s._L.svnicp_set_row_shard(s.handle, 0, 1, 0) == 0
    s.set_minibatch(64, 1)
    _align_refused(s, "mini-batch")
    s.set_minibatch(0)
    s.set_option("correspondence", "full")
    _align_refused(s, "correspondence=full")
    s.set_option("correspondence", "fast")
    g = _solver(hip, src, tgt, P, K, svgd=True)
    g.set_particle_weighting("softmin", 0.3, 1e-3)
    _align_refused(g, "SVGD")
    assert hip.SVGDICP(hip.SteinICPParam(iterations=1), pc.particles(hip, 4), hip.ParticleWeightOpt(True, 0.3, 1e-3))   # the option is SVNICP's
    # the refused context stays usable: the same one now registers, weighted, and agrees with a fresh one
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    fresh = _weighted(hip, src, tgt, 1e-3)
    assert np.array_equal(s.get_particle_weight(), fresh.get_particle_weight()) and np.array_equal(s.get_transformation(), fresh.get_transformation())
    g.set_particle_weighting("uniform")
    assert g.stein_align() == hip.SteinICPState.ALIGN_SUCCESS and g.score_particles(0.3).cost.shape == (P,)


def test_scoring_refusals(hip, orc):
    src, tgt, _ = _case(hip, orc, "random")
    P, K, I = 16, 16, 2
    s = _solver(hip, src, tgt, P, K, iterations=I)
    _score_refused(s, "no finished registration")
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    for gate in (0.0, -1.0, float("nan"), float("inf")):
        out = np.zeros((P, 6))
        assert s._L.svnicp_score_particles(s.handle, gate, out.ctypes.data_as(C.POINTER(C.c_double)), None) == ERR_INVALID and "max_corr_dist" in _err(s)
    want = _fields(s.score_particles(0.3))
    s.set_k(K)
    _score_refused(s, "register again")
    s.set_option("correspondence", "full")
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    _score_refused(s, "correspondence=full")
    s.set_option("correspondence", "fast")
    s.set_minibatch(64, 1)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    _score_refused(s, "mini-batch")
    s.set_minibatch(0)
    assert s._L.svnicp_set_shard(s.handle, 0, 8) == 0
    _split_phase(s, I)
    _score_refused(s, "particle shard")
    assert s._L.svnicp_set_shard(s.handle, 0, P) == 0
    assert s._L.svnicp_set_row_shard(s.handle, 0, 2, 2 * len(src)) == 0
    _split_phase(s, I)
    _score_refused(s, "row shard")
    assert s._L.svnicp_set_row_shard(s.handle, 0, 1, 0) == 0
    # the refused context stays usable
    s.add_cloud(src, tgt, pc.particles(hip, P))
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    assert np.allclose(_fields(s.score_particles(0.3)), want, rtol=TIGHT, atol=0)


# ------------------------------------------------------------------------------------------------ 7. the pipeline
def test_pipeline_with_weighted_particles(hip):
    """Five scans through the pipeline with weight_dist set: it runs, the weights reach ScanResult and sum to 1, and the
    poses stay within 1e-3 of the unweighted run.  The temperature is chosen so that this bound follows from the contract
    alone: the costs lie in [0, gate^2], so P w_p lies in [e^-A, e^A] with A = gate^2 / temperature, sum |w_p - 1/P| <=
    e^A - 1, and a coordinate of the weighted mean moves by at most (e^A - 1) R, R = 0.6 m the width of the particle prior
    (a Stein particle set keeps about that spread: it does not collapse onto its mode).  gate 0.5 m and 400 m^2 give
    A = 6.25e-4 and at most 3.8e-4 per registration.  A sharp temperature moves the mean inside the spread of the particles by
    centimetres (printed, not asserted: DESIGN.md section 4.12)."""
    pl, sc = hip.pipeline, hip.scans
    scene = sc.make_scene()
    scans = [sc.lidar_scan(scene, sc.rot_zyx(0.0, 0.0, np.radians(0.3 * k)), np.array([0.0, 0.0, 0.05 * k]), 8192, stream=300 + k) for k in range(5)]
    gate, temperature = 0.5, 400.0
    assert np.expm1(gate * gate / temperature) * 0.6 <= 5e-4
    runs = {}
    for name, kw in (("uniform", {}), ("weighted", dict(weight_dist=gate, weight_temperature=temperature)),
                     ("sharp", dict(weight_dist=gate, weight_temperature=1e-3))):
        cfg = pl.PipelineConfig(min_range=1.0, max_range=80.0, voxel_size=0.5, map_voxel_size=0.5, map_voxel_max_points=20, map_range=100.0,
                                particle_count=32, solver=hip.SteinICPParam(iterations=30, lr=1.0, max_dist=1.0, KNN_count=50), **kw)
        pipe = pl.RegistrationPipeline(cfg, device=0)
        runs[name] = [pipe.process_scan(pts, stamp=0.1 * k) for k, pts in enumerate(scans)]
    uniform = np.float64(np.float32(1.0) / np.float32(32))
    for k in range(1, 5):
        u, w, sh = runs["uniform"][k], runs["weighted"][k], runs["sharp"][k]
        assert w.state == int(hip.SteinICPState.ALIGN_SUCCESS)
        assert abs(w.weights.sum() - 1.0) <= 1e-12 and (w.weights >= 0).all() and not np.array_equal(w.weights, u.weights)
        assert abs(sh.weights.sum() - 1.0) <= 1e-12 and sh.weights.max() > 2.0 / 32
        assert np.array_equal(u.weights, np.full(32, uniform))
        assert np.allclose(w.pose, w.initial_guess @ pl.correction_to_pose(w.correction))
        x = u.particles.reshape(6, -1)
        print(f"scan {k}: |pose - unweighted pose| = {np.abs(w.pose - u.pose).max():.3e} (weights {w.weights.min():.6e}..{w.weights.max():.6e}); "
              f"temperature 1e-3: {np.abs(sh.pose - u.pose).max():.3e} (weights {sh.weights.min():.3e}..{sh.weights.max():.3e}); "
              f"particle spread {np.round(x.max(1) - x.min(1), 4)}")
        assert np.abs(w.pose - u.pose).max() <= 1e-3
