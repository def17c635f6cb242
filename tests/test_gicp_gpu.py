"""The generalized-ICP residual on the device (include/svnicp_hip.h "generalized-ICP residual") against
tests/gicp_reference.py, the float64 numpy restatement that tests/test_gicp_cpu.py pins on its own.  The reference has no such
mode: every expectation is computed at test time.  Correspondences are held to equality, H, b, N, phi and h to
rtol = atol = TIGHT (1e-9, tests/helpers.py), particles and statistics to TIGHT: the tolerances of tests/test_plane_gpu.py."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

import gicp_reference as gr
import plane_cases
import plane_mp_reference as pm
import pose_prior_cases
from helpers import TIGHT

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
GICP = "svnicp_align: the generalized-ICP residual (svnicp_set_residual_gicp) is not available here: "


def _exp(w):
    w = np.asarray(w, float)
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) if a == 0 else np.eye(3) + np.sin(a) / a * K + (1 - np.cos(a)) / a ** 2 * K @ K


R0 = _exp([0.002, 0.001, -0.003])
T0 = np.array([0.01, 0.02, -0.01])


def _T(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


@functools.lru_cache(maxsize=None)
def _pair(B, M):
    """(source, target, target normals from 16 neighbours, source normals) of make_pair(B, M).  The source normals are
    SUPPLIED ones: the normal of the nearest target at the true pose, turned into the source frame — a 512-point sample of the
    scene is too sparse for neighbourhoods of its own (its estimated normals are valid on a quarter of the rows)."""
    import __graft_entry__ as graft
    pkg, orc = graft.load_package(), graft.load_oracle()
    p = pkg.scans.make_pair(B, M)
    nt, _, _ = gr.normals(orc, p.target, 16)
    Rtrue, ttrue = _exp(p.true_pose[3:]), np.asarray(p.true_pose[:3], float)
    nn, _ = orc.knn_topk(orc.transform(p.source, Rtrue, ttrue), p.target, 1)
    ns = np.ascontiguousarray(nt[nn[:, 0]] @ Rtrue)
    return p.source, p.target, nt, ns


def _solver(pkg, src, tgt, init, *, K=16, iterations=1, max_dist=1.0, lr=1.0, full=False, stop=False, thr=1e-5, trace=False,
            residual="gicp", delta=0.1, kn=16, eps=1e-3, options=(), mean=None):
    prm = pkg.SteinICPParam(iterations=iterations, lr=lr, max_dist=max_dist, KNN_count=K, SVN_full_grad=full,
                            check_early_stop=stop, convergence_threshold=thr, record_trace=trace)
    s = pkg.SVNICP(prm, init, pkg.ParticleWeightOpt())
    for k, v in options:
        s.set_option(k, v)
    if residual is not None:
        s.set_residual(residual, delta, kn, eps)
    s.add_cloud(src, tgt, init)
    s.set_initial_mean(_T(*mean) if mean is not None else np.eye(4))
    return s


def _outputs(s):
    return [s.get_particles(), s.get_transformation(), s.get_distribution(), s.get_cov_matrix(), s.get_particle_history()]


# ---------------------------------------------------------------------------------------------
# 1. the source's normal pass
# ---------------------------------------------------------------------------------------------
# The isolated-cluster clouds of tests/plane_cases.py as the SOURCE: every row's normal_k nearest source points are its own
# cluster, so the neighbourhood is known without a search, and the pass is held to the judgment of
# tests/test_plane_alone_gpu.py::test_normals_alone — plane_mp_reference.judge_clusters against the exact eigenvalues and
# validity of tests/golden/plane.npz: validity on every row (the kinds that sit on the rule lambda1 >= 0.01 lambda2 included),
# an exact kind's normal a signed unit axis vector bit for bit, | |n| - 1 | <= 4 * 2^-53, eigen-residual and Rayleigh excess
# against the cluster's exact scatter matrix within 16 max(E_ref, kn 2^-52) — no second number for rows with a small gap.
# knn = tiles needs 8192 source rows to plan the tile kernels for the source cloud: the clusters are then repeated on a lattice
# far outside each other's reach.  The copies' coordinates are rounded anew, so their exact matrices are not the fixture's:
# they are held to what survives a shift by whole metres — validity on every row (the threshold kinds lie 1e-6 from the rule,
# the shift moves a matrix by 1e-12; the exact kinds stay exact) and the exact kinds' axis vectors bit for bit.
_spec = importlib.util.spec_from_file_location("make_plane", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_plane.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)
NORM_BAR = 4 * 2.0 ** -53


class _Placement:
    """The clusters of one placement of a normal case, rows renumbered for a cloud that holds them alone, in cluster order."""
    def __init__(self, case, ref, placement):
        self.kn, self.name = case.kn, case.name + "/" + placement
        keep = [i for i, c in enumerate(case.clusters) if c.placement == placement]
        self.clusters, at = [], 0
        for i in keep:
            c = case.clusters[i]
            k = plane_cases.Cluster(c.kind, c.placement, c.pts, c.declared, c.axis, c.judged)
            k.rows = np.arange(at, at + len(c.pts))
            at += len(c.pts)
            self.clusters.append(k)
        self.lam, self.valid = [ref["lam"][i] for i in keep], [ref["valid"][i] for i in keep]
        self.pts = np.ascontiguousarray(np.concatenate([c.pts for c in self.clusters]))


def _cluster_source(sub, rows_min):
    reps = max(1, -(-rows_min // len(sub.pts)))
    step = 16.0 * plane_cases.SPACING                        # a 4 x 4 x n lattice of copies, 8192 m apart; copy 0 is the case itself
    return np.ascontiguousarray(np.concatenate([sub.pts + step * np.array([r % 4, (r // 4) % 4, r // 16], np.float64) for r in range(reps)])), reps


@pytest.fixture(scope="module")
def plane_fixture():
    return mk.load()


@pytest.mark.parametrize("shifted", [False, True], ids=["origin", "shifted"])
@pytest.mark.parametrize("knn", [None, "brute", "tiles"], ids=["default", "brute", "tiles"])
@pytest.mark.parametrize("kn", [8, 16])
def test_estimated_source_normals_row_by_row(hip, plane_fixture, kn, knn, shifted):
    case = next(c for c in plane_cases.normal_cases() if c.name == "normals_kn%d" % kn)
    ref = mk.normal_reference(plane_fixture, case)
    assert ref["chk"] == int(case.checksum()), "tests/golden/plane.npz is stale: run tests/golden/make_plane.py"
    sub = _Placement(case, ref, "shifted" if shifted else "origin")
    src, reps = _cluster_source(sub, 8192 if knn == "tiles" else 0)
    tgt = src[:64] + 0.25                                    # any target: the source pass does not read it
    s = _solver(hip, src, tgt, np.zeros((6, 1)), K=4, kn=kn, options=(("knn", knn),) if knn else ())
    s.set_target_normals(np.tile([0.0, 0.0, 1.0], (len(tgt), 1)))
    assert s._L.svnicp_align_begin(s.handle) == 0, s._L.svnicp_last_error(s.handle)
    n = s.get_source_normals()
    assert s.get_gicp_stats(with_sums=False)[1] == (0, 1)
    s.close()
    assert n.shape == src.shape and np.isfinite(n).all()
    nb = len(sub.pts)
    wrong, fig, axes = pm.judge_clusters(sub, sub.lam, sub.valid, n[:nb])
    assert not wrong, "%d rows have a normal where there is none, or none where there is one; first (kind, placement, row): %s" % (len(wrong), wrong[:4])
    assert not axes, "an exactly diagonal scatter matrix must give a signed unit axis vector bit for bit: %s" % (axes[:4],)
    assert set(fig) == {c.kind for c, v in zip(sub.clusters, sub.valid) if v}, "every valid kind was judged"
    bar = 16.0 * max(max(ref["eref"]), kn * 2.0 ** -52)
    for kind, (nm, res, ray) in sorted(fig.items()):
        print("%s %-18s | |n| - 1 | %.2e (bar %.2e), residual %.2e, rayleigh %.2e (bar %.2e)" % (sub.name, kind, nm, NORM_BAR, res, ray, bar))
        assert nm <= NORM_BAR and res <= bar and abs(ray) <= bar, (sub.name, kind, nm, res, ray)
    has0 = (n[:nb] != 0.0).any(axis=1)
    exact_rows = np.concatenate([c.rows for c in sub.clusters if c.axis is not None and c.declared])
    for r in range(1, reps):                                 # the lattice copies: every row's validity, the exact kinds bit for bit
        blk = n[r * nb:(r + 1) * nb]
        assert np.array_equal((blk != 0.0).any(axis=1), has0), "copy %d: validity differs from the case's own rows" % r
        assert np.array_equal(np.abs(blk[exact_rows]), np.abs(n[exact_rows])), "copy %d: an exact kind's axis vector" % r


# ---------------------------------------------------------------------------------------------
# 2. solver parity with supplied normals on both sides
# ---------------------------------------------------------------------------------------------
PAR = dict(K=16, iterations=10, max_dist=0.3, delta=0.05, eps=1e-3)
STOP_THR = 0.03


@pytest.mark.parametrize("stop", [False, True], ids=["full", "earlystop"])
@pytest.mark.parametrize("P", [1, 4, 64, 130], ids=["P1", "P4", "P64", "P130"])
def test_solver_parity_with_supplied_normals(hip, orc, P, stop):
    src, tgt, nt, ns = _pair(512, 2048)
    init = hip.scans.make_particles(P, seed=3) * 0.2
    ref = gr.run(orc, src, tgt, nt, ns, init, PAR["K"], PAR["iterations"], PAR["max_dist"], PAR["delta"], PAR["eps"], lr=1.0,
                 svn_full_grad=False, check_early_stop=stop, convergence_threshold=STOP_THR, R0=R0, t0=T0)
    # the restatement's own run shows the configuration exercises the gate, both Huber branches and (when on) the early stop
    res = np.concatenate([np.concatenate(x) for x in ref.residuals])
    outside = float((res > PAR["delta"]).mean())
    assert 0.05 <= outside <= 0.95, outside
    cand, _ = orc.knn_topk(orc.transform(src, R0, T0), tgt, PAR["K"])
    Rt, tt = gr.total_pose(orc, init[:, 0], R0, T0)
    _, ok_gate, _, _ = gr.pairs(src, tgt, nt, ns, cand, Rt, tt, PAR["max_dist"])
    _, ok_all, _, _ = gr.pairs(src, tgt, nt, ns, cand, Rt, tt, np.inf)
    assert ok_gate.sum() < ok_all.sum() < src.shape[0], "max_dist must reject pairs that have both normals, and some rows have none"
    if stop:
        assert 1 < ref.iterations_run < PAR["iterations"], ref.iterations_run
    else:
        assert ref.iterations_run == PAR["iterations"]

    s = _solver(hip, src, tgt, init, K=PAR["K"], iterations=PAR["iterations"], max_dist=PAR["max_dist"], stop=stop, thr=STOP_THR,
                trace=True, delta=PAR["delta"], eps=PAR["eps"], mean=(R0, T0))
    s.set_target_normals(nt)
    s.set_source_normals(ns)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    assert s.get_gicp_stats(with_sums=False)[1] == (0, 0), "supplied normals: no normal pass on either side"
    run = s.get_iterations_run()
    assert run == ref.iterations_run
    tr = s.get_trace()
    assert np.array_equal(tr["corr"][:run], ref.corr[:run])
    for k, r in (("H", ref.H), ("b", ref.b), ("newton", ref.newton), ("phi", ref.phi)):
        d = np.abs(tr[k][:run] - r[:run]).max()
        print(f"P {P} {k}: max |device - restatement| = {d:.3e} (max |restatement| {np.abs(r[:run]).max():.3e})")
        assert np.allclose(tr[k][:run], r[:run], rtol=TIGHT, atol=TIGHT), k
    assert np.allclose(tr["h"][:run], ref.h[:run], rtol=TIGHT, atol=TIGHT, equal_nan=True)
    assert np.abs(s.get_particles() - ref.particles).max() <= TIGHT
    assert np.abs(s.get_transformation() - ref.solver.get_transformation()).max() <= TIGHT
    assert np.abs(s.get_distribution() - ref.solver.get_distribution()).max() <= TIGHT
    assert np.abs(s.get_cov_matrix() - ref.solver.get_cov_matrix()).max() <= TIGHT
    stats, _ = s.get_gicp_stats()
    assert np.array_equal(stats[:, 0], ref.stats[:, 0])
    assert np.allclose(stats[:, 1], ref.stats[:, 1], rtol=TIGHT, atol=TIGHT)
    kept = s.get_source_normals()
    assert np.array_equal(kept != 0.0, ns != 0.0) and np.abs(kept - gr.normalise_supplied(ns, src)).max() <= 2 * 2.0 ** -53
    s.close()


def _mixed_normals(ns):
    """The supplied source normals turned away from the target's: every row by a random 0.3 (about 17 degrees), every fourth
    row replaced by a random direction.  _pair's own are parallel to the winner's normal in almost every pair, the regime where
    W collapses to (1 - eps) m m^T + eps I; these make S a general symmetric matrix.  (Registrations of several particles do not
    converge with them, so the multi-iteration parity test keeps _pair's; a record of one iteration needs no convergence.)"""
    rng = np.random.default_rng(7)
    v = rng.standard_normal(ns.shape)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    mix = np.where((np.arange(len(ns)) % 4 == 3)[:, None], v, ns + 0.3 * v)
    mix /= np.linalg.norm(mix, axis=1, keepdims=True)
    return np.ascontiguousarray(np.where((ns != 0.0).any(axis=1)[:, None], mix, 0.0))


@pytest.mark.parametrize("eps,mixed", [(1.0, False), (1e-6, False), (1e-3, True), (1e-6, True)], ids=["eps1", "eps1e-6", "eps1e-3-mixed", "eps1e-6-mixed"])
def test_one_iteration_record(hip, orc, eps, mixed):
    """The general inverse (source normals that are not parallel to the winners': `mixed`), eps = 1 (W = I: the unweighted point-to-point cost of the pairs that have both normals) and eps = 1e-6 (cond(S) up to 1e6)
    against the restatement: the record H | b of ONE iteration at the initial particles.  Device and restatement evaluate the same
    cofactor expressions, so the closed-form inverse's cond(S) u is common to both and TIGHT holds.  The particles behind the
    Stein step are not compared here: at eps = 1e-6 H of this scene is singular up to the 1e-6 damping and the Newton step is
    hundreds of metres long, which says nothing about the record."""
    src, tgt, nt, ns = _pair(512, 2048)
    if mixed:
        ns = _mixed_normals(ns)
        cos = np.abs((ns * _pair(512, 2048)[3]).sum(axis=1))
        assert np.median(cos) < 0.97 and (cos < 0.7).mean() > 0.15, "the normals must leave the parallel regime"
    init = hip.scans.make_particles(16, seed=3) * 0.2
    ref = gr.run(orc, src, tgt, nt, ns, init, 16, 1, 0.3, 0.05, eps, svn_full_grad=False, R0=R0, t0=T0)
    s = _solver(hip, src, tgt, init, iterations=1, max_dist=0.3, trace=True, delta=0.05, eps=eps, mean=(R0, T0))
    s.set_target_normals(nt)
    s.set_source_normals(ns)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    tr = s.get_trace()
    assert np.array_equal(tr["corr"], ref.corr)
    for k, r in (("H", ref.H), ("b", ref.b)):
        d = np.abs(tr[k] - r).max()
        print(f"eps {eps:g} {k}: max |device - restatement| = {d:.3e} (max |restatement| {np.abs(r).max():.3e})")
        assert np.allclose(tr[k], r, rtol=TIGHT, atol=TIGHT), k
    stats, _ = s.get_gicp_stats()
    assert np.array_equal(stats[:, 0], ref.stats[:, 0]) and np.allclose(stats[:, 1], ref.stats[:, 1], rtol=TIGHT, atol=TIGHT)
    s.close()


def test_pose_prior_on_a_gicp_context(hip, orc):
    """svnicp_set_pose_prior with the generalized-ICP residual: the restatement's record plus tests/pose_prior_reference.py's
    terms in front of the oracle's Stein step."""
    src, tgt, nt, ns = _pair(512, 2048)
    P = 16
    init = pose_prior_cases.scene_particles(P)
    prior = (pose_prior_cases.MU_NONZERO * 0.1, pose_prior_cases.lam_diag())
    ref = gr.run(orc, src, tgt, nt, ns, init, 16, 5, 0.3, 0.05, 1e-3, svn_full_grad=False, prior=prior)
    s = _solver(hip, src, tgt, init, iterations=5, max_dist=0.3, trace=True, delta=0.05)
    s.set_target_normals(nt)
    s.set_source_normals(ns)
    s.set_pose_prior(*prior)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    tr = s.get_trace()
    assert np.array_equal(tr["corr"], ref.corr)
    for k, r in (("H", ref.H), ("b", ref.b)):
        assert np.allclose(tr[k], r, rtol=TIGHT, atol=TIGHT), k
    assert np.abs(s.get_particles() - ref.particles).max() <= TIGHT
    plain = _solver(hip, src, tgt, init, iterations=5, max_dist=0.3, delta=0.05)
    plain.set_target_normals(nt)
    plain.set_source_normals(ns)
    plain.stein_align()
    assert np.abs(plain.get_particles() - s.get_particles()).max() > 1e-6, "the prior must move the result"
    s.close()
    plain.close()


# ---------------------------------------------------------------------------------------------
# 3. estimated normals end to end, and their reuse
# ---------------------------------------------------------------------------------------------
def test_estimated_normals_end_to_end_and_reuse(hip, orc):
    """make_pair(4096, 8192), 8 particles, 10 iterations, K = 20, max_dist 1, delta 0.1, normal_k 16: the device with ITS normals
    of both clouds against the restatement with its own.  Bound 1e-6, as tests/test_plane_gpu.py has it for the same reason
    (normals of points with a small eigenvalue gap differ by about 1e-15 / gap).  Then the passes: {1, 1}; {1, 1} again after
    svnicp_set_particles alone, with the outputs of a fresh context; a source pass again after svnicp_set_source."""
    p = hip.scans.make_pair(4096, 8192)
    src, tgt = p.source, p.target
    nt, _, _ = gr.normals(orc, tgt, 16)
    ns, vs, _ = gr.normals(orc, src, 16)
    init = hip.scans.make_particles(8)
    ref = gr.run(orc, src, tgt, nt, ns, init, 20, 10, 1.0, 0.1, 1e-3, lr=1.0, svn_full_grad=False)
    s = _solver(hip, src, tgt, init, K=20, iterations=10)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    d = np.abs(s.get_transformation() - ref.solver.get_transformation()).max()
    dp_ = np.abs(s.get_particles() - ref.particles).max()
    stats, passes = s.get_gicp_stats()
    print(f"estimated normals end to end: |mean pose device - restatement| max = {d:.3e}, particles {dp_:.3e}; source normals valid "
          f"{vs.mean():.4f}; accepted pairs {stats[:, 0].min():.0f}..{stats[:, 0].max():.0f}")
    assert d <= 1e-6
    assert passes == (1, 1)
    assert np.mean((s.get_source_normals() != 0).any(axis=1) != vs) < 1e-3, "validity differs at the threshold only"
    first = _outputs(s)
    dp = C.POINTER(C.c_double)
    s._check(s._L.svnicp_set_particles(s.handle, np.ascontiguousarray(init).ctypes.data_as(dp), 8), "svnicp_set_particles")
    s.stein_align()                                   # same clouds: no second pass on either side …
    assert s.get_gicp_stats(with_sums=False)[1] == (1, 1)
    for a, b in zip(_outputs(s), first):              # … and the same result
        assert np.array_equal(a, b)
    s._check(s._L.svnicp_set_source(s.handle, np.ascontiguousarray(src).ctypes.data_as(C.c_void_p), src.shape[0], 0), "svnicp_set_source")
    assert s._L.svnicp_get_source_normals(s.handle, np.zeros_like(src).ctypes.data_as(dp)) == ERR_INVALID   # dropped with the source
    s._check(s._L.svnicp_set_particles(s.handle, np.ascontiguousarray(init).ctypes.data_as(dp), 8), "svnicp_set_particles")
    s.stein_align()                                   # a new svnicp_set_source, even of the same points: the source's pass again
    assert s.get_gicp_stats(with_sums=False)[1] == (1, 2)
    for a, b in zip(_outputs(s), first):
        assert np.array_equal(a, b)
    s.set_residual("gicp", 0.1, 12)                   # another normal_k: both passes again
    s._check(s._L.svnicp_set_particles(s.handle, np.ascontiguousarray(init).ctypes.data_as(dp), 8), "svnicp_set_particles")
    s.stein_align()
    assert s.get_gicp_stats(with_sums=False)[1] == (2, 3)
    s.close()


# ---------------------------------------------------------------------------------------------
# 4. refusals, bad arguments, isolation
# ---------------------------------------------------------------------------------------------
def _refused(s, needle, begin=False):
    rc = s._L.svnicp_align_begin(s.handle) if begin else s._L.svnicp_align(s.handle)
    msg = s._L.svnicp_last_error(s.handle).decode()
    assert rc == ERR_INVALID, (rc, msg)
    assert msg.startswith(GICP) and needle in msg, msg


def test_gicp_mode_refusals(hip):
    src, tgt = hip.scans.random_clouds(512, 2048, seed=3)
    init = hip.scans.make_particles(16, seed=3) * 0.2

    def gicp(**kw):
        return _solver(hip, src, tgt, init, iterations=3, **kw)

    prm = hip.SteinICPParam(iterations=3, KNN_count=16, optimizer="Adam")
    g = hip.SVGDICP(prm, init)
    g.set_residual("gicp")
    g.add_cloud(src, tgt, init)
    _refused(g, "SVGD mode has no Hessian to put the plane residual in")
    s = gicp()
    assert s._L.svnicp_set_shard(s.handle, 0, 8) == 0
    _refused(s, "a partial particle shard (svnicp_set_shard) is set", begin=True)
    s = gicp()
    assert s._L.svnicp_set_row_shard(s.handle, 0, 2, 1024) == 0
    _refused(s, "a source-row shard (svnicp_set_row_shard) is set", begin=True)
    s = gicp()
    s.set_minibatch(64, 1)
    _refused(s, "mini-batch mode (svnicp_set_minibatch) is set")
    _refused(gicp(options=(("correspondence", "full"),)), "option correspondence=full is set")
    _refused(gicp(options=(("chain", "persistent"),)), "option chain=persistent is set")
    _refused(gicp(options=(("accum", "f64"),)), "option accum is not split")
    _refused(gicp(options=(("accum", "valu"),)), "option accum is not split")
    _refused(gicp(K=130), "knn_count exceeds 128")
    _refused(_solver(hip, src, tgt[:10], init, K=8, iterations=3, kn=16), "the target has fewer points than normal_k and no normals were supplied")
    few = _solver(hip, src[:10], tgt, init, K=8, iterations=3, kn=16)
    _refused(few, "the source has fewer points than normal_k and no source normals were supplied")
    few.set_source_normals(np.tile([0.0, 0.0, 1.0], (10, 1)))       # supplied: the ladder lets it pass
    assert few.stein_align() == hip.SteinICPState.ALIGN_SUCCESS


def test_bad_setter_arguments(hip):
    src, tgt = hip.scans.random_clouds(512, 2048, seed=3)
    init = hip.scans.make_particles(16, seed=3) * 0.2
    s = _solver(hip, src, tgt, init, iterations=3)
    L = s._L
    for args in ((0.1, 16, -1e-3), (0.1, 16, 1.0000001), (0.1, 16, float("nan")), (0.1, 16, 9e-7), (0.1, 16, float("inf")),
                 (0.0, 16, 1e-3), (-1.0, 16, 1e-3), (float("nan"), 16, 1e-3), (0.1, 3, 1e-3), (0.1, 65, 1e-3)):
        assert L.svnicp_set_residual_gicp(s.handle, *args) == ERR_INVALID, args
    assert L.svnicp_set_residual(s.handle, 2, 0.1, 16) == ERR_INVALID      # the mode is entered through its own setter only
    bad = np.zeros((src.shape[0] - 1, 3))
    assert L.svnicp_set_source_normals(s.handle, bad.ctypes.data_as(C.c_void_p), bad.shape[0], 0) == ERR_INVALID
    assert L.svnicp_set_source_normals(s.handle, None, src.shape[0], 0) == ERR_INVALID
    assert L.svnicp_get_source_normals(s.handle, np.zeros_like(src).ctypes.data_as(C.POINTER(C.c_double))) == ERR_INVALID   # none yet
    assert L.svnicp_get_gicp_stats(s.handle, np.zeros((16, 2)).ctypes.data_as(C.POINTER(C.c_double)), None) == ERR_INVALID    # no registration yet
    # epsilon = 0.0 is accepted on purpose: the header declares "0 / 0.0 = defaults 16 / 1e-3", the convention normal_k = 0 has in
    # svnicp_set_residual; every other value outside [1e-6, 1] is refused above
    assert L.svnicp_set_residual_gicp(s.handle, float("inf"), 0, 0.0) == 0      # +inf: unweighted; 0 / 0.0: the defaults 16 / 1e-3
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    assert np.isfinite(s.get_particles()).all()
    assert L.svnicp_set_residual_gicp(s.handle, 0.1, 16, 1e-6) == 0 and L.svnicp_set_residual_gicp(s.handle, 0.1, 16, 1.0) == 0
    s.close()


def test_all_zero_source_normals_accept_nothing(hip):
    src, tgt = hip.scans.random_clouds(512, 2048, seed=3)
    init = hip.scans.make_particles(16, seed=3) * 0.2
    s = _solver(hip, src, tgt, init, iterations=3)
    s.set_source_normals(np.zeros_like(src))
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    stats, passes = s.get_gicp_stats()
    assert passes == (1, 0) and np.array_equal(stats, np.zeros_like(stats))
    assert np.isfinite(s.get_particles()).all() and np.isfinite(s.get_transformation()).all()
    assert np.array_equal(s.get_source_normals(), np.zeros_like(src))
    s.close()


@pytest.mark.parametrize("P", [1, 16, 130])
def test_plane_and_point_modes_are_untouched(hip, P):
    """After a generalized-ICP registration on a context, svnicp_set_residual(PLANE) and then (POINT): every output array
    equals that of a fresh context of that mode (the pattern of test_point_residual_is_untouched)."""
    src, tgt = hip.scans.random_clouds(1024, 4096, seed=3)
    init = hip.scans.make_particles(P, seed=3) * 0.2

    def outputs(s):
        tr = s.get_trace()
        return _outputs(s) + [s.get_candidates(), tr["corr"], tr["H"], tr["b"], tr["newton"], tr["phi"], tr["h"]]

    point = _solver(hip, src, tgt, init, iterations=6, trace=True, residual=None)
    point.stein_align()
    plane = _solver(hip, src, tgt, init, iterations=6, trace=True, residual="plane")
    plane.stein_align()
    g = _solver(hip, src, tgt, init, iterations=6, trace=True)
    g.stein_align()
    assert g.get_gicp_stats(with_sums=False)[1] == (1, 1)
    assert not np.array_equal(g.get_particles(), plane.get_particles()), "the two residuals are different costs"
    g.set_residual("plane", 0.1, 16)
    g.add_cloud(src, tgt, init)
    g.stein_align()
    for x, y in zip(outputs(plane), outputs(g)):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.array_equal(g.get_plane_stats()[0], plane.get_plane_stats()[0])
    g.set_residual("point", 0.1, 16)
    g.add_cloud(src, tgt, init)
    g.stein_align()
    for x, y in zip(outputs(point), outputs(g)):
        assert np.array_equal(x, y, equal_nan=True)
    for s in (point, plane, g):
        s.close()
