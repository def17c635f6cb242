"""The point-to-plane residual on the device (include/svnicp_hip.h "point-to-plane residual") against
tests/plane_reference.py, the float64 numpy restatement that tests/test_plane_cpu.py pins on its own.  The reference has no
such mode: every expectation is computed at test time.  Correspondences are held to equality, H, b, N, phi and h to
rtol = atol = TIGHT (1e-9, tests/helpers.py), particles and statistics to TIGHT."""
import ctypes as C
import functools

import numpy as np
import pytest

import plane_reference as pr
from helpers import TIGHT

pytestmark = pytest.mark.gpu

SHIFT = np.array([3000.0, -2000.0, 50.0])
GAP_FLOOR = 1e-3       # normals are compared where (lambda1 - lambda0) / lambda2 >= this: the eigenvector of lambda0 is then
#                        determined to eps / gap ~ 1e-13 rad.  Helper on the CPU, normal_k = 8 and 16, both clouds, shifted and
#                        not: 0 % of the valid points lie below it (below 3e-3: 0.014 %, below 1e-2: 1.05 % at normal_k = 8).
ERR_INVALID = -1


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
def _clouds(pkg_id, name):
    import __graft_entry__ as graft
    scans = graft.load_package().scans
    if name == "random":
        return scans.random_clouds(2048, 8192, seed=3)
    if name == "pair2k":
        p = scans.make_pair(2048, 8192)
        return p.source, p.target
    p = scans.make_pair(4096, 8192)
    return p.source, p.target


_NORMALS = {}


def _ref_normals(orc, name, kn, shifted):
    key = (name, kn, shifted)
    if key not in _NORMALS:
        tgt = _clouds(0, name)[1] + (SHIFT if shifted else 0.0)
        _NORMALS[key] = pr.normals(orc, tgt, kn)
    return _NORMALS[key]


def _solver(pkg, src, tgt, init, *, K=16, iterations=1, max_dist=1.0, lr=1.0, full=False, stop=False, thr=1e-5, trace=False,
            residual=None, delta=0.1, kn=16, options=(), mean=None):
    prm = pkg.SteinICPParam(iterations=iterations, lr=lr, max_dist=max_dist, KNN_count=K, SVN_full_grad=full,
                            check_early_stop=stop, convergence_threshold=thr, record_trace=trace)
    s = pkg.SVNICP(prm, init, pkg.ParticleWeightOpt())
    for k, v in options:
        s.set_option(k, v)
    if residual is not None:
        s.set_residual(residual, delta, kn)
    s.add_cloud(src, tgt, init)
    s.set_initial_mean(_T(*mean) if mean is not None else np.eye(4))
    return s


# ---------------------------------------------------------------------------------------------
# 1. normals
# ---------------------------------------------------------------------------------------------
# every (cloud, normal_k, stage-A kernel, shift) at K = 16, and one search whose normal_k = 64 lists are larger than the
# context's own K = 3 would size
NORMAL_CASES = [pytest.param(name, kn, knn, shifted, 16, id=f"{name}-{kn}-{knn or 'default'}-{'shifted' if shifted else 'origin'}")
                for shifted in (False, True) for knn in (None, "brute", "tiles") for kn in (8, 16) for name in ("random", "pair4k")]
NORMAL_CASES.append(pytest.param("random", 64, "tiles", False, 3, id="random-64-tiles-origin-K3"))


@pytest.mark.parametrize("name,kn,knn,shifted,K", NORMAL_CASES)
def test_estimated_normals_agree_with_the_helper(hip, orc, name, kn, knn, shifted, K):
    src, tgt = _clouds(0, name)
    off = SHIFT if shifted else 0.0
    src, tgt = src + off, tgt + off
    ref_n, ref_valid, lam = _ref_normals(orc, name, kn, shifted)
    s = _solver(hip, src, tgt, np.zeros((6, 1)), K=K, residual="plane", kn=kn, options=(("knn", knn),) if knn else ())
    assert s._L.svnicp_align_begin(s.handle) == 0, s._L.svnicp_last_error(s.handle)
    n = s.get_target_normals()
    assert s.get_plane_stats(with_sums=False)[1] == 1
    M = tgt.shape[0]
    valid = (n != 0.0).any(axis=1)
    l2 = np.where(lam[:, 2] > 0, lam[:, 2], 1.0)
    near_thr = np.abs(lam[:, 1] / l2 - pr.MIN_RATIO) <= 1e-6 * pr.MIN_RATIO
    print(f"{name} normal_k {kn} knn {knn}: valid {valid.mean():.4f} (helper {ref_valid.mean():.4f}), at the threshold {near_thr.sum()}")
    assert near_thr.sum() <= 0.001 * M
    assert np.array_equal(valid[~near_thr], ref_valid[~near_thr])
    norm = np.linalg.norm(n[valid], axis=1)
    assert np.abs(norm - 1.0).max() <= 1e-12
    assert np.array_equal(n[~valid], np.zeros_like(n[~valid]))
    both = valid & ref_valid
    low_gap = both & ((lam[:, 1] - lam[:, 0]) / l2 < GAP_FLOOR)
    cmp = both & ~low_gap
    dev = 1.0 - np.abs((n[cmp] * ref_n[cmp]).sum(axis=1))
    print(f"  excluded for a small eigenvalue gap {low_gap.sum()} of {M}; max 1 - |n.n_ref| = {dev.max():.3e}")
    assert low_gap.sum() <= 0.02 * M
    assert dev.max() <= TIGHT


# ---------------------------------------------------------------------------------------------
# 2. solver parity with supplied normals
# ---------------------------------------------------------------------------------------------
PAR = dict(K=16, iterations=10, max_dist=0.3, delta=0.05)
STOP_THR = 0.03


@pytest.mark.parametrize("stop", [False, True], ids=["full", "earlystop"])
@pytest.mark.parametrize("full", [False, True], ids=["meanH", "fullgrad"])
@pytest.mark.parametrize("P,fused", [(1, False), (4, False), (4, True), (64, False), (130, False)],
                         ids=["P1", "P4", "P4fused", "P64", "P130"])
def test_solver_parity_with_supplied_normals(hip, orc, P, fused, full, stop):
    src, tgt = _clouds(0, "pair2k")
    nrm, _, _ = _ref_normals(orc, "pair2k", 16, False)
    init = hip.scans.make_particles(P, seed=3) * 0.2
    lr = 0.7 if full else 1.0
    ref = pr.run(orc, src, tgt, nrm, init, PAR["K"], PAR["iterations"], PAR["max_dist"], PAR["delta"], lr=lr, svn_full_grad=full,
                 check_early_stop=stop, convergence_threshold=STOP_THR, R0=R0, t0=T0)
    # the helper's own run shows the configuration exercises the gate, both Huber branches and (when on) the early stop
    res = np.abs(np.concatenate([np.concatenate(x) for x in ref.residuals]))
    outside = float((res > PAR["delta"]).mean())
    assert 0.05 <= outside <= 0.95, outside
    cand, _ = orc.knn_topk(orc.transform(src, R0, T0), tgt, PAR["K"])
    Rt, tt = pr.total_pose(orc, init[:, 0], R0, T0)
    _, ok_gate, _, _ = pr.pairs(src, tgt, nrm, cand, Rt, tt, PAR["max_dist"])
    _, ok_all, _, _ = pr.pairs(src, tgt, nrm, cand, Rt, tt, np.inf)
    assert ok_gate.sum() < ok_all.sum(), "max_dist must reject some pairs that have a normal"
    if stop:
        assert 1 < ref.iterations_run < PAR["iterations"], ref.iterations_run
    else:
        assert ref.iterations_run == PAR["iterations"]

    s = _solver(hip, src, tgt, init, K=PAR["K"], iterations=PAR["iterations"], max_dist=PAR["max_dist"], lr=lr, full=full, stop=stop,
                thr=STOP_THR, trace=True, residual="plane", delta=PAR["delta"], options=(("update", "fused"),) if fused else (),
                mean=(R0, T0))
    s.set_target_normals(nrm)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    assert s.get_plane_stats(with_sums=False)[1] == 0, "supplied normals: no normal pass"
    run = s.get_iterations_run()
    assert run == ref.iterations_run
    tr = s.get_trace()
    assert np.array_equal(tr["corr"][:run], ref.corr[:run])
    for k, r in (("H", ref.H), ("b", ref.b), ("newton", ref.newton), ("phi", ref.phi)):
        d = np.abs(tr[k][:run] - r[:run]).max()
        print(f"P {P} {k}: max |device - helper| = {d:.3e} (max |helper| {np.abs(r[:run]).max():.3e})")
        assert np.allclose(tr[k][:run], r[:run], rtol=TIGHT, atol=TIGHT), k
    assert np.allclose(tr["h"][:run], ref.h[:run], rtol=TIGHT, atol=TIGHT, equal_nan=True)
    assert np.abs(s.get_particles() - ref.particles).max() <= TIGHT
    assert np.abs(s.get_transformation() - ref.solver.get_transformation()).max() <= TIGHT
    assert np.abs(s.get_distribution() - ref.solver.get_distribution()).max() <= TIGHT
    assert np.abs(s.get_cov_matrix() - ref.solver.get_cov_matrix()).max() <= TIGHT
    stats, _ = s.get_plane_stats()
    assert np.array_equal(stats[:, 0], ref.stats[:, 0])
    assert np.allclose(stats[:, 1], ref.stats[:, 1], rtol=TIGHT, atol=TIGHT)


# ---------------------------------------------------------------------------------------------
# 3. estimated normals end to end
# ---------------------------------------------------------------------------------------------
def test_estimated_normals_end_to_end(hip, orc):
    """make_pair(4096, 8192), 8 particles, 10 iterations, K = 20, max_dist 1, delta 0.1, normal_k 16: the device with ITS
    normals against the helper with the helper's.  Bound 1e-6 (100x inside the project's 1e-4 bar): normals of points with a
    small eigenvalue gap differ by about 1e-15 / gap, so this is looser than TIGHT.
    Measured on an MI355X: mean pose 5.8e-15, particles 9.8e-14 from the helper's."""
    src, tgt = _clouds(0, "pair4k")
    nrm, _, _ = _ref_normals(orc, "pair4k", 16, False)
    init = hip.scans.make_particles(8)
    ref = pr.run(orc, src, tgt, nrm, init, 20, 10, 1.0, 0.1, lr=1.0, svn_full_grad=False)
    s = _solver(hip, src, tgt, init, K=20, iterations=10, residual="plane")
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    d = np.abs(s.get_transformation() - ref.solver.get_transformation()).max()
    dp = np.abs(s.get_particles() - ref.particles).max()
    print(f"estimated normals end to end: |mean pose device - helper| max = {d:.3e}, particles {dp:.3e}")
    assert d <= 1e-6


# ---------------------------------------------------------------------------------------------
# 4. behaviour
# ---------------------------------------------------------------------------------------------
def test_plane_mode_halves_the_pose_error_on_the_device(hip):
    """make_pair(16384, 32768), 30 particles, 20 iterations, K = 20, max_dist 1: the mean pose of plane mode (delta 0.1,
    normal_k 16) ends within half of point mode's error to true_pose, in translation and in rotation, both on the device."""
    pair = hip.scans.make_pair(16384, 32768)
    init = hip.scans.make_particles(30)
    err = {}
    for residual in ("point", "plane"):
        s = _solver(hip, pair.source, pair.target, init, K=20, iterations=20, residual=residual)
        assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
        err[residual] = pr.pose_error(s.get_transformation(), pair.true_pose)
    print(f"point mode {err['point'][0]:.4e} m {err['point'][1]:.4e} rad | plane mode {err['plane'][0]:.4e} m {err['plane'][1]:.4e} rad")
    assert err["plane"][0] <= 0.5 * err["point"][0] and err["plane"][1] <= 0.5 * err["point"][1]


# ---------------------------------------------------------------------------------------------
# 5. reuse of the normals
# ---------------------------------------------------------------------------------------------
def _outputs(s):
    return [s.get_particles(), s.get_transformation(), s.get_distribution(), s.get_cov_matrix(), s.get_particle_history()]


def test_normals_are_reused_until_the_target_or_normal_k_changes(hip):
    src, tgt = _clouds(0, "pair4k")
    init = hip.scans.make_particles(8)
    s = _solver(hip, src, tgt, init, K=20, iterations=5, residual="plane")
    s.stein_align()
    assert s.get_plane_stats(with_sums=False)[1] == 1
    dp = C.POINTER(C.c_double)
    s._check(s._L.svnicp_set_particles(s.handle, np.ascontiguousarray(init).ctypes.data_as(dp), 8), "svnicp_set_particles")
    s.stein_align()                                   # same target: no second pass …
    assert s.get_plane_stats(with_sums=False)[1] == 1
    fresh = _solver(hip, src, tgt, init, K=20, iterations=5, residual="plane")
    fresh.stein_align()
    for a, b in zip(_outputs(s), _outputs(fresh)):    # … and the result of a fresh context
        assert np.array_equal(a, b)
    s.set_residual("plane", 0.1, 12)                  # another normal_k
    s._check(s._L.svnicp_set_particles(s.handle, np.ascontiguousarray(init).ctypes.data_as(dp), 8), "svnicp_set_particles")
    s.stein_align()
    assert s.get_plane_stats(with_sums=False)[1] == 2
    s.add_cloud(src, tgt, init)                       # a new svnicp_set_target, even of the same points
    s.stein_align()
    assert s.get_plane_stats(with_sums=False)[1] == 3


# ---------------------------------------------------------------------------------------------
# 6. refusals and isolation
# ---------------------------------------------------------------------------------------------
def _refused(s, needle):
    rc = s._L.svnicp_align(s.handle)
    msg = s._L.svnicp_last_error(s.handle).decode()
    assert rc == ERR_INVALID, (rc, msg)
    assert needle in msg, msg


def test_plane_mode_refusals(hip):
    src, tgt = hip.scans.random_clouds(512, 2048, seed=3)
    init = hip.scans.make_particles(16, seed=3) * 0.2

    def plane(**kw):
        return _solver(hip, src, tgt, init, iterations=3, residual="plane", **kw)

    prm = hip.SteinICPParam(iterations=3, KNN_count=16, optimizer="Adam")
    g = hip.SVGDICP(prm, init)
    g.set_residual("plane")
    g.add_cloud(src, tgt, init)
    _refused(g, "SVGD")
    s = plane()
    assert s._L.svnicp_set_shard(s.handle, 0, 8) == 0
    rc = s._L.svnicp_align_begin(s.handle)
    assert rc == ERR_INVALID and "particle shard" in s._L.svnicp_last_error(s.handle).decode()
    s = plane()
    assert s._L.svnicp_set_row_shard(s.handle, 0, 2, 1024) == 0
    rc = s._L.svnicp_align_begin(s.handle)
    assert rc == ERR_INVALID and "row shard" in s._L.svnicp_last_error(s.handle).decode()
    s = plane()
    s.set_minibatch(64, 1)
    _refused(s, "mini-batch")
    _refused(plane(options=(("correspondence", "full"),)), "correspondence=full")
    _refused(plane(options=(("chain", "persistent"),)), "chain=persistent")
    _refused(plane(options=(("accum", "f64"),)), "accum")
    _refused(plane(options=(("accum", "valu"),)), "accum")
    _refused(plane(K=130), "knn_count")
    small = _solver(hip, src, tgt[:10], init, K=8, iterations=3, residual="plane", kn=16)
    _refused(small, "normal_k")
    s = plane()
    bad = np.zeros((tgt.shape[0] - 1, 3))
    assert s._L.svnicp_set_target_normals(s.handle, bad.ctypes.data_as(C.c_void_p), bad.shape[0], 0) == ERR_INVALID
    for args in ((2, 0.1, 16), (1, 0.0, 16), (1, -1.0, 16), (1, float("nan"), 16), (1, 0.1, 3), (1, 0.1, 65)):
        assert s._L.svnicp_set_residual(s.handle, *args) == ERR_INVALID, args
    assert s._L.svnicp_set_residual(s.handle, 1, float("inf"), 0) == 0
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS       # +inf: unweighted; normal_k 0 = 16
    assert np.isfinite(s.get_particles()).all()


def test_all_zero_normals_accept_nothing(hip):
    src, tgt = hip.scans.random_clouds(512, 2048, seed=3)
    init = hip.scans.make_particles(16, seed=3) * 0.2
    s = _solver(hip, src, tgt, init, iterations=3, residual="plane")
    s.set_target_normals(np.zeros_like(tgt))
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    stats, passes = s.get_plane_stats()
    assert passes == 0 and np.array_equal(stats, np.zeros_like(stats))
    assert np.isfinite(s.get_particles()).all() and np.isfinite(s.get_transformation()).all()
    assert np.array_equal(s.get_target_normals(), np.zeros_like(tgt))


@pytest.mark.parametrize("P", [1, 16, 130])
def test_point_residual_is_untouched(hip, P):
    """set_residual(POINT, ...) — also after a plane registration on the same context — leaves every output array equal to
    that of a context that never called it."""
    src, tgt = hip.scans.random_clouds(1024, 4096, seed=3)
    init = hip.scans.make_particles(P, seed=3) * 0.2

    def outputs(s):
        tr = s.get_trace()
        return _outputs(s) + [s.get_candidates(), tr["corr"], tr["H"], tr["b"], tr["newton"], tr["phi"], tr["h"]]

    plain = _solver(hip, src, tgt, init, iterations=6, trace=True)
    plain.stein_align()
    a = _solver(hip, src, tgt, init, iterations=6, trace=True, residual="point", delta=0.3, kn=8)
    a.stein_align()
    b = _solver(hip, src, tgt, init, iterations=6, trace=True, residual="plane")
    b.stein_align()
    b.set_residual("point", 0.1, 16)
    b.add_cloud(src, tgt, init)
    b.stein_align()
    for other in (a, b):
        for x, y in zip(outputs(plain), outputs(other)):
            assert np.array_equal(x, y, equal_nan=True)
