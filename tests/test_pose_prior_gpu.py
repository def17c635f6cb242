"""The Gaussian pose prior on the correction on the GPU (include/svnicp_hip.h "pose prior").

1. the kernel alone, in the manner of tests/test_stein_step_gpu.py: tiny clouds that are never searched, svnicp_align_begin,
   crafted sums (svnicp_sums_devptr) or a crafted plane record (svnicp_plane_record_devptr), the particles' correction poses
   read back through svnicp_particle_pose_devptr, ONE svnicp_iter_update, the trace H, b against the mpmath restatement at
   the bar E <= 16 max(E_f64, 2^-52) per particle and quantity, E_f64 the float64 restatement's error on the same inputs;
2. zero information is no prior: every array equal to a run without one under the same plan;
3. point mode, whole iterations through the split-phase calls (also mini-batch and correspondence=full);
4. plane mode, the degenerate scene of tests/test_pose_prior_cpu.py against its reference;
5. refusals, the setter between registrations, NULL, the getter, two runs bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import pose_prior_cases as cases
import pose_prior_reference as pref
import stein_step_reference as ss
from helpers import TIGHT

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
B0 = 256


def _T(R=None, t=None):
    T = np.eye(4)
    if R is not None:
        T[:3, :3] = R
    if t is not None:
        T[:3, 3] = t
    return T


def _dev(ptr, shape, dtype="<f8"):
    import torch
    from svnicp_amd.sharded import _DevView
    assert ptr, "null device pointer"
    return torch.as_tensor(_DevView(ptr, shape, dtype), device="cuda")


def _read(ptr, shape, dtype="<f8"):
    import torch
    torch.cuda.synchronize()
    return _dev(ptr, shape, dtype).cpu().numpy().copy()


def _write(ptr, arr):
    import torch
    _dev(ptr, arr.shape).copy_(torch.from_numpy(np.ascontiguousarray(arr, np.float64)))
    torch.cuda.synchronize()


def _solver(hip, src, tgt, init, *, K=8, iterations=2, max_dist=1.0, full=False, trace=True, options=(), mean=None, plane=None,
            normals=None, prior=None):
    prm = hip.SteinICPParam(iterations=iterations, lr=1.0, max_dist=max_dist, KNN_count=K, SVN_full_grad=full, record_trace=trace)
    s = hip.SVNICP(prm, init, hip.ParticleWeightOpt())
    for k, v in options:
        s.set_option(k, v)
    if plane is not None:
        s.set_residual("plane", plane, 16)
    s.add_cloud(src, tgt, init)
    if normals is not None:
        s.set_target_normals(normals)
    s.set_initial_mean(np.eye(4) if mean is None else mean)
    if prior is not None:
        s.set_pose_prior(*prior)
    return s


def _guard(hip, f, *a):
    """An error of the HIP runtime ends the session: nothing more is started on a device that has faulted."""
    try:
        return f(*a)
    except hip.SvnIcpError as e:
        pytest.exit("HIP error: %s" % e, returncode=3)


def _poses(s, P):
    L = s._L
    return _read(L.svnicp_particle_pose_devptr(s.handle, 0), (P, 9)), _read(L.svnicp_particle_pose_devptr(s.handle, 1), (P, 3))


def _bar(name, got_H, got_b, bases, R0, R, t, mean6, Lam, plane=False):
    """trace H, b of one iteration against the mpmath restatement, per particle and quantity."""
    Lf = None if Lam is None else np.asarray(Lam, np.float64).reshape(36)
    Hf, bf = pref.records(ss.F64(), bases, R0, R, t, mean6, Lf, plane)
    Hm, bm = pref.records(ss.MP(), bases, R0, R, t, mean6, Lf, plane)
    worst = 0.0
    for p in range(len(R)):
        for q, got, f64, mp_ in (("H", got_H[p], Hf[p], Hm[p]), ("b", got_b[p], bf[p], bm[p])):
            e, eo = pref.rel_err(got, mp_), pref.rel_err(f64, mp_)
            assert e is not None and eo is not None, "%s particle %d %s: the non-finite pattern differs\n%r\n%r" % (name, p, q, got, mp_)
            ratio = e / max(eo, pref.EPS)
            worst = max(worst, ratio)
            assert ratio <= pref.FACTOR, "%s particle %d %s: E_gpu %.3e is %.3g x max(E_f64 %.3e, 2^-52)" % (name, p, q, e, ratio, eo)
        Hp = np.asarray(got_H[p]).reshape(6, 6)
        if np.isfinite(Hp).all():
            assert np.array_equal(Hp, Hp.T), "%s particle %d: H is not exactly symmetric" % (name, p)
    print("%s: largest E_gpu / max(E_f64, 2^-52) = %.3g" % (name, worst))


@pytest.fixture(scope="module")
def tiny():
    g = np.arange(B0, dtype=np.float64)
    src = np.stack([g % 8, (g // 8) % 8, g // 64], 1) * 0.5
    return src, src + 0.01


# ---------------------------------------------------------------------------------------------
# 1. the kernel alone
# ---------------------------------------------------------------------------------------------
def _run_kernel_case(hip, tiny, P, options, lam, mean6, far, nan_p, plane):
    src, tgt = tiny
    init = cases.particles(P)
    Lam = cases.LAMBDAS[lam]()
    T = cases.far_mean() if far else np.eye(4)
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (B0, 1)) if plane else None
    s = _solver(hip, src, tgt, init, options=options, mean=T, plane=float("inf") if plane else None, normals=nrm, prior=(mean6, Lam))
    L = s._L
    s._check(L.svnicp_align_begin(s.handle), "svnicp_align_begin")
    s.synchronize()
    if plane:
        bases = cases.plane_records(P)
        _write(L.svnicp_plane_record_devptr(s.handle), bases)
    else:
        bases = cases.sums(P)
        _write(L.svnicp_sums_devptr(s.handle), bases)
    if nan_p is not None:
        R = _read(L.svnicp_particle_pose_devptr(s.handle, 0), (P, 9))
        R[nan_p, 4] = np.nan
        _write(L.svnicp_particle_pose_devptr(s.handle, 0), R)
    R, t = _poses(s, P)
    s._check(L.svnicp_iter_update(s.handle, 0), "svnicp_iter_update")
    s._check(L.svnicp_finish(s.handle), "svnicp_finish")
    s.synchronize()
    tr = s.get_trace(with_corr=False)
    if plane:   # the base record is never written in place
        assert np.array_equal(_read(L.svnicp_plane_record_devptr(s.handle), (P, 42)), bases)
    else:
        assert np.array_equal(_read(L.svnicp_sums_devptr(s.handle), (P, 22)), bases)
    s.close()
    return tr["H"][0].reshape(P, 36), tr["b"][0], bases, T[:3, :3].reshape(9), R, t, Lam


@pytest.mark.parametrize("name,P,options,lam,mean6,far,nan_p,plane", cases.KERNEL_CASES, ids=[c[0] for c in cases.KERNEL_CASES])
def test_kernel_alone(hip, tiny, name, P, options, lam, mean6, far, nan_p, plane):
    H, b, bases, R0, R, t, Lam = _guard(hip, _run_kernel_case, hip, tiny, P, options, lam, mean6, far, nan_p, plane)
    if nan_p is not None:
        assert np.isnan(H[nan_p]).all() and np.isnan(b[nan_p]).all(), "a non-finite pose gives a non-finite record"
        others = [p for p in range(P) if p != nan_p]
        assert np.isfinite(H[others]).all() and np.isfinite(b[others]).all(), "the other particles are unaffected"
    _bar(name, H, b, bases, R0, R, t, mean6, Lam, plane)
    if lam != "zero":   # the prior is in the trace: it differs from the base record alone
        H0, _ = pref.records(ss.F64(), bases, R0, R, t, mean6, None, plane)
        assert not np.allclose(H0[0], H[0], rtol=1e-12, atol=0)


def test_update_runs_twice_on_one_record(hip, tiny):
    """svnicp_iter_update may run more than once on one record (the Stein-step tests do): the second run adds the prior to
    the same base again, at the poses the first one left."""
    src, tgt = tiny
    P = 8
    init, Lam = cases.particles(P), cases.lam_full()
    s = _solver(hip, src, tgt, init, prior=(cases.MU_NONZERO, Lam))
    L = s._L
    s._check(L.svnicp_align_begin(s.handle), "svnicp_align_begin")
    s.synchronize()
    bases = cases.sums(P)
    _write(L.svnicp_sums_devptr(s.handle), bases)
    poses = []
    for it in range(2):
        poses.append(_poses(s, P))
        _guard(hip, s._check, L.svnicp_iter_update(s.handle, it), "svnicp_iter_update")
        s.synchronize()
    s._check(L.svnicp_finish(s.handle), "svnicp_finish")
    s.synchronize()
    tr = s.get_trace(with_corr=False)
    for it in range(2):
        _bar("twice-%d" % it, tr["H"][it].reshape(P, 36), tr["b"][it], bases, np.eye(3).reshape(9), poses[it][0], poses[it][1],
             cases.MU_NONZERO, Lam)
    assert not np.array_equal(poses[0][1], poses[1][1])


# ---------------------------------------------------------------------------------------------
# 2. zero information is no prior
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clouds(hip):
    return hip.scans.random_clouds(512, 2048, seed=3)


SAME_PLAN = (("chain", "general"), ("single", "split"))


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
@pytest.mark.parametrize("P", [1, 8, 64])
def test_zero_information_is_no_prior(hip, clouds, P, plane):
    src, tgt = clouds
    init = hip.scans.make_particles(P, seed=3) * 0.2
    outs = []
    for prior in (None, (cases.MU_NONZERO, np.zeros((6, 6)))):
        s = _solver(hip, src, tgt, init, K=16, iterations=3, options=SAME_PLAN, plane=0.1 if plane else None, prior=prior)
        assert _guard(hip, s.stein_align) == hip.SteinICPState.ALIGN_SUCCESS
        tr = s.get_trace()
        outs.append((tr["H"], tr["b"], tr["corr"], s.get_particles(), s.get_transformation(), s.get_cov_matrix()))
        s.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert np.isfinite(outs[0][3]).all()


# ---------------------------------------------------------------------------------------------
# 3. point mode, whole iterations
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,variant", [(8, "plain"), (64, "plain"), (64, "minibatch"), (8, "full")])
def test_point_mode_iterations(hip, clouds, P, variant):
    src, tgt = clouds
    init = hip.scans.make_particles(P, seed=3) * 0.2
    Lam, mean6 = cases.lam_full(), cases.MU_NONZERO * 0.5
    s = _solver(hip, src, tgt, init, K=16, iterations=3, options=(("correspondence", "full"),) if variant == "full" else (),
                prior=(mean6, Lam))
    if variant == "minibatch":
        s.set_minibatch(128, 7)
    L = s._L
    s._check(L.svnicp_align_begin(s.handle), "svnicp_align_begin")
    s._check(L.svnicp_stage_candidates(s.handle, 0, src.shape[0]), "svnicp_stage_candidates")
    s._check(L.svnicp_build_candidate_table(s.handle), "svnicp_build_candidate_table")
    sums, poses = [], []
    for it in range(3):
        _guard(hip, s._check, L.svnicp_iter_accumulate(s.handle, it), "svnicp_iter_accumulate")
        s.synchronize()
        sums.append(_read(L.svnicp_sums_devptr(s.handle), (P, 22)))
        poses.append(_poses(s, P))
        tot = _read(L.svnicp_total_pose_devptr(s.handle), (P, 12))
        assert np.array_equal(tot[:, :9], poses[-1][0]) and np.array_equal(tot[:, 9:], poses[-1][1])   # R0 = I, t0 = 0
        _guard(hip, s._check, L.svnicp_iter_update(s.handle, it), "svnicp_iter_update")
    s._check(L.svnicp_finish(s.handle), "svnicp_finish")
    s.synchronize()
    tr = s.get_trace(with_corr=False)
    assert sums[0][:, 0].min() > 10.0, "the iterations matched points"
    for it in range(3):
        _bar("%s-P%d-it%d" % (variant, P, it), tr["H"][it].reshape(P, 36), tr["b"][it], sums[it], np.eye(3).reshape(9), poses[it][0],
             poses[it][1], mean6, Lam)
    s.close()


# ---------------------------------------------------------------------------------------------
# 4. plane mode, the degenerate scene
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_reference(orc):
    src, tgt, nrm = cases.plane_scene()
    return {P: pref.run_scene(orc, src, tgt, nrm, cases.scene_particles(P), cases.SCENE_K, cases.SCENE_ITERS, 1.0, float("inf"),
                              cases.SCENE_MU, cases.scene_lambda()) for P in (1, 64)}


def _scene(hip, P, prior):
    src, tgt, nrm = cases.plane_scene()
    s = _solver(hip, src, tgt, cases.scene_particles(P), K=cases.SCENE_K, iterations=cases.SCENE_ITERS, plane=float("inf"), normals=nrm,
                prior=(cases.SCENE_MU, cases.scene_lambda()) if prior else None)
    assert _guard(hip, s.stein_align) == hip.SteinICPState.ALIGN_SUCCESS
    return s


@pytest.mark.parametrize("P", [1, 64])
def test_plane_scene_against_the_reference(hip, scene_reference, P):
    ref = scene_reference[P]
    s = _scene(hip, P, True)
    tr = s.get_trace()
    assert np.array_equal(tr["corr"], ref.corr)
    for k, r in (("H", ref.H), ("b", ref.b)):
        d = np.abs(tr[k] - r).max()
        print("P %d %s: max |device - reference| = %.3e (max |reference| %.3e)" % (P, k, d, np.abs(r).max()))
        assert np.allclose(tr[k], r, rtol=TIGHT, atol=TIGHT), k
    assert np.abs(s.get_particles() - ref.particles).max() <= TIGHT
    assert np.abs(s.get_transformation() - ref.solver.get_transformation()).max() <= TIGHT
    assert np.abs(s.get_cov_matrix() - ref.solver.get_cov_matrix()).max() <= TIGHT
    if P == 1:
        x = s.get_particles().reshape(6)
        print("P = 1 with prior: pose - mu =", x - cases.SCENE_MU)
        assert np.abs(x - cases.SCENE_MU).max() < 1e-6
        c = _scene(hip, 1, False)
        xc = c.get_particles().reshape(6)
        print("P = 1 without prior: pose =", xc)
        assert np.linalg.norm(xc[:2] - cases.SCENE_MU[:2]) > 0.1
        c.close()
    s.close()


# ---------------------------------------------------------------------------------------------
# 5. interface behaviour
# ---------------------------------------------------------------------------------------------
def _refused(s, needle):
    rc = s._L.svnicp_align(s.handle)
    msg = s._L.svnicp_last_error(s.handle).decode()
    assert rc == ERR_INVALID, (rc, msg)
    assert msg.startswith("svnicp_align: the pose prior (svnicp_set_pose_prior) is not available here: ") and needle in msg, msg


def test_refusals(hip, clouds):
    src, tgt = clouds
    init = hip.scans.make_particles(16, seed=3) * 0.2
    prior = (np.zeros(6), cases.lam_diag())
    g = hip.SVGDICP(hip.SteinICPParam(iterations=3, KNN_count=16, optimizer="Adam"), init)
    g.add_cloud(src, tgt, init)
    g.set_pose_prior(*prior)
    _refused(g, "SVGD mode")
    with pytest.raises(hip.SvnIcpError, match="SVGD mode"):
        g.stein_align()
    g.set_pose_prior(None, None)
    assert g.stein_align() == hip.SteinICPState.ALIGN_SUCCESS      # off again: the refusal is gone
    s = _solver(hip, src, tgt, init, K=16, prior=prior)
    assert s._L.svnicp_set_shard(s.handle, 0, 8) == 0
    assert s._L.svnicp_align_begin(s.handle) == ERR_INVALID and "a partial particle shard" in s._L.svnicp_last_error(s.handle).decode()
    s = _solver(hip, src, tgt, init, K=16, prior=prior)
    assert s._L.svnicp_set_row_shard(s.handle, 0, 2, 1024) == 0
    assert s._L.svnicp_align_begin(s.handle) == ERR_INVALID and "a source-row shard" in s._L.svnicp_last_error(s.handle).decode()
    _refused(_solver(hip, src, tgt, init, K=16, options=(("chain", "persistent"),), prior=prior), "chain=persistent")
    # the setter's own refusals leave the prior as it was
    s = _solver(hip, src, tgt, init, K=16, prior=prior)
    dp = C.POINTER(C.c_double)
    bad = cases.lam_diag(); bad[0, 1] = 1.0
    m = np.zeros(6)
    assert s._L.svnicp_set_pose_prior(s.handle, m.ctypes.data_as(dp), bad.ctypes.data_as(dp)) == ERR_INVALID
    assert "not symmetric" in s._L.svnicp_last_error(s.handle).decode()
    bad = cases.lam_diag(); bad[2, 2] = np.nan
    assert s._L.svnicp_set_pose_prior(s.handle, m.ctypes.data_as(dp), bad.ctypes.data_as(dp)) == ERR_INVALID
    m[3] = np.pi
    good = cases.lam_diag()
    assert s._L.svnicp_set_pose_prior(s.handle, m.ctypes.data_as(dp), good.ctypes.data_as(dp)) == ERR_INVALID
    got = s.pose_prior()
    assert got is not None and np.array_equal(got[0], prior[0]) and np.array_equal(got[1], prior[1])


@pytest.mark.parametrize("P", [1, 16])
def test_setter_between_registrations(hip, clouds, P):
    src, tgt = clouds
    init = hip.scans.make_particles(P, seed=3) * 0.2

    def run(s):
        s.add_cloud(src, tgt, init)
        assert _guard(hip, s.stein_align) == hip.SteinICPState.ALIGN_SUCCESS
        tr = s.get_trace()
        return [s.get_particles(), s.get_transformation(), s.get_cov_matrix(), tr["H"], tr["b"], tr["corr"]]

    s = _solver(hip, src, tgt, init, K=16, iterations=4)
    assert s.pose_prior() is None
    plain = run(s)
    Lam = cases.lam_full() * 20.0
    asym = Lam.copy(); asym[0, 1] += 1e-13 * np.abs(Lam).max(); asym[1, 0] -= 1e-13 * np.abs(Lam).max()
    s.set_pose_prior(cases.MU_NONZERO, asym)
    m, got = s.pose_prior()
    assert np.array_equal(m, cases.MU_NONZERO) and np.array_equal(got, got.T) and np.allclose(got, Lam, rtol=1e-12, atol=0)
    with_prior = run(s)
    again = run(s)
    for a, b in zip(with_prior, again):
        assert np.array_equal(a, b), "two runs with the same prior are bit-identical"
    assert not np.array_equal(with_prior[0], plain[0])
    d_plain = np.linalg.norm(plain[1] - cases.MU_NONZERO)
    d_prior = np.linalg.norm(with_prior[1] - cases.MU_NONZERO)
    print("P %d: |mean - mu| without prior %.4f, with %.4f" % (P, d_plain, d_prior))
    assert d_prior < d_plain
    s.set_pose_prior(None, None)
    assert s.pose_prior() is None
    off = run(s)
    for a, b in zip(plain, off):
        assert np.array_equal(a, b), "NULL turns the prior off: the launches of a context that never set one"
    s.close()


def test_weighting_and_update_fused_with_prior(hip, clouds):
    """Allowed combinations run: particle weighting and option update=fused."""
    src, tgt = clouds
    init = hip.scans.make_particles(16, seed=3) * 0.2
    prior = (np.zeros(6), cases.lam_diag())
    s = _solver(hip, src, tgt, init, K=16, iterations=4, prior=prior)
    s.set_particle_weighting("softmin", 0.5, 1.0)
    assert _guard(hip, s.stein_align) == hip.SteinICPState.ALIGN_SUCCESS
    w = s.get_particle_weight()
    assert np.isfinite(w).all() and abs(w.sum() - 1.0) < 1e-12
    f = _solver(hip, src, tgt, init, K=16, iterations=4, options=(("update", "fused"),), prior=prior)
    assert _guard(hip, f.stein_align) == hip.SteinICPState.ALIGN_SUCCESS
    g = _solver(hip, src, tgt, init, K=16, iterations=4, prior=prior)
    assert _guard(hip, g.stein_align) == hip.SteinICPState.ALIGN_SUCCESS
    assert np.abs(f.get_particles() - g.get_particles()).max() < 1e-9     # two launch shapes of the same step
