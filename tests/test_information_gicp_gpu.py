"""svnicp_eval_information_gicp on the device (csrc/information.hip, k_information_pairs<gicp>) against
tests/information_gicp_reference.py, the numpy restatement of the header's GICP form.  P = 4, K = 16, 3 iterations unless a case
says otherwise.

Tolerances are those of tests/test_information_gpu.py: pairs is exact, every entry of H and b lies within TIGHT = 1e-9 of A (the
sum of the entry's absolute terms, with |W|'s entries), and everything svnicp_information_solve derives is bit for bit what the
same routine gives on the host for the returned sums.  Both sides form W by the same cofactor expression; its own error, a few
cond(S) u <= 1.2e-10 at epsilon = 1e-6, is inside TIGHT (tests/test_information_gicp_cpu.py measures it against mpmath).  The
restatement is fed the normals as the context holds them (the getters), so no rounding of the upload's normalisation enters."""
import ctypes as C

import numpy as np
import pytest

import evaluate_cases as ec
import evaluate_reference as er
import information_gicp_reference as igr
import nonfinite_reference as nf
import plane_reference as pr
from test_evaluate_gpu import P_, _case, _param, _registered, _same, _snapshot
from test_information_gpu import _bits, _check, _unit_rows

pytestmark = pytest.mark.gpu

INF = float("inf")
DELTAS = (0.1, INF)
EPSILONS = (1e-3, 1e-6, 1.0)
_SRC_NORMALS = {}


def _source_normals(orc, name, src):
    """Normals of a shared case's source from 16 neighbours, every eleventh row bare: computed once per session."""
    if name not in _SRC_NORMALS:
        n = pr.normals(orc, src, 16)[0].copy()
        n[::11] = 0.0
        _SRC_NORMALS[name] = n
    return _SRC_NORMALS[name]


def _with_normals(hip, orc, cloud, knn="auto", **kw):
    src, tgt, poses, nrm = _case(hip, orc, cloud)
    s = _registered(hip, src, tgt, knn, **kw)
    s.set_target_normals(nrm)
    s.set_source_normals(_source_normals(orc, cloud, src))
    return s, src, tgt, poses


def _raw(s, delta=0.1, eps=1e-3, floor=0.0, struct_size=None):
    from svnicp_amd.binding import InformationStruct
    o = InformationStruct()
    o.struct_size = C.sizeof(InformationStruct) if struct_size is None else struct_size
    rc = s._L.svnicp_eval_information_gicp(s._h, float(delta), float(eps), float(floor), C.byref(o))
    return rc, s._L.svnicp_last_error(s._h).decode(), o


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("knn", ["auto", "tiles"])
@pytest.mark.parametrize("cloud", ec.CLOUDS)
def test_gicp_information_agrees_with_the_restatement(hip, orc, cloud, knn):
    """Two poses (NULL = the registration's own result), Huber delta 0.1 and +inf, epsilon 1e-3, 1e-6 and 1, gate 0.3, supplied
    normals of both clouds."""
    s, src, tgt, poses = _with_normals(hip, orc, cloud, knn)
    nt, ns = s.get_target_normals(), s.get_source_normals()
    for pose_name in ("null", "true_pose"):
        ev = s.evaluate(0.3, None if pose_name == "null" else poses[pose_name])
        T = ev.pose
        if pose_name == "null":      # this pose is not among the ones checked on the CPU: check it here
            near_gate, tie = er.preconditions(er.evaluate(orc, src, tgt, T, 0.3, with_second=True), 0.3)
            assert near_gate.size == 0 and tie.size == 0
        ref = er.evaluate(orc, src, tgt, T, 0.3, normals=nt)
        for delta in DELTAS:
            for eps in EPSILONS:
                got = s.information("gicp", delta, gicp_epsilon=eps)
                assert np.array_equal(got.pose, T)
                want = igr.sums(orc, src, tgt, T, 0.3, delta, eps, nt, ns, ev=ref)
                _check(hip, got, want, f"{cloud} {knn} {pose_name} delta {delta} eps {eps:g}", 0.3, delta)
                assert 0 < got.pairs < ev.plane_inliers           # some source rows are bare


@pytest.mark.parametrize("B,M", [(1, 1), (70, 64), (257, 300)])
def test_gicp_information_edges(hip, orc, B, M):
    """One row; a partial wave past 64; one row past the 256-row workgroup.  One target row and several source rows are bare."""
    src, tgt = hip.scans.random_clouds(B, M, seed=7)
    nt = _unit_rows(M, 11)
    ns = _unit_rows(B, 13)
    if B > 2:
        ns[[0, B // 2, B - 1]] = 0.0
    s = _registered(hip, src, tgt)
    s.set_target_normals(nt)
    s.set_source_normals(ns)
    ev = s.evaluate(1.0, np.eye(4))
    nt_held, ns_held = s.get_target_normals(), s.get_source_normals()
    for eps in EPSILONS:
        got = s.information("gicp", 0.1, gicp_epsilon=eps)
        want = igr.sums(orc, src, tgt, ev.pose, 1.0, 0.1, eps, nt_held, ns_held)
        _check(hip, got, want, f"B {B} M {M} eps {eps:g}", 1.0, 0.1)
    assert got.pairs <= ev.plane_inliers
    if B > 2:
        assert 0 < got.pairs and not want.rows[[0, B // 2, B - 1]].any()


# ------------------------------------------------------------------------------------------------ non-finite
@pytest.mark.parametrize("nan_target_0", [False, True])
def test_gicp_information_with_nonfinite_rows_and_normals(hip, orc, nan_target_0):
    """The poisoned clouds of the evaluate tests, and source normals poisoned the same way on those rows and on others: such
    rows reach no sum, the counts are exact, every output is finite."""
    src, tgt, poses, nrm = _case(hip, orc, "random")
    src_rows, tgt_rows, nrm_rows = [3, 64, 65, 700, 1023, 2047], [5, 511, 512, 4000, 8191], [3, 7, 255, 256, 1500]
    kinds = ("nan1", "+inf", "big64")
    src_b, tgt_b = nf.poison(src, src_rows, kinds), nf.poison(tgt, tgt_rows, kinds)
    ns_b = nf.poison(_source_normals(orc, "random", src), nrm_rows, ("nan1", "+inf", "nan3"))
    if nan_target_0:
        tgt_b = nf.poison(tgt_b, [0], "nan1")
    s = _registered(hip, src_b, tgt_b)
    s.set_target_normals(nrm)
    s.set_source_normals(ns_b)
    nt_held, ns_held = s.get_target_normals(), s.get_source_normals()
    assert not ns_held[nrm_rows].any() and np.isfinite(ns_held).all()        # a non-finite normal is "no normal here"
    T = poses["true_pose"]
    for gate in (0.3, INF):
        ev = s.evaluate(gate, T)
        ref = er.evaluate(orc, src_b, tgt_b, T, gate, normals=nt_held, finite=False)
        got = s.information("gicp", 0.1)
        want = igr.sums(orc, src_b, tgt_b, T, gate, 0.1, 1e-3, nt_held, ns_held, finite=False, ev=ref)
        _check(hip, got, want, f"non-finite target0 {nan_target_0} gate {gate}", gate, 0.1)
        assert 0 < got.pairs <= ev.evaluated - 2 and not want.rows[src_rows].any() and not want.rows[nrm_rows].any()


# ------------------------------------------------------------------------------------------------ the solver's own normals
def test_gicp_information_with_the_normals_the_solver_estimated(hip, orc):
    src, tgt, poses, _ = _case(hip, orc, "random")
    s = _registered(hip, src, tgt, residual="gicp")
    ev = s.evaluate(0.3, poses["true_pose"])
    assert ev.has_normals
    nt, ns = s.get_target_normals(), s.get_source_normals()
    assert (nt != 0).any(axis=1).sum() > 1000 and (ns != 0).any(axis=1).sum() > 1000
    got = s.information("gicp", 0.1)                       # epsilon: the solver's own, SteinICPParam.gicp_epsilon
    want = igr.sums(orc, src, tgt, ev.pose, 0.3, 0.1, s.config.gicp_epsilon, nt, ns)
    _check(hip, got, want, "estimated normals", 0.3, 0.1)
    assert got.pairs > 0


# ------------------------------------------------------------------------------------------------ stationarity
def test_step_is_smallest_in_the_objective_the_solver_minimised(hip):
    """What the form exists for.  One particle, GICP mode, 100 iterations with 100 candidates on scans.make_pair(2048, 8192):
    at the solver's own result, with its delta, epsilon and gate, the Gauss-Newton step of the GICP form is smaller than the
    plane form's and the point form's at the same pose.  The restatements on the CPU give, for this registration,
    |step| = 7.8e-13 (gicp), 8.4e-2 (plane), 1.8e-2 (point); no absolute threshold is set."""
    p = hip.scans.make_pair(2048, 8192)
    init = np.zeros((6, 1))
    prm = _param(hip, iterations=100, KNN_count=100, residual="gicp", huber_delta=0.1, normal_k=16, gicp_epsilon=1e-3)
    s = hip.SVNICP(prm, init, hip.ParticleWeightOpt())
    s.add_cloud(p.source, p.target, init)
    s.set_initial_mean(np.eye(4))
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    s.evaluate(1.0)                                        # the solver's gate: d2 < max_dist = 1
    step = {f: float(np.linalg.norm(s.information(f, 0.1).step)) for f in ("gicp", "plane", "point")}
    print(f"|step| at the GICP registration's own result: {step}")
    assert step["gicp"] < step["plane"] and step["gicp"] < step["point"]


# ------------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def ready(hip, orc):
    """A context with normals of both clouds and an evaluate: every call with good arguments succeeds."""
    s, src, tgt, poses = _with_normals(hip, orc, "ragged")
    s.evaluate(0.3, np.eye(4))
    return s, src, tgt


def test_refused_without_an_evaluate(hip, orc):
    s, *_ = _with_normals(hip, orc, "ragged")
    rc, msg, _ = _raw(s)
    assert rc == -1 and "svnicp_eval_information_gicp" in msg and "no svnicp_evaluate yet" in msg


def test_refused_after_an_evaluate_without_normals(hip, orc):
    src, tgt, _, _ = _case(hip, orc, "ragged")
    s = _registered(hip, src, tgt)
    s.set_source_normals(_source_normals(orc, "ragged", src))
    assert not s.evaluate(0.3, np.eye(4)).has_normals
    rc, msg, _ = _raw(s)
    assert rc == -1 and "has_normals = 0" in msg


def test_refused_without_source_normals(hip, orc):
    src, tgt, _, nrm = _case(hip, orc, "ragged")
    s = _registered(hip, src, tgt)
    s.set_target_normals(nrm)
    assert s.evaluate(0.3, np.eye(4)).has_normals
    rc, msg, _ = _raw(s)
    assert rc == -1 and "no normals of the current source" in msg
    s.set_source_normals(_source_normals(orc, "ragged", src))      # the rows do not depend on them: no new evaluate is needed
    assert _raw(s)[0] == 0


def test_refused_after_the_source_was_replaced(hip, orc):
    s, src, tgt, _ = _with_normals(hip, orc, "ragged")
    s.evaluate(0.3, np.eye(4))
    assert _raw(s)[0] == 0
    s._check(s._L.svnicp_set_source(s._h, np.ascontiguousarray(src).ctypes.data_as(C.c_void_p), len(src), 0), "svnicp_set_source")
    rc, msg, _ = _raw(s)
    assert rc == -1 and "the source changed" in msg
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    s.evaluate(0.3, np.eye(4))
    rc, msg, _ = _raw(s)                                    # the new source came without normals
    assert rc == -1 and "no normals of the current source" in msg


def test_refused_epsilon_outside_the_range(ready):
    s = ready[0]
    for eps in (0.9e-6, 1.0000001, -1e-3, float("nan"), INF):
        rc, msg, _ = _raw(s, eps=eps)
        assert rc == -1 and "epsilon" in msg, eps
    for eps in (0.0, 1e-6, 1.0):
        assert _raw(s, eps=eps)[0] == 0, eps
    a, b = _raw(s, eps=0.0)[2], _raw(s, eps=1e-3)[2]         # 0 means 1e-3
    assert bytes(a) == bytes(b)


def test_refused_huber_delta_not_positive(ready):
    s = ready[0]
    for delta in (0.0, -1.0, float("nan")):
        rc, msg, _ = _raw(s, delta=delta)
        assert rc == -1 and "huber_delta" in msg, delta
    assert _raw(s, delta=INF)[0] == 0


def test_refused_floor_outside_zero_one(ready):
    s = ready[0]
    for floor in (1.0, -0.1, float("nan")):
        rc, msg, _ = _raw(s, floor=floor)
        assert rc == -1 and "eig_floor_ratio" in msg, floor
    assert _raw(s, floor=0.5)[0] == 0


def test_refused_wrong_struct_size(ready):
    rc, msg, _ = _raw(ready[0], struct_size=8)
    assert rc == -1 and "struct_size" in msg


def test_form_three_stays_unknown_to_the_old_entry_point(ready):
    from svnicp_amd.binding import InformationStruct, INFO_GICP
    s = ready[0]
    o = InformationStruct()
    o.struct_size = C.sizeof(InformationStruct)
    rc = s._L.svnicp_eval_information(s._h, INFO_GICP, 0.1, 0.0, C.byref(o))
    msg = s._L.svnicp_last_error(s._h).decode()
    assert rc == -1 and "unknown form" in msg and "svnicp_eval_information_gicp" in msg
    rc, _, o = _raw(s)
    assert rc == 0 and o.form == INFO_GICP == 3


# ------------------------------------------------------------------------------------------------ leaves everything alone
def _snapshot_gicp(s):
    d = _snapshot(s, False, True)
    stats, passes = s.get_gicp_stats()
    d.update(gicp_stats=stats, passes=np.array(passes), normals=s.get_target_normals(), source_normals=s.get_source_normals())
    return d


def test_gicp_information_is_repeatable_and_changes_nothing(hip, orc):
    src, tgt, poses, _ = _case(hip, orc, "random")
    kw = dict(record_trace=True, residual="gicp")
    s = _registered(hip, src, tgt, "tiles", **kw)
    s.evaluate(0.3, poses["true_pose"])
    before, pairs_before = _snapshot_gicp(s), s.get_eval_pairs()
    first = s.information("gicp", 0.1)
    _same(before, _snapshot_gicp(s))
    second = s.information("gicp", 0.1)
    _same(before, _snapshot_gicp(s))
    assert _bits(first) == _bits(second) and first.pairs > 0
    pairs_after = s.get_eval_pairs()
    assert pairs_before[0].tobytes() == pairs_after[0].tobytes() and pairs_before[1].tobytes() == pairs_after[1].tobytes()
    # the next registration: bit for bit that of a context that never asked
    init = hip.scans.make_particles(P_, seed=3) * 0.2
    fresh = _registered(hip, src, tgt, "tiles", **kw)
    for ctx in (s, fresh):
        ctx.add_cloud(src, tgt, init)
        assert ctx.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    a, b = _snapshot_gicp(s), _snapshot_gicp(fresh)
    a.pop("gpu_ms"); b.pop("gpu_ms")          # elapsed time of two different runs
    _same(a, b)


# ------------------------------------------------------------------------------------------------ pipeline
def test_python_pipeline_reports_the_gicp_information(hip):
    """Two scans of the evaluate tests' drive, residual = information = "gicp": the second scan's ScanResult.information is
    what a direct call at its result pose gives."""
    pl, sc = hip.pipeline, hip.scans
    P, I, K, voxel = 24, 12, 40, 0.5
    scene = sc.make_scene()
    rng = np.random.default_rng(11)
    cfg = pl.PipelineConfig(min_range=1.0, max_range=80.0, voxel_size=voxel, map_voxel_size=voxel, map_voxel_max_points=20,
                            map_range=100.0, particle_count=P, gpu_map=True, map_normals=True, eval_dist=0.5, information="gicp", info_huber=0.1,
                            solver=hip.SteinICPParam(iterations=I, lr=1.0, max_dist=1.0, KNN_count=K, SVN_full_grad=False, residual="gicp"))
    pipe = pl.RegistrationPipeline(cfg, device=0)
    parts = [hip.initialize_particles(P, pl.PRIOR_UB, pl.PRIOR_LB, rng) for _ in range(2)]
    it = iter(parts)
    pipe._particles = lambda: next(it)
    for k in range(2):
        t = np.array([0.0, 0.0, 0.05 * k]); R = sc.rot_zyx(0.0, 0.0, np.radians(0.3 * k))
        res = pipe.process_scan(sc.lidar_scan(scene, R, t, 16384, stream=700 + k).astype(np.float32), 0.1 * k)
        if k == 0:
            assert res.information is None
    info = res.information
    assert info is not None and info.form == "gicp" and info.huber_delta == 0.1 and 0 < info.pairs <= res.plane_inliers
    pipe._solver.evaluate(0.5, res.pose)                 # the context still holds this scan's clouds
    assert _bits(pipe._solver.information("gicp", 0.1)) == _bits(info)
