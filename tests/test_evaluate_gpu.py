"""svnicp_evaluate on the device (csrc/evaluate.hip) against tests/evaluate_reference.py, the numpy
restatement of include/svnicp_hip.h "evaluate a registration".  P = 4, K = 16, 3 iterations unless a case says otherwise.

Tolerances: the index array and the four counts are exact (tests/test_evaluate_cpu.py checks that no row of these clouds sits
on the gate or has two nearest targets within 1e-12); d2 is the same unfused float64 expression on both sides and the sums
differ by the order of at most 2048 additions, all inside TIGHT = 1e-9 relative; fitness is one correctly rounded division
and the RMSEs one division and one square root of the returned sums, compared exactly."""
import ctypes as C
import dataclasses
import os
import struct
import subprocess

import numpy as np
import pytest

from helpers import TIGHT

import evaluate_cases as ec
import evaluate_reference as er
import nonfinite_reference as nf
import plane_reference as pr

pytestmark = pytest.mark.gpu

P_, K_, I_ = 4, 16, 3


def _param(hip, **kw):
    base = dict(iterations=I_, lr=1.0, max_dist=1.0, KNN_count=K_, SVN_full_grad=False)
    base.update(kw)
    return hip.SteinICPParam(**base)


def _registered(hip, src, tgt, knn="auto", T0=None, **kw):
    init = hip.scans.make_particles(P_, seed=3) * 0.2
    s = hip.SVNICP(_param(hip, **kw), init, hip.ParticleWeightOpt())
    if knn != "auto":
        s.set_option("knn", knn)
    s.add_cloud(src, tgt, init)
    s.set_initial_mean(np.eye(4) if T0 is None else T0)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    return s


_CASES = {}


def _case(hip, orc, name):
    """(source, target, poses, normals of the target) of a shared case: computed once per session."""
    if name not in _CASES:
        src, tgt, poses = ec.clouds(hip, name)
        _CASES[name] = (src, tgt, poses, pr.normals(orc, tgt, 16)[0])
    return _CASES[name]


def _rel(a, b):
    return abs(a - b) <= TIGHT * max(abs(a), abs(b))


def _check(got, pairs, want, label):
    idx, d2 = pairs
    assert np.array_equal(idx.astype(np.int64), want.index), label
    ok = want.index >= 0
    assert np.isnan(d2[~ok]).all() and np.allclose(d2[ok], want.d2[ok], rtol=TIGHT, atol=0), label
    print(f"{label}: evaluated {got.evaluated} inliers {got.inliers} plane {got.plane_inliers} fitness {got.fitness:.6f} "
          f"rmse {got.inlier_rmse:.6f} plane rmse {got.plane_rmse:.6f} | sums {got.sum_d2!r} {want.sum_d2!r} {got.sum_r2!r} {want.sum_r2!r}")
    assert (got.has_normals, got.rows, got.evaluated, got.inliers, got.plane_inliers) == \
           (want.has_normals, want.rows, want.evaluated, want.inliers, want.plane_inliers), label
    assert _rel(got.sum_d2, want.sum_d2) and _rel(got.sum_r2, want.sum_r2), label
    assert not np.isnan([got.sum_d2, got.sum_r2, got.fitness, got.inlier_rmse, got.plane_rmse]).any(), label
    assert got.fitness == got.inliers / got.rows, label
    assert got.inlier_rmse == (np.sqrt(got.sum_d2 / got.inliers) if got.inliers else 0.0), label
    assert got.plane_rmse == (np.sqrt(got.sum_r2 / got.plane_inliers) if got.plane_inliers else 0.0), label


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("knn", ["auto", "brute", "tiles"])
@pytest.mark.parametrize("cloud", ec.CLOUDS)
def test_evaluate_agrees_with_the_restatement(hip, orc, cloud, knn):
    """Every stage-A kernel family, three poses (NULL = the registration's own result), two gates, without and with
    supplied normals.  M = 3000 is below the tile kernel's range: knn=tiles runs the streaming kernel there."""
    src, tgt, poses, nrm = _case(hip, orc, cloud)
    T0 = hip.pipeline.correction_to_pose([0.01, -0.02, 0.005, 0.001, 0.002, -0.001])   # a non-trivial initial mean for NULL
    s = _registered(hip, src, tgt, knn, T0=T0)
    want_null = T0 @ hip.pipeline.correction_to_pose(s.get_transformation())
    for normals in (None, nrm):
        if normals is not None:
            s.set_target_normals(normals)
        for pose_name in ("null", "identity", "true_pose"):
            for gate in ec.GATES:
                got = s.evaluate(gate, None if pose_name == "null" else poses[pose_name])
                T = got.pose
                if pose_name == "null":
                    assert np.allclose(T, want_null, rtol=0, atol=TIGHT)
                else:
                    assert np.array_equal(T, poses[pose_name])
                want = er.evaluate(orc, src, tgt, T, gate, normals=normals)
                if pose_name == "null":      # this pose is not among the ones checked on the CPU: check it here
                    near_gate, tie = er.preconditions(er.evaluate(orc, src, tgt, T, gate, with_second=True), gate)
                    assert near_gate.size == 0 and tie.size == 0
                _check(got, s.get_eval_pairs(), want, f"{cloud} {knn} {pose_name} gate {gate} normals {normals is not None}")
    assert s.eval_index_ptr != 0 and s.eval_dist2_ptr != 0


@pytest.mark.parametrize("B,M", [(1, 1), (70, 64)])
def test_evaluate_edges(hip, orc, B, M):
    src, tgt = hip.scans.random_clouds(B, M, seed=7)
    s = _registered(hip, src, tgt)
    for pose in (None, np.eye(4)):
        got = s.evaluate(1.0, pose)
        _check(got, s.get_eval_pairs(), er.evaluate(orc, src, tgt, got.pose, 1.0), f"B {B} M {M}")
        assert got.evaluated == B


# ------------------------------------------------------------------------------------------------ non-finite
@pytest.mark.parametrize("knn", ["auto", "tiles"])
@pytest.mark.parametrize("nan_target_0", [False, True])
def test_evaluate_with_nonfinite_and_huge_rows(hip, orc, knn, nan_target_0):
    src, tgt, poses, _ = _case(hip, orc, "random")
    src_rows, tgt_rows = [3, 64, 65, 700, 1023, 2047], [5, 511, 512, 4000, 8191]
    kinds = ("nan1", "+inf", "big64")
    src_b, tgt_b = nf.poison(src, src_rows, kinds), nf.poison(tgt, tgt_rows, kinds)
    if nan_target_0:
        tgt_b = nf.poison(tgt_b, [0], "nan1")
    s = _registered(hip, src_b, tgt_b, knn)
    T = poses["true_pose"]
    for gate in (0.3, float("inf")):
        got = s.evaluate(gate, T)
        want = er.evaluate(orc, src_b, tgt_b, T, gate, finite=False)
        _check(got, s.get_eval_pairs(), want, f"non-finite {knn} target0 {nan_target_0} gate {gate}")
        # NaN and inf source rows are not evaluated; the 1e160 rows are (d2 = +inf: never an inlier, even with an infinite gate)
        assert got.evaluated == want.evaluated == len(src) - 4 and got.inliers <= got.evaluated - 2


# ------------------------------------------------------------------------------------------------ after an early stop
def test_evaluate_after_an_early_stop(hip, orc):
    src, tgt, poses, nrm = _case(hip, orc, "random")
    s = _registered(hip, src, tgt, iterations=6, check_early_stop=True, convergence_threshold=10.0)
    assert s.get_iterations_run() < 6
    s.set_target_normals(nrm)
    for pose in (None, poses["true_pose"]):
        got = s.evaluate(0.3, pose)
        assert got.evaluated == len(src)
        _check(got, s.get_eval_pairs(), er.evaluate(orc, src, tgt, got.pose, 0.3, normals=nrm), "early stop")


# ------------------------------------------------------------------------------------------------ leaves everything alone
def _snapshot(s, plane, tiles):
    d = dict(transformation=s.get_transformation(), distribution=s.get_distribution(), cov=s.get_cov_matrix(),
             particles=s.get_particles(), weights=s.get_particle_weight(), history=s.get_particle_history(),
             candidates=s.get_candidates(), cand_d2=s.get_candidate_dist2(), fallbacks=np.array(s.get_knn_fallbacks()),
             fallback_rows=np.sort(s.get_knn_fallback_rows()), ambiguous=np.array(s.get_ambiguous_pairs()), gpu_ms=s.get_gpu_ms(),
             iterations=np.array(s.get_iterations_run()))
    if tiles:
        d["survivors"] = s.get_knn_survivors()
    for k, v in s.get_trace().items():
        d["trace_" + k] = v
    if plane:
        stats, passes = s.get_plane_stats()
        d.update(plane_stats=stats, passes=np.array(passes), normals=s.get_target_normals())
    return d


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


@pytest.mark.parametrize("residual,knn", [("point", "tiles"), ("plane", "tiles"), ("point", "auto")])
def test_evaluate_changes_nothing(hip, orc, residual, knn):
    src, tgt, poses, _ = _case(hip, orc, "random")
    plane, tiles = residual == "plane", knn == "tiles"
    kw = dict(record_trace=True, residual=residual)
    s = _registered(hip, src, tgt, knn, **kw)
    before = _snapshot(s, plane, tiles)
    if tiles:
        assert before["survivors"].max() > 0
    e1 = s.evaluate(0.3, poses["true_pose"]); p1 = s.get_eval_pairs()
    _same(before, _snapshot(s, plane, tiles))
    e2 = s.evaluate(0.3, poses["true_pose"]); p2 = s.get_eval_pairs()
    _same(before, _snapshot(s, plane, tiles))
    assert e1.has_normals == plane
    a1, a2 = dataclasses.asdict(e1), dataclasses.asdict(e2)
    assert all(np.asarray(a1[k]).tobytes() == np.asarray(a2[k]).tobytes() for k in a1)
    assert p1[0].tobytes() == p2[0].tobytes() and p1[1].tobytes() == p2[1].tobytes()
    # the next registration: bit for bit that of a context that never evaluated
    init = hip.scans.make_particles(P_, seed=3) * 0.2
    fresh = _registered(hip, src, tgt, knn, **kw)
    for ctx in (s, fresh):
        ctx.add_cloud(src, tgt, init)
        assert ctx.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    a, b = _snapshot(s, plane, tiles), _snapshot(fresh, plane, tiles)
    a.pop("gpu_ms"); b.pop("gpu_ms")          # elapsed time of two different runs
    _same(a, b)


# ------------------------------------------------------------------------------------------------ after a mini-batch registration
@pytest.mark.parametrize("knn", ["auto", "tiles"])
def test_evaluate_after_a_minibatch_registration(hip, orc, knn):
    """Stage A of a mini-batch registration is sized for the 192 drawn rows: evaluate searches the 2048 rows in blocks."""
    src, tgt, poses, _ = _case(hip, orc, "random")
    mb = _registered(hip, src, tgt, knn, use_minibatch=True, batch_size=64, minibatch_seed=5)
    full = _registered(hip, src, tgt, knn)
    ea, eb = mb.evaluate(0.3, poses["true_pose"]), full.evaluate(0.3, poses["true_pose"])
    pa, pb = mb.get_eval_pairs(), full.get_eval_pairs()
    assert pa[0].tobytes() == pb[0].tobytes() and pa[1].tobytes() == pb[1].tobytes()
    a, b = dataclasses.asdict(ea), dataclasses.asdict(eb)
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    assert ea.evaluated == len(src) and mb.get_minibatch_rows()[1] == 192


# ------------------------------------------------------------------------------------------------ refusals
def _raw_evaluate(s, R, t, gate, struct_size=None):
    from svnicp_amd.binding import EvalStruct
    e = EvalStruct()
    e.struct_size = C.sizeof(EvalStruct) if struct_size is None else struct_size
    dp = C.POINTER(C.c_double)
    Rk = None if R is None else np.ascontiguousarray(R, np.float64).reshape(9)
    tk = None if t is None else np.ascontiguousarray(t, np.float64).reshape(3)
    rc = s._L.svnicp_evaluate(s._h, None if Rk is None else Rk.ctypes.data_as(dp), None if tk is None else tk.ctypes.data_as(dp),
                              float(gate), C.byref(e))
    return rc, s._L.svnicp_last_error(s._h).decode()


def test_evaluate_refusals(hip, orc):
    src, tgt, _, _ = _case(hip, orc, "ragged")
    init = hip.scans.make_particles(P_, seed=3) * 0.2
    s = hip.SVNICP(_param(hip), init, hip.ParticleWeightOpt())
    s.add_cloud(src, tgt, init)
    rc, msg = _raw_evaluate(s, None, None, 0.3)
    assert rc == -1 and "registration" in msg                        # before any registration
    assert s.eval_index_ptr == 0
    with pytest.raises(hip.SvnIcpError):
        s.get_eval_pairs()
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    assert _raw_evaluate(s, None, None, 0.3)[0] == 0
    I3, z = np.eye(3), np.zeros(3)
    for gate in (0.0, -1.0, float("nan")):
        rc, msg = _raw_evaluate(s, I3, z, gate)
        assert rc == -1 and "max_corr_dist" in msg, gate
    rc, msg = _raw_evaluate(s, I3, z, 0.3, struct_size=8)
    assert rc == -1 and "struct_size" in msg
    for R, t in ((I3, None), (None, z)):
        rc, msg = _raw_evaluate(s, R, t, 0.3)
        assert rc == -1 and "both" in msg
    bad = I3.copy(); bad[1, 2] = np.nan
    rc, msg = _raw_evaluate(s, bad, z, 0.3)
    assert rc == -1 and "non-finite" in msg
    assert _raw_evaluate(s, I3, z, float("inf"))[0] == 0              # an infinite gate is allowed
    s._check(s._L.svnicp_set_target(s._h, np.ascontiguousarray(tgt).ctypes.data_as(C.c_void_p), len(tgt), 0), "svnicp_set_target")
    rc, msg = _raw_evaluate(s, I3, z, 0.3)
    assert rc == -1 and "register again" in msg                       # the target changed: stage A's layout is gone
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS and _raw_evaluate(s, I3, z, 0.3)[0] == 0
    # the seeded scan is built for K neighbours
    src2, tgt2, _, _ = _case(hip, orc, "random")
    v2 = _registered(hip, src2, tgt2, "v2")
    rc, msg = _raw_evaluate(v2, I3, z, 0.3)
    assert rc == -1 and "K = 1" in msg and "knn=v2" in msg


# ------------------------------------------------------------------------------------------------ pipelines
@pytest.mark.parametrize("plane", [False, True])
def test_pipelines_report_the_evaluation(hip, tmp_path, plane):
    """Three scans of the synthetic drive of tests/test_pipeline_gpu.py, device map, eval_dist = 0.5: pipeline.py fills the
    ScanResult fields from the second scan on with what a direct evaluate at the result pose gives, and pipeline_drive (the C++
    pipeline on the same scans and particles) prints the same numbers."""
    from test_pipeline_gpu import _build_pipeline_drive
    pl, sc = hip.pipeline, hip.scans
    root = os.path.dirname(os.path.dirname(hip.library_path()))
    exe = _build_pipeline_drive(root)
    P, I, K, voxel, n_scans = 24, 12, 40, 0.5, 3
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
    cfg = pl.PipelineConfig(min_range=1.0, max_range=80.0, voxel_size=voxel, map_voxel_size=voxel, map_voxel_max_points=20,
                            map_range=100.0, particle_count=P, gpu_map=True, map_normals=plane, eval_dist=0.5,
                            solver=hip.SteinICPParam(iterations=I, lr=1.0, max_dist=1.0, KNN_count=K, SVN_full_grad=False,
                                                     residual="plane" if plane else "point"))
    pipe = pl.RegistrationPipeline(cfg, device=0)
    it = iter(parts)
    pipe._particles = lambda: next(it)
    py = []
    for k, (stamp, pts) in enumerate(scans):
        res = pipe.process_scan(pts, stamp)
        if k == 0:
            assert res.fitness is None and res.inlier_rmse is None and res.plane_rmse is None and res.plane_inliers is None
            continue
        ev = pipe._solver.evaluate(0.5, res.pose)            # the context still holds this scan's clouds
        assert res.fitness == ev.fitness and res.inlier_rmse == ev.inlier_rmse and 0.0 < res.fitness <= 1.0
        if plane:
            assert ev.has_normals and res.plane_rmse == ev.plane_rmse and res.plane_inliers == ev.plane_inliers > 0
        else:
            assert not ev.has_normals and res.plane_rmse is None and res.plane_inliers is None
        py.append((k, res.fitness, res.inlier_rmse, res.plane_rmse if plane else -1.0, res.plane_inliers if plane else -1))
    r = subprocess.run([exe, str(tmp_path / "scans.bin"), str(tmp_path / "out.bin"), str(P), str(I), str(K), str(voxel),
                        str(tmp_path / "particles.bin"), "1", "0", "0", "1" if plane else "0", "0.5"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("eval ")]
    assert [ln[1] for ln in lines] == ["0:", "1:", "2:"] and [float(v) for v in lines[0][2:]] == [-1, -1, -1, -1]
    for (k, fit, rmse, prmse, n_pl), ln in zip(py, lines[1:]):
        got = [float(v) for v in ln[2:]]
        print(f"scan {k}: python {fit!r} {rmse!r} {prmse!r} {n_pl}   c++ {got}")
        assert _rel(got[0], fit) and _rel(got[1], rmse) and _rel(got[2], prmse) and int(got[3]) == n_pl
