"""svnicp_eval_information on the device (csrc/information.hip) against tests/information_reference.py, the
numpy restatement of include/svnicp_hip.h "information matrix of a registration".  P = 4, K = 16, 3 iterations.

Tolerances: pairs is exact (the evaluate tests' preconditions exclude rows on the gate and nearest-neighbour ties, and the Huber
weight is continuous at delta).  Every term of H and b is the same float64 expression on both sides up to the order of a
handful of products; the sums differ by the order of at most 2048 additions: every entry within TIGHT = 1e-9 of A, the sum of
the entry's absolute terms.  Everything svnicp_information_solve derives is compared bit for bit with the same routine run on
the host on the returned H, b, pairs and sum_wr2."""
import ctypes as C
import dataclasses
import os
import struct
import subprocess

import numpy as np
import pytest

from helpers import TIGHT

import evaluate_reference as er
import information_reference as ir
import nonfinite_reference as nf
from test_evaluate_gpu import P_, _case, _registered, _rel, _same, _snapshot
from test_information_cpu import check_single_plane, single_plane

import evaluate_cases as ec

pytestmark = pytest.mark.gpu

INF = float("inf")
_DERIVED = ("rank", "sigma2", "eigval", "eigvec", "eig_t", "vec_t", "eig_r", "vec_r", "step", "cov")


def _bits(info):
    return {k: np.asarray(v).tobytes() for k, v in dataclasses.asdict(info).items()}


def _check(hip, got, want, label, gate, delta):
    """``got``: RegistrationInformation of the device; ``want``: information_reference.Sums of the same evaluate."""
    errH = np.abs(got.H - want.H) / np.where(want.A_H > 0, want.A_H, 1.0)
    errb = np.abs(got.b - want.b) / np.where(want.A_b > 0, want.A_b, 1.0)
    print(f"{label}: pairs {got.pairs} rank {got.rank} sum_w {got.sum_w!r} / {want.sum_w!r} sum_wr2 {got.sum_wr2!r} / {want.sum_wr2!r} "
          f"max |dH| / A {errH.max():.3e} max |db| / A {errb.max():.3e} eigval {got.eigval.tolist()}")
    assert got.form == want.form and got.pairs == want.pairs, label
    assert got.max_corr_dist == gate and got.huber_delta == delta and got.eig_floor_ratio == 0.0, label
    assert np.all(np.abs(got.H - want.H) <= TIGHT * want.A_H) and np.all(np.abs(got.b - want.b) <= TIGHT * want.A_b), label
    assert np.array_equal(got.H, got.H.T), label
    assert _rel(got.sum_w, want.sum_w) and _rel(got.sum_wr2, want.sum_wr2), label
    host = hip.information_solve(got.form, got.pairs, got.sum_wr2, got.H, got.b)
    for f in _DERIVED:
        assert np.asarray(getattr(got, f)).tobytes() == np.asarray(getattr(host, f)).tobytes(), (label, f)
    assert np.isfinite(np.concatenate([np.ravel(np.asarray(v, float)) for k, v in dataclasses.asdict(got).items()
                                       if k not in ("form", "huber_delta", "max_corr_dist")])).all(), label   # the two may be +inf as passed


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("knn", ["auto", "tiles"])
@pytest.mark.parametrize("cloud", ec.CLOUDS)
def test_information_agrees_with_the_restatement(hip, orc, cloud, knn):
    """Both forms, two poses (NULL = the registration's own result), Huber delta 0.1 and +inf, gate 0.3, supplied normals."""
    src, tgt, poses, nrm = _case(hip, orc, cloud)
    s = _registered(hip, src, tgt, knn)
    s.set_target_normals(nrm)
    for pose_name in ("null", "true_pose"):
        ev = s.evaluate(0.3, None if pose_name == "null" else poses[pose_name])
        T = ev.pose
        if pose_name == "null":      # this pose is not among the ones checked on the CPU: check it here
            near_gate, tie = er.preconditions(er.evaluate(orc, src, tgt, T, 0.3, with_second=True), 0.3)
            assert near_gate.size == 0 and tie.size == 0
        ref = er.evaluate(orc, src, tgt, T, 0.3, normals=nrm)
        for form in ("point", "plane"):
            for delta in (0.1, INF):
                got = s.information(form, delta)
                assert np.array_equal(got.pose, T)
                want = ir.sums(orc, src, tgt, T, 0.3, form, delta, normals=nrm, ev=ref)
                _check(hip, got, want, f"{cloud} {knn} {pose_name} {form} delta {delta}", 0.3, delta)
                assert got.pairs == (ev.inliers if form == "point" else ev.plane_inliers) > 0


def _unit_rows(M, seed):
    n = np.random.default_rng(seed).normal(size=(M, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    if M > 2:
        n[1] = 0.0                   # a target row without a normal
    return n


@pytest.mark.parametrize("B,M", [(1, 1), (70, 64), (257, 300)])
def test_information_edges(hip, orc, B, M):
    """One row; a partial wave; a second workgroup that holds a single row."""
    src, tgt = hip.scans.random_clouds(B, M, seed=7)
    nrm = _unit_rows(M, 11)
    s = _registered(hip, src, tgt)
    ev = s.evaluate(1.0, np.eye(4))
    _check(hip, s.information("point", 0.1), ir.sums(orc, src, tgt, ev.pose, 1.0, "point", 0.1), f"B {B} M {M} point", 1.0, 0.1)
    s.set_target_normals(nrm)
    ev = s.evaluate(1.0, np.eye(4))
    nrm_held = s.get_target_normals()
    for form in ("point", "plane"):
        got = s.information(form, 0.1)
        _check(hip, got, ir.sums(orc, src, tgt, ev.pose, 1.0, form, 0.1, normals=nrm_held), f"B {B} M {M} {form} normals", 1.0, 0.1)
    assert got.pairs == ev.plane_inliers


# ------------------------------------------------------------------------------------------------ non-finite
@pytest.mark.parametrize("nan_target_0", [False, True])
def test_information_with_nonfinite_and_huge_rows(hip, orc, nan_target_0):
    """The poisoned clouds of the evaluate tests: rows that are not evaluated (and the 1e160 rows, whose d2 is +inf) contribute
    nothing, every output is finite."""
    src, tgt, poses, nrm = _case(hip, orc, "random")
    src_rows, tgt_rows = [3, 64, 65, 700, 1023, 2047], [5, 511, 512, 4000, 8191]
    kinds = ("nan1", "+inf", "big64")
    src_b, tgt_b = nf.poison(src, src_rows, kinds), nf.poison(tgt, tgt_rows, kinds)
    if nan_target_0:
        tgt_b = nf.poison(tgt_b, [0], "nan1")
    s = _registered(hip, src_b, tgt_b)
    s.set_target_normals(nrm)
    T = poses["true_pose"]
    for gate in (0.3, INF):
        ev = s.evaluate(gate, T)
        ref = er.evaluate(orc, src_b, tgt_b, T, gate, normals=nrm, finite=False)
        for form in ("point", "plane"):
            got = s.information(form, 0.1)
            want = ir.sums(orc, src_b, tgt_b, T, gate, form, 0.1, normals=nrm, finite=False, ev=ref)
            _check(hip, got, want, f"non-finite target0 {nan_target_0} gate {gate} {form}", gate, 0.1)
            assert got.pairs <= ev.evaluated - 2 and not want.rows[src_rows].any()


# ------------------------------------------------------------------------------------------------ known answer
def test_single_plane_on_the_device(hip, orc):
    src, tgt, nrm = single_plane()
    s = _registered(hip, src, tgt)
    s.set_target_normals(nrm)
    ev = s.evaluate(0.5, np.eye(4))
    assert ev.plane_inliers == 300
    got = s.information("plane")
    _check(hip, got, ir.sums(orc, src, tgt, np.eye(4), 0.5, "plane", INF, normals=nrm), "single plane", 0.5, INF)
    check_single_plane(got.pairs, got.b, got.rank, got.eigval, got.eigvec, got.eig_t, got.step, got.cov)


# ------------------------------------------------------------------------------------------------ leaves everything alone
@pytest.mark.parametrize("residual", ["point", "plane"])
def test_information_is_repeatable_and_changes_nothing(hip, orc, residual):
    src, tgt, poses, _ = _case(hip, orc, "random")
    plane = residual == "plane"
    kw = dict(record_trace=True, residual=residual)
    s = _registered(hip, src, tgt, "tiles", **kw)
    s.evaluate(0.3, poses["true_pose"])
    before, pairs_before = _snapshot(s, plane, True), s.get_eval_pairs()
    forms = ("point", "plane") if plane else ("point",)
    first = {f: s.information(f, 0.1) for f in forms}
    _same(before, _snapshot(s, plane, True))
    second = {f: s.information(f, 0.1) for f in forms}
    _same(before, _snapshot(s, plane, True))
    for f in forms:
        assert _bits(first[f]) == _bits(second[f]), f
        assert first[f].pairs > 0
    pairs_after = s.get_eval_pairs()
    assert pairs_before[0].tobytes() == pairs_after[0].tobytes() and pairs_before[1].tobytes() == pairs_after[1].tobytes()
    # the next registration: bit for bit that of a context that never asked
    init = hip.scans.make_particles(P_, seed=3) * 0.2
    fresh = _registered(hip, src, tgt, "tiles", **kw)
    for ctx in (s, fresh):
        ctx.add_cloud(src, tgt, init)
        assert ctx.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    a, b = _snapshot(s, plane, True), _snapshot(fresh, plane, True)
    a.pop("gpu_ms"); b.pop("gpu_ms")          # elapsed time of two different runs
    _same(a, b)


# ------------------------------------------------------------------------------------------------ refusals
def _raw(s, form=0, delta=0.1, floor=0.0, struct_size=None):
    from svnicp_amd.binding import InformationStruct
    o = InformationStruct()
    o.struct_size = C.sizeof(InformationStruct) if struct_size is None else struct_size
    rc = s._L.svnicp_eval_information(s._h, int(form), float(delta), float(floor), C.byref(o))
    return rc, s._L.svnicp_last_error(s._h).decode()


def test_information_refusals(hip, orc):
    src, tgt, _, nrm = _case(hip, orc, "ragged")
    vp = C.c_void_p
    s = _registered(hip, src, tgt)
    I4 = np.eye(4)
    # no evaluate at all
    rc, msg = _raw(s)
    assert rc == -1 and "no svnicp_evaluate yet" in msg
    s.evaluate(0.3, I4)
    assert _raw(s)[0] == 0
    # the arguments
    rc, msg = _raw(s, form=7)
    assert rc == -1 and "unknown form" in msg
    for delta in (0.0, -1.0, float("nan")):
        rc, msg = _raw(s, delta=delta)
        assert rc == -1 and "huber_delta" in msg, delta
    for floor in (1.0, -0.1, float("nan")):
        rc, msg = _raw(s, floor=floor)
        assert rc == -1 and "eig_floor_ratio" in msg, floor
    rc, msg = _raw(s, struct_size=8)
    assert rc == -1 and "struct_size" in msg
    rc, msg = _raw(s, form=1)
    assert rc == -1 and "has_normals = 0" in msg       # the plane form after an evaluate without normals
    assert _raw(s, delta=INF)[0] == 0 and _raw(s, floor=0.5)[0] == 0
    # the normals changed: the rows' classes belong to the evaluate before
    s.set_target_normals(nrm)
    rc, msg = _raw(s, form=1)
    assert rc == -1 and "the target normals changed" in msg
    s.evaluate(0.3, I4)
    assert _raw(s, form=1)[0] == 0 and _raw(s, form=0)[0] == 0
    # a registration began
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    rc, msg = _raw(s)
    assert rc == -1 and "a registration began" in msg
    s.evaluate(0.3, I4)
    assert _raw(s)[0] == 0
    # the source, then the target, changed (evaluate itself wants a registration first)
    for setter, cloud, why in (("svnicp_set_source", src, "the source changed"), ("svnicp_set_target", tgt, "the target changed")):
        s._check(getattr(s._L, setter)(s._h, np.ascontiguousarray(cloud).ctypes.data_as(vp), len(cloud), 0), setter)
        rc, msg = _raw(s)
        assert rc == -1 and why in msg, setter
        assert s.get_eval_pairs()[0].shape == (len(src),)            # the getter keeps answering
        assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
        rc, msg = _raw(s)
        assert rc == -1 and "a registration began" in msg
        s.evaluate(0.3, I4)
        assert _raw(s)[0] == 0


# ------------------------------------------------------------------------------------------------ pipelines
def test_pipelines_report_the_information(hip, tmp_path):
    """The three-scan drive of tests/test_evaluate_gpu.py with information = "plane": pipeline.py fills ScanResult.information
    with what a direct call gives, and pipeline_drive (the C++ pipeline on the same scans and particles) prints the same
    pairs, rank and eigenvalues.  With information = "off" the field stays None."""
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

    def config(information):
        return pl.PipelineConfig(min_range=1.0, max_range=80.0, voxel_size=voxel, map_voxel_size=voxel, map_voxel_max_points=20,
                                 map_range=100.0, particle_count=P, gpu_map=True, map_normals=True, eval_dist=0.5, information=information,
                                 solver=hip.SteinICPParam(iterations=I, lr=1.0, max_dist=1.0, KNN_count=K, SVN_full_grad=False, residual="plane"))
    py = []
    for information in ("plane", "off"):
        pipe = pl.RegistrationPipeline(config(information), device=0)
        it = iter(parts)
        pipe._particles = lambda: next(it)
        for k, (stamp, pts) in enumerate(scans[:n_scans if information == "plane" else 2]):
            res = pipe.process_scan(pts, stamp)
            if k == 0 or information == "off":
                assert res.information is None
                continue
            pipe._solver.evaluate(0.5, res.pose)             # the context still holds this scan's clouds
            direct = pipe._solver.information("plane", INF)
            assert _bits(res.information) == _bits(direct) and res.information.pairs == res.plane_inliers > 0
            py.append((k, res.information))
    r = subprocess.run([exe, str(tmp_path / "scans.bin"), str(tmp_path / "out.bin"), str(P), str(I), str(K), str(voxel),
                        str(tmp_path / "particles.bin"), "1", "0", "0", "1", "0.5", "plane"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("info ")]
    assert [ln[1] for ln in lines] == ["1:", "2:"]
    for (k, info), ln in zip(py, lines):
        lam = [float(v) for v in ln[4:]]
        print(f"scan {k}: python {info.pairs} {info.rank} {info.eigval.tolist()}   c++ {ln[2:]}")
        assert int(ln[2]) == info.pairs and int(ln[3]) == info.rank and len(lam) == 6
        assert all(_rel(a, b) for a, b in zip(lam, info.eigval))
