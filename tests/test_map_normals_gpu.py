"""Normals from the voxel map's own cells on the device (svnicp_map_query_normals, k_map_normals in csrc/map_normals.hip,
DESIGN.md section 4.4) against tests/map_normals_reference.py, the numpy restatement of the same definition.

Comparison rule: flags equal; with_normal equal to the restatement's count; 1 - |n.n_ref| <= 1e-9 where
(lambda1 - lambda0) / lambda2 >= 1e-3 (the eigenvector of lambda0 is then determined to eps / gap ~ 1e-13 rad); rows left
out by that floor, or whose flag sits on the threshold (|lambda1 - 0.01 lambda2| <= 1e-9 lambda2), are at most 1 % of the
rows (on the CPU the restatement alone leaves out at most 0.31 %, on the lattice at normal_k 8).  On every input here the
restatement has NO row on the threshold; the tests assert that, so flags and counts are compared on all rows.
The dense cases (voxels of up to 65, 130 and 256 points, normal_k 4, 16, 64) leave out no row; on an MI355X every flag and count
is equal and max 1 - |n.n_ref| = 2.2e-16 in all nine."""
import ctypes as C
import importlib
import os
import struct
import subprocess

import numpy as np
import pytest

import map_normals_cases as mc
import map_normals_reference as mr
import plane_reference as pr
from helpers import TIGHT

pytestmark = pytest.mark.gpu

ERR_INVALID = -1


def _device_map(hip, name):
    voxel, mp, max_range, steps = mc.case_inputs(name)
    dm = hip.pipeline.DeviceVoxelHashMap(voxel, max_range, mp, device=0, capacity_voxels=1 if name in mc.DENSE else 0)
    for cloud, T in steps:
        dm.add_pointcloud(cloud, T)
    return dm


def _compare(tag, n_dev, with_normal, ref, rows):
    """The comparison rule of the module docstring for the rows ``rows`` of the whole map."""
    assert n_dev.shape == (rows.size, 3), (tag, n_dev.shape, rows.size)
    valid = (n_dev != 0.0).any(axis=1)
    near, low_gap = (a[rows] for a in mc.left_out(ref))
    ref_valid, ref_n = ref.valid[rows], ref.normals[rows]
    out = int((near | low_gap).sum())
    cmp = valid & ref_valid & ~low_gap
    dev = 1.0 - np.abs((n_dev[cmp] * ref_n[cmp]).sum(axis=1)) if cmp.any() else np.zeros(1)
    print(f"{tag}: {rows.size} rows, with a normal {with_normal} (restatement {int(ref_valid.sum())}), left out {out}, "
          f"flags differ {int((valid != ref_valid).sum())}, max 1 - |n.n_ref| = {dev.max():.3e}")
    assert out <= 0.01 * rows.size
    assert not near.any()      # no flag of these inputs sits on the threshold itself (restatement, CPU): the equalities below are exact
    assert np.array_equal(valid, ref_valid)
    assert with_normal == int(valid.sum()) == int(ref_valid.sum())
    assert np.abs(np.linalg.norm(n_dev[valid], axis=1) - 1.0).max(initial=0.0) <= 1e-12
    assert np.array_equal(n_dev[~valid], np.zeros_like(n_dev[~valid]))
    assert dev.max() <= 1e-9


def _check_queries(tag, dm, vox, ref, kn, pose, radius, cut_may_be_empty=False):
    """Whole-map query, then a range query that cuts the map (neighbours then lie outside the selected rows)."""
    for what, args in (("whole", ()), ("cut", (pose, radius))):
        ptr, M = dm.get_map(*args)
        rows = mr.rows_of(vox, *args)
        assert M == rows.size and (what == "whole" or M < ref.points.shape[0])
        assert M > 0 or (what == "cut" and cut_may_be_empty)
        assert np.array_equal(dm.download(), ref.points[rows])
        nptr, with_normal = dm.get_map_normals(kn)
        assert (nptr != 0) == (M > 0)
        _compare(f"{tag} normal_k {kn} {what}", dm.download_normals(), with_normal, ref, rows)


# ---------------------------------------------------------------------------------------------
# 1. inputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kn", [(name, kn) for name in ("drive", "drive_shifted", "uniform64", "uniform3", "lattice") for kn in (8, 16)] +
                         [(name, kn) for name in mc.DENSE for kn in (4, 16, 64)])
def test_map_normals_agree_with_the_restatement(hip, name, kn):
    ref = mc.reference(name, kn)
    dm = _device_map(hip, name)
    pose, radius = mc.cut_query(name)
    if name == "lattice":      # the tie rule decides most neighbour sets here (59.9 % of the rows at normal_k 8, 78.5 % at 16)
        print(f"lattice normal_k {kn}: rows with distinct points tied at the boundary {ref.boundary_tie.mean():.3f}")
        assert ref.boundary_tie.mean() > 0.5
    if name == "uniform64":    # more candidates than one tile of the kernel (1024), and the 64 copies of point 0
        assert ref.n_cand.max() > 1024 and int((~ref.valid).sum()) >= 64
    if name in mc.DENSE:       # rows in a voxel's second (and at 256: third, fourth) block of 64; at normal_k 64 every lane holds a
        in_voxel = np.arange(ref.points.shape[0]) - np.repeat(ref.offs[:-1], np.diff(ref.offs))      # neighbour and some blocks are too small
        print(f"{name} normal_k {kn}: {len(ref.keys)} voxels, {int((np.diff(ref.offs) > 64).sum())} above 64 points, rows past the first "
              f"block {int((in_voxel >= 64).sum())}, candidates {ref.n_cand.min()}..{ref.n_cand.max()}, no normal {int((~ref.valid).sum())}")
        assert ref.valid[in_voxel >= 64].sum() >= 10 and ref.n_cand.max() > 1024 and int((~ref.valid).sum()) >= 65
        if name == "dense256":     # blocks below normal_k 64 and blocks of four tiles; rows in a third block
            assert ref.n_cand.min() < 64 and ref.n_cand.max() > 3072 and ref.valid[in_voxel >= 128].sum() >= 100
    _check_queries(name, dm, mc.host_map(name)._vox, ref, kn, pose, radius)
    if name in mc.DENSE and kn == 16:      # normal_k 0 means 16
        _, w16 = dm.get_map_normals(16)
        n16 = dm.download_normals()
        _, w0 = dm.get_map_normals(0)
        assert w0 == w16 and n16.shape[0] > 0 and np.array_equal(dm.download_normals(), n16)


# ---------------------------------------------------------------------------------------------
# 2. moving sensor: tombstones and a rebuild
# ---------------------------------------------------------------------------------------------
def test_map_normals_follow_a_moving_sensor(hip):
    """The sequence of test_device_map_equals_host_map's first case: 5 clouds of 30 000 points, the sensor moves, far voxels
    are culled (tombstones in the probe chains) and the table is rebuilt: it starts at 65 536 slots, so from the second cloud on
    (live + 30 000) * 2 exceeds the capacity and live voxels are moved into a larger table, with tombstones arriving afterwards.
    Normals are checked after every step."""
    from test_voxel_map_gpu import _pose
    pl = hip.pipeline
    voxel, max_pts, n, extent, steps, kn = 1.0, 20, 30000, 40.0, 5, 8
    rng = np.random.default_rng(int(voxel * 100) + max_pts)
    max_range = 0.6 * extent
    hm = pl.VoxelHashMap(voxel, max_range, max_pts)
    dm = pl.DeviceVoxelHashMap(voxel, max_range, max_pts, device=0, capacity_voxels=1)
    moved = []      # live voxels at each rebuild
    for k in range(steps):
        cloud = (rng.uniform(-1, 1, size=(n, 3)) * extent * 0.5).astype(np.float32)
        cloud[: n // 10] = cloud[0]
        T = _pose(rng, extent * 0.15 * k)
        live, rebuilds = len(hm), dm.table_info()[2]
        hm.add_pointcloud(cloud, T); dm.add_pointcloud(cloud, T)
        if dm.table_info()[2] > rebuilds:
            moved.append(live)
        assert len(dm) == len(hm), k
        Q = _pose(rng, extent * 0.1)
        _check_queries(f"step {k}", dm, hm._vox, mr.map_normals(hm._vox, kn), kn, Q, 0.3 * extent,
                       cut_may_be_empty=True)      # the last step's query centre has left the map
    print(f"table_info {dm.table_info()}, live voxels at the rebuilds {moved}")
    assert dm.table_info()[2] >= 1
    assert max(moved) > 1000      # a rebuild of a table that held voxels


# ---------------------------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------------------------
def test_map_normals_refusals(hip):
    L = hip.load_library()
    dm = _device_map(hip, "uniform3")
    n = C.c_int64(-5)

    def rc(kn):
        return L.svnicp_map_query_normals(dm._h, kn, C.byref(n))

    assert rc(16) == ERR_INVALID and "query" in L.svnicp_map_last_error(dm._h).decode()      # before any query
    assert dm.download_normals().shape == (0, 3)
    _, M = dm.get_map()
    assert rc(3) == ERR_INVALID and rc(65) == ERR_INVALID and rc(-1) == ERR_INVALID
    assert "normal_k" in L.svnicp_map_last_error(dm._h).decode()
    assert rc(16) == 0 and n.value > 0
    n16 = dm.download_normals()
    assert rc(0) == 0                                                                        # 0 = 16
    assert np.array_equal(dm.download_normals(), n16) and n16.shape == (M, 3)
    dm.add_pointcloud(np.zeros((1, 3), np.float32), np.eye(4))                               # the map changed since the query
    assert rc(16) == ERR_INVALID and n.value == 0
    assert L.svnicp_map_normals_devptr(dm._h) is None
    dm.get_map()
    assert rc(16) == 0
    assert L.svnicp_map_clear(dm._h) == 0
    assert rc(16) == ERR_INVALID
    dm.add_pointcloud(mc.case_inputs("uniform3")[3][0][0], np.eye(4))
    _, M = dm.get_map(np.eye(4), 1e-6)                                                       # an empty selection
    assert M == 0
    n.value = -5
    assert rc(16) == 0 and n.value == 0
    assert dm.download_normals().shape == (0, 3)
    assert L.svnicp_map_query_normals(dm._h, 16, None) == 0                                  # with_normal_out may be NULL


# ---------------------------------------------------------------------------------------------
# 4. determinism
# ---------------------------------------------------------------------------------------------
def test_map_normals_are_bit_identical_on_every_call(hip):
    dm = _device_map(hip, "uniform64")
    dm.get_map()
    _, w1 = dm.get_map_normals(16)
    a = dm.download_normals()
    _, w2 = dm.get_map_normals(16)
    b = dm.download_normals()
    other = _device_map(hip, "uniform64")          # another table, filled the same way
    other.get_map()
    _, w3 = other.get_map_normals(16)
    assert w1 == w2 == w3
    assert np.array_equal(a, b) and np.array_equal(a, other.download_normals())


# ---------------------------------------------------------------------------------------------
# 5. solver hand-over
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [4, 64])
def test_solver_takes_the_map_normals_by_device_pointer(hip, orc, P):
    """512 source points of the drive's scan 1 against a map of about 4 000 points (scan 0 sampled at 0.6 m, voxel 2.0, 20
    points per voxel — the whole scene: ground, walls and boxes constrain all six directions; a single sheet or the ground
    patch around the sensor leaves H singular but for its 1e-6 damping, the particles fly off and no 1e-9 parity can be asked
    of them): the context is given the map's rows and normals by device pointer, runs no normal pass, and its registration
    agrees with plane_reference.run on the same normals to the tolerances of test_solver_parity_with_supplied_normals.
    The helper's own run shows the configuration is well conditioned and exercises the gate and both Huber branches.
    svnicp_set_target_normals normalises what it is given: a unit row comes back within 2 ulp (4.5e-16), a zero row as zero."""
    from test_plane_gpu import PAR, _T
    R0, T0 = np.eye(3), np.zeros(3)                          # scan 0's true pose; the planted motion is 0.05 m and 0.3 degrees
    to_map, _, _ = mc._drive_scan(0)
    _, source, _ = mc._drive_scan(1)
    tgt = hip.pipeline.downsample_uniform(to_map, 0.6)
    src = np.ascontiguousarray(source[np.linspace(0, source.shape[0] - 1, 512).astype(int)], np.float64)
    dm = hip.pipeline.DeviceVoxelHashMap(2.0, 1e9, 20, device=0)
    dm.add_pointcloud(tgt.astype(np.float32), np.eye(4))
    ptr, M = dm.get_map()
    rows = dm.download()
    nptr, with_normal = dm.get_map_normals(16)
    nrm = dm.download_normals()
    assert 3500 <= M <= 4500 and with_normal > 0.9 * M
    init = hip.scans.make_particles(P, seed=3) * 0.2
    prm = hip.SteinICPParam(iterations=PAR["iterations"], lr=1.0, max_dist=PAR["max_dist"], KNN_count=PAR["K"], SVN_full_grad=False,
                            record_trace=True, residual="plane", huber_delta=PAR["delta"], normal_k=16)
    s = hip.SVNICP(prm, init, hip.ParticleWeightOpt())
    s.add_cloud_device_target(src, ptr, M, init)
    s.set_target_normals_device(nptr, M)
    s.set_initial_mean(_T(R0, T0))
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    assert s.get_plane_stats(with_sums=False)[1] == 0, "normals from the map: no normal pass"
    held = s.get_target_normals()
    assert np.abs(held - nrm).max() <= 4.5e-16
    assert np.array_equal((held != 0).any(axis=1), (nrm != 0).any(axis=1))
    ref = pr.run(orc, src, rows, held, init, PAR["K"], PAR["iterations"], PAR["max_dist"], PAR["delta"], lr=1.0, svn_full_grad=False,
                 R0=R0, t0=T0)
    accepted = np.array([[len(x) for x in it] for it in ref.residuals])
    res = np.abs(np.concatenate([np.concatenate(x) for x in ref.residuals]))
    cond = max(np.linalg.cond(h.reshape(6, 6)) for h in ref.H.reshape(-1, 36))
    print(f"P {P}: helper accepts {accepted.min()}..{accepted.max()} of 512 pairs, {(res > PAR['delta']).mean():.2f} outside delta, cond H <= {cond:.1e}")
    assert 128 <= accepted.min() and accepted.max() < 512 and 0.05 <= (res > PAR["delta"]).mean() <= 0.95 and cond < 1e5
    run = s.get_iterations_run()
    assert run == ref.iterations_run == PAR["iterations"]
    tr = s.get_trace()
    assert np.array_equal(tr["corr"][:run], ref.corr[:run])
    for k, r in (("H", ref.H), ("b", ref.b), ("newton", ref.newton), ("phi", ref.phi)):
        print(f"P {P} {k}: max |device - helper| = {np.abs(tr[k][:run] - r[:run]).max():.3e}")
        assert np.allclose(tr[k][:run], r[:run], rtol=TIGHT, atol=TIGHT), k
    assert np.allclose(tr["h"][:run], ref.h[:run], rtol=TIGHT, atol=TIGHT, equal_nan=True)
    assert np.abs(s.get_particles() - ref.particles).max() <= TIGHT
    assert np.abs(s.get_transformation() - ref.solver.get_transformation()).max() <= TIGHT
    assert np.abs(s.get_distribution() - ref.solver.get_distribution()).max() <= TIGHT
    assert np.abs(s.get_cov_matrix() - ref.solver.get_cov_matrix()).max() <= TIGHT
    stats, _ = s.get_plane_stats()
    assert np.array_equal(stats[:, 0], ref.stats[:, 0])
    assert stats[:, 0].min() >= 128   # the map's normals reached the accumulation for every particle
    assert np.allclose(stats[:, 1], ref.stats[:, 1], rtol=TIGHT, atol=TIGHT)


# ---------------------------------------------------------------------------------------------
# 6. the Python drive
# ---------------------------------------------------------------------------------------------
def test_python_drive_with_map_normals(hip):
    """tests/test_pipeline_gpu.py's drive (8 scans, climb + yaw) in point mode and in plane mode with the map's normals: no
    normal pass over the whole drive, every pose finite, maximum z error and final yaw error no larger than point mode's, and
    the maximum z error below the 0.05 m the existing test demands.  The solver's own pass (residual="plane" without
    map_normals) counts one per registered scan (run over the first three scans).
    Measured on an MI355X: maximum z error 34.7 mm in point mode, 5.1 mm with the map's normals; final rotation error 6.2e-3
    against 7.6e-4 rad (both series: DESIGN.md section 4.4)."""
    pl, sc = hip.pipeline, hip.scans
    scene = sc.make_scene()
    truth, scans = [], []
    for k in range(8):
        T = mc.drive_pose(sc, k)
        truth.append(T)
        scans.append(sc.lidar_scan(scene, T[:3, :3], T[:3, 3], 32768, stream=300 + k))

    def drive(n_scans, residual, map_normals):
        cfg = pl.PipelineConfig(min_range=1.0, max_range=80.0, voxel_size=0.5, map_voxel_size=0.5, map_voxel_max_points=20,
                                map_range=100.0, particle_count=32, gpu_map=True, map_normals=map_normals,
                                solver=hip.SteinICPParam(iterations=30, lr=1.0, max_dist=1.0, KNN_count=50, residual=residual))
        pipe = pl.RegistrationPipeline(cfg, device=0)
        res = [pipe.process_scan(scans[k], stamp=0.1 * k) for k in range(n_scans)]
        assert all(r.state == int(hip.SteinICPState.ALIGN_SUCCESS) for r in res[1:])
        return pipe, res

    def errors(res):
        ez = np.array([abs(T[2, 3] - r.pose[2, 3]) for T, r in zip(truth, res)])
        eyaw = np.array([np.linalg.norm(pl.so3_log(T[:3, :3].T @ r.pose[:3, :3])) for T, r in zip(truth, res)])
        return ez, eyaw

    _, point = drive(8, "point", False)
    pipe, plane = drive(8, "plane", True)
    assert pipe._solver.get_plane_stats(with_sums=False)[1] == 0
    assert all(np.isfinite(r.pose).all() for r in plane)
    assert plane[0].with_normal is None and all(r.with_normal > 0 for r in plane[1:])
    assert all(r.with_normal is None for r in point)
    ez_pt, eyaw_pt = errors(point)
    ez_pl, eyaw_pl = errors(plane)
    print("point mode  z error per frame:", np.round(ez_pt, 4), "rot err", np.round(eyaw_pt, 5))
    print("map normals z error per frame:", np.round(ez_pl, 4), "rot err", np.round(eyaw_pl, 5))
    print("rows with a normal per registered scan:", [r.with_normal for r in plane[1:]])
    assert ez_pl.max() <= ez_pt.max() and eyaw_pl[-1] <= eyaw_pt[-1]
    assert ez_pl.max() < 0.05
    own, _ = drive(3, "plane", False)
    assert own._solver.get_plane_stats(with_sums=False)[1] == 2


# ---------------------------------------------------------------------------------------------
# 7. the C++ drive
# ---------------------------------------------------------------------------------------------
def test_cpp_drive_with_map_normals_agrees_with_python(hip, tmp_path):
    """pipeline_drive with its map_normals switch (device map, plane residual, normals from the map) against pipeline.py on the
    same scans and particles: poses to 1e-9, the same with_normal per registered scan."""
    from test_pipeline_gpu import _build_pipeline_drive
    pl, sc = hip.pipeline, hip.scans
    root = os.path.dirname(os.path.dirname(hip.library_path()))
    exe = _build_pipeline_drive(root)
    P, I, K, voxel, n_scans = 24, 12, 40, 0.5, 4
    scene = sc.make_scene()
    rng = np.random.default_rng(11)
    scans, parts = [], []
    for k in range(n_scans):
        T = mc.drive_pose(sc, k)
        scans.append((0.1 * k, sc.lidar_scan(scene, T[:3, :3], T[:3, 3], 16384, stream=700 + k).astype(np.float32)))
        parts.append(hip.initialize_particles(P, pl.PRIOR_UB, pl.PRIOR_LB, rng))
    with open(tmp_path / "scans.bin", "wb") as f:
        f.write(struct.pack("<i", n_scans))
        for stamp, pts in scans:
            f.write(struct.pack("<di", stamp, pts.shape[0])); f.write(np.ascontiguousarray(pts[:, :3], np.float32).tobytes())
    with open(tmp_path / "particles.bin", "wb") as f:
        for p in parts:
            f.write(np.ascontiguousarray(p, np.float64).tobytes())
    r = subprocess.run([exe, str(tmp_path / "scans.bin"), str(tmp_path / "out.bin"), str(P), str(I), str(K), str(voxel),
                        str(tmp_path / "particles.bin"), "1", "0", "0", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    off = 0

    def take(dtype, n):
        nonlocal off
        a = np.frombuffer(raw, dtype, n, off); off += a.nbytes
        return a
    recs = []
    for k in range(n_scans):
        aligned = int(take("<i4", 1)[0])
        pose, guess = take("<f8", 12), take("<f8", 12)
        take("<f8", 6 + 6 + 36)
        B, M = (int(v) for v in take("<i8", 2))
        take("<f8", 3 * B + 3 * M + 6 * P)
        recs.append(dict(aligned=aligned, pose=pose, M=M, with_normal=int(take("<i8", 1)[0]) if aligned else None))
    assert off == len(raw) and recs[0]["aligned"] == 0 and all(rc["aligned"] == 1 for rc in recs[1:])
    cfg = pl.PipelineConfig(min_range=1.0, max_range=80.0, voxel_size=voxel, map_voxel_size=voxel, map_voxel_max_points=20,
                            map_range=100.0, particle_count=P, gpu_map=True, map_normals=True,
                            solver=hip.SteinICPParam(iterations=I, lr=1.0, max_dist=1.0, KNN_count=K, SVN_full_grad=False,
                                                     residual="plane"))
    pipe = pl.RegistrationPipeline(cfg, device=0)
    it = iter(parts)
    pipe._particles = lambda: next(it)
    for k, (stamp, pts) in enumerate(scans):
        res = pipe.process_scan(pts, stamp)
        T = np.eye(4); T[:3, :3] = recs[k]["pose"][:9].reshape(3, 3); T[:3, 3] = recs[k]["pose"][9:]
        assert np.allclose(res.pose, T, rtol=0, atol=1e-9), k
        assert res.with_normal == recs[k]["with_normal"], k
        if k:
            assert 0 < res.with_normal <= recs[k]["M"]
    assert pipe._solver.get_plane_stats(with_sums=False)[1] == 0
