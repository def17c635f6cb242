"""Visibility-based clearing of the device voxel map (svnicp_map_clear_seen_through, csrc/map_visibility.hip)
against pipeline.VoxelHashMap.clear_seen_through, the numpy restatement of the same contract: after every call the device map
(svnicp_map_download after a whole-map query) equals the restatement's point for point and in order, and every field of
svnicp_visibility_stats is equal.  The crafted cases carry expectations written out by hand (tests/map_visibility_cases.py)."""
import ctypes as C
import functools
import importlib
import os
import struct
import subprocess

import numpy as np
import pytest

import map_normals_cases as mc
import map_normals_reference as mr
import map_visibility_cases as mv
from test_voxel_map_gpu import _host_rows
from test_voxel_map_lifecycle_gpu import sequence

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
CASES = mv.crafted_cases()


def _same(tag, dm, hm):
    assert len(dm) == len(hm), tag
    _, M = dm.get_map()
    want = _host_rows(hm)
    assert M == want.shape[0], (tag, M, want.shape[0])
    assert np.array_equal(dm.download(), want), tag


def _dev(scan):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(scan, np.float32)).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    return t


# ---------------------------------------------------------------------------------------------
# 1. the crafted cases through the C ABI, scan on the host and in device memory
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_crafted_case(hip, case):
    pl = hip.pipeline
    sensor = mv.tiny_sensor(pl)
    stored = mv.to_map_frame(case.points, case.pose)
    kw = dict(window=case.window, margin=case.margin, max_range=case.max_range)
    hm = pl.VoxelHashMap(1.0, 100.0, 20)
    hm.add_pointcloud(stored, np.eye(4))
    want = hm.clear_seen_through(case.scan, case.pose, sensor, **kw)
    keep = ~np.array(case.removed)
    assert want == {"pixels_filled": case.filled, "points_tested": case.tested, "points_removed": sum(case.removed),
                    "voxels_emptied": mv.voxels_emptied(stored, keep)}          # the hand-written expectation
    for mem in ("host", "device"):
        dm = pl.DeviceVoxelHashMap(1.0, 100.0, 20, device=0, capacity_voxels=1)
        dm.add_pointcloud(stored, np.eye(4))
        if mem == "host":
            got = dm.clear_seen_through(case.scan, case.pose, sensor, **kw)
        else:
            t = _dev(case.scan)
            got = dm.clear_seen_through_device(t.data_ptr(), t.shape[0], case.pose, sensor, **kw)
        assert got == want, (mem, got, want)
        _same(f"{case.name} {mem}", dm, hm)
        assert dm.table_info()[1] == want["voxels_emptied"]
        dm.close()


# ---------------------------------------------------------------------------------------------
# 2. compaction across the 64-point blocks of a voxel
# ---------------------------------------------------------------------------------------------
def _block_sensor(pl):
    """32 rows x 360 columns at 1 degree: at 9.5 m a 4 m voxel spans some 20 x 12 pixels, one stored point per pixel."""
    return pl.SegParams(n_scan=32, horizon_scan=360, ground_scan_ind=7, ang_res_x=1.0, ang_res_y=1.0, ang_bottom=16.0, min_range=1.0)


def _block_pixels(pl):
    """Three voxels of 4 m around the +x, +y and -x axes: (2, 0, 0), (0, 2, 0) and (-2, 0, 0); per voxel the pixels (row, col) of
    rows 17..28 (elevation 1.5..12.5 degrees) and 19 columns, every one inside the voxel at 9.5 m range."""
    H = 360
    col_of = lambda h: (-round((h - 90.0) / 1.0) + H // 2) % H
    sectors = ([89 - k for k in range(19)], [1 + k for k in range(19)], [-89 + k for k in range(19)])     # h = atan2(x, y), degrees
    out = []
    for hs in sectors:
        out.append([(row, col_of(h)) for h in hs for row in range(17, 29)])
    return out


def _block_setup(pl):
    sensor = _block_sensor(pl)
    pix = _block_pixels(pl)
    fills = (65, 130, 130)
    vox = [np.stack([mv.beam(r, c, 9.5, sensor) for r, c in p[:n]]) for p, n in zip(pix, fills)]
    keys = [tuple(np.trunc(v / np.float32(4.0)).astype(int)[0]) for v in vox]
    assert keys == [(2, 0, 0), (0, 2, 0), (-2, 0, 0)]
    for v, k in zip(vox, keys):
        assert (np.trunc(v / np.float32(4.0)).astype(int) == k).all()
    extra = np.stack([mv.beam(r, c, 9.5, sensor) for r, c in pix[1][130:140]])          # finds voxel (0, 2, 0) full
    # several add_cloud calls: the voxels fill over three of them, interleaved in the input
    clouds = [np.concatenate([vox[0][:30], vox[1][:50], vox[2][:64]]),
              np.concatenate([vox[2][64:100], vox[0][30:65], vox[1][50:128]]),
              np.concatenate([vox[1][128:], extra, vox[2][100:]])]
    return sensor, pix, fills, vox, clouds


def _pattern_scan(sensor, pix, fills, remove):
    """One return per stored point's pixel: at 20 m where ``remove(i, n)`` says so (seen through), else at the point's own range."""
    scan = [mv.beam(r, c, 20.0 if remove(i, n) else 9.5, sensor) for p, n in zip(pix, fills) for i, (r, c) in enumerate(p[:n])]
    return np.stack(scan)


PATTERNS = {
    "every_second": (lambda i, n: i % 2 == 1, 32 + 65 + 65, 0),
    "first_block": (lambda i, n: i < 64, 3 * 64, 0),
    "last_point": (lambda i, n: i == n - 1, 3, 0),
    "everything": (lambda i, n: True, 65 + 130 + 130, 3),
}


@pytest.mark.parametrize("name", list(PATTERNS))
def test_compaction_across_blocks(hip, name):
    pl = hip.pipeline
    remove, n_removed, n_emptied = PATTERNS[name]
    sensor, pix, fills, vox, clouds = _block_setup(pl)
    hm = pl.VoxelHashMap(4.0, 100.0, 130)
    dm = pl.DeviceVoxelHashMap(4.0, 100.0, 130, device=0, capacity_voxels=1)
    for c in clouds:
        hm.add_pointcloud(c, np.eye(4)); dm.add_pointcloud(c, np.eye(4))
    assert sorted(len(v) for v in hm._vox.values()) == [65, 130, 130]
    _same(name + " filled", dm, hm)
    scan = _pattern_scan(sensor, pix, fills, remove)
    kw = dict(window=(0, 0), margin=(0.3, 0.02), max_range=50.0)
    want = hm.clear_seen_through(scan, np.eye(4), sensor, **kw)
    assert (want["points_tested"], want["points_removed"], want["voxels_emptied"]) == (325, n_removed, n_emptied)   # by hand
    got = dm.clear_seen_through(scan, np.eye(4), sensor, **kw)
    assert got == want, (got, want)
    _same(name + " cleared", dm, hm)
    cap, tomb, reb = dm.table_info()
    assert (cap, tomb, reb) == (1 << 16, n_emptied, 0)
    if name == "first_block":
        assert sorted(len(v) for v in hm._vox.values()) == [1, 66, 66]
        assert np.array_equal(np.asarray(hm._vox[(2, 0, 0)], np.float32), vox[0][64:])            # the survivor is the 65th point
    # freed room is refilled in input order by the untouched insert
    refill = np.concatenate([np.stack([mv.beam(r, c, 9.6, sensor) for r, c in p[:100]]) for p in pix])
    hm.add_pointcloud(refill, np.eye(4)); dm.add_pointcloud(refill, np.eye(4))
    _same(name + " refilled", dm, hm)
    dm.close()


# ---------------------------------------------------------------------------------------------
# 3. drives
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _drive(hip, sensor_name, n_scans):
    return mv.drive_scans(hip.scans, hip.pipeline.SEG_PRESETS[sensor_name], n_scans, True)


def test_drive_on_a_small_table(hip):
    """OS1-16 (16 384 points per scan), 8 scans past the moving box, a table of 65 536 slots: after every clear and every insert
    (which ends with the range cull) the device map equals the restatement's."""
    pl = hip.pipeline
    sensor = pl.SEG_PRESETS["OS1-16"]
    hm = pl.VoxelHashMap(1.0, 100.0, 20)
    dm = pl.DeviceVoxelHashMap(1.0, 100.0, 20, device=0, capacity_voxels=1)
    removed = 0
    for i, (T, scan) in enumerate(_drive(hip, "OS1-16", 8)):
        assert scan.shape[0] == 16384
        cropped = np.asarray(pl.crop_pointcloud(scan, 1.0, 100.0)[0], np.float32)
        if i > 0:
            want = hm.clear_seen_through(cropped, T, sensor, window=(1, 1), margin=(0.3, 0.02))
            got = dm.clear_seen_through(cropped, T, sensor, window=(1, 1), margin=(0.3, 0.02))
            assert got == want, (i, got, want)
            removed += got["points_removed"]
            _same(f"scan {i} cleared", dm, hm)
        to_map = pl.downsample_uniform(cropped, 0.5)
        hm.add_pointcloud(to_map, T); dm.add_pointcloud(to_map, T)
        _same(f"scan {i} added", dm, hm)
    print(f"OS1-16 drive: {removed} points removed, {len(hm)} voxels, table_info {dm.table_info()}")
    assert removed > 100
    dm.close()


def test_rebuild_after_a_wall_of_voxels_was_cleared(hip):
    """Tombstones made by the clearing count like the range cull's: a crafted scan that returns from 90 m in every direction
    clears everything within 28 m, the next insert finds tombstones * 4 > capacity and rebuilds at unchanged capacity, and the
    live voxels (the ring beyond 28 m) move intact."""
    pl = hip.pipeline
    s = sequence()
    hm = pl.VoxelHashMap(0.5, 30.0, 3)
    dm = pl.DeviceVoxelHashMap(0.5, 30.0, 3, device=0, capacity_voxels=1)
    hm.add_pointcloud(s["c1"], s["P1"]); dm.add_pointcloud(s["c1"], s["P1"])
    wide = pl.SegParams(n_scan=32, horizon_scan=360, ground_scan_ind=7, ang_res_x=1.0, ang_res_y=2.0, ang_bottom=32.0, min_range=1.0)
    sphere = np.stack([mv.beam(r, c, 90.0, wide) for r in range(32) for c in range(360)])
    kw = dict(window=(1, 1), margin=(0.3, 0.02), max_range=28.0)
    want = hm.clear_seen_through(sphere, s["P1"], wide, **kw)
    got = dm.clear_seen_through(sphere, s["P1"], wide, **kw)
    assert got == want
    cap, tomb, reb = dm.table_info()
    live = len(hm)
    print(f"wall cleared: {got}, live {live}, table_info {(cap, tomb, reb)}")
    assert (cap, reb) == (1 << 16, 0) and want["voxels_emptied"] > 10000 and live > 1000
    assert tomb * 4 > cap, "the next insert must find enough tombstones to rebuild"
    _same("wall cleared", dm, hm)
    small = s["c5"][:2000]
    assert (live + small.shape[0]) * 2 <= cap, "the next insert must not grow the table"
    hm.add_pointcloud(small, s["P1"]); dm.add_pointcloud(small, s["P1"])
    cap2, tomb2, reb2 = dm.table_info()
    assert (cap2, reb2) == (cap, 1) and tomb2 < tomb
    _same("rebuilt", dm, hm)
    dm.close()


def test_one_os1_64_step(hip):
    """A 65 536-point scan against the map of five earlier scans: the image is 256 KB."""
    pl = hip.pipeline
    sensor = pl.SEG_PRESETS["OS1-64"]
    hm = pl.VoxelHashMap(1.0, 100.0, 20)
    dm = pl.DeviceVoxelHashMap(1.0, 100.0, 20, device=0)
    scans = _drive(hip, "OS1-64", 6)
    for T, scan in scans[:5]:
        to_map = pl.downsample_uniform(pl.crop_pointcloud(scan, 1.0, 100.0)[0], 0.5)
        hm.add_pointcloud(to_map, T); dm.add_pointcloud(to_map, T)
    T, scan = scans[5]
    assert scan.shape[0] == 65536
    cropped = np.asarray(pl.crop_pointcloud(scan, 1.0, 100.0)[0], np.float32)
    want = hm.clear_seen_through(cropped, T, sensor)
    t = _dev(cropped)
    got = dm.clear_seen_through_device(t.data_ptr(), t.shape[0], T, sensor)
    M = hm.get_map().shape[0] + got["points_removed"]
    print(f"OS1-64 step: {got}, map points before the call {M}")
    assert got == want and got["points_removed"] > 20 and M > 50000 and got["points_tested"] > 0.5 * M
    _same("OS1-64", dm, hm)
    dm.close()


# ---------------------------------------------------------------------------------------------
# 4. two calls
# ---------------------------------------------------------------------------------------------
def test_two_maps_agree_bit_for_bit_and_a_second_call_removes_nothing(hip):
    pl = hip.pipeline
    sensor = pl.SEG_PRESETS["OS1-16"]
    (T0, s0), (T1, s1) = _drive(hip, "OS1-16", 8)[:2]
    maps = [pl.DeviceVoxelHashMap(1.0, 100.0, 20, device=0, capacity_voxels=1) for _ in range(2)]
    rows, stats = [], []
    for dm in maps:
        dm.add_pointcloud(s0, T0)
        stats.append(dm.clear_seen_through(s1, T1, sensor, window=(0, 0)))      # the single-pixel window removes a lot
        dm.get_map(); rows.append(dm.download())
    assert stats[0] == stats[1] and stats[0]["points_removed"] > 100
    assert np.array_equal(rows[0], rows[1])
    again = maps[0].clear_seen_through(s1, T1, sensor, window=(0, 0))            # the survivors were tested against the same image
    assert again["points_removed"] == 0 and again["voxels_emptied"] == 0
    assert again["pixels_filled"] == stats[0]["pixels_filled"]
    maps[0].get_map()
    assert np.array_equal(maps[0].download(), rows[0])
    for dm in maps:
        dm.close()


# ---------------------------------------------------------------------------------------------
# 5. refusals and the surrounding behaviour
# ---------------------------------------------------------------------------------------------
def test_refusals(hip):
    binding = importlib.import_module(hip.__name__ + ".binding")
    pl = hip.pipeline
    L = hip.load_library()
    dm = pl.DeviceVoxelHashMap(1.0, 100.0, 20, device=0, capacity_voxels=1)
    dm.add_pointcloud(np.array([[10, 0, 0], [12, 3, 0]], np.float32), np.eye(4))
    dm.get_map(); before = dm.download()
    scan = np.array([[20, 0, 0]], np.float32)
    dp = C.POINTER(C.c_double)
    R = np.eye(3).reshape(9).copy(); t = np.zeros(3)
    good_s = pl.seg_params_struct(mv.tiny_sensor(pl))
    good_o = binding.VisibilityOptStruct(C.sizeof(binding.VisibilityOptStruct), 1, 1, 0.3, 0.02, 100.0)
    st = binding.VisibilityStatsStruct()

    def call(m=dm._h, xyz=scan.ctypes.data_as(C.c_void_p), n=1, R_=R.ctypes.data_as(dp), t_=t.ctypes.data_as(dp), s=good_s, o=good_o, out=st):
        return L.svnicp_map_clear_seen_through(m, xyz, n, 0, R_, t_, C.byref(s) if s is not None else None,
                                               C.byref(o) if o is not None else None, C.byref(out) if out is not None else None)

    def sensor(**kw):
        s = pl.seg_params_struct(mv.tiny_sensor(pl))
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def opt(**kw):
        o = binding.VisibilityOptStruct(C.sizeof(binding.VisibilityOptStruct), 1, 1, 0.3, 0.02, 100.0)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    nan, inf = float("nan"), float("inf")
    bad = [dict(m=None), dict(xyz=None), dict(R_=None), dict(t_=None), dict(s=None), dict(o=None), dict(out=None),
           dict(n=-1), dict(n=1 << 31),
           dict(s=sensor(struct_size=4)), dict(o=opt(struct_size=4)),
           dict(s=sensor(n_scan=0)), dict(s=sensor(n_scan=129)), dict(s=sensor(horizon_scan=0)), dict(s=sensor(n_scan=128, horizon_scan=4097)),
           dict(s=sensor(ang_res_x=0.0)), dict(s=sensor(ang_res_y=-1.0)), dict(s=sensor(ang_res_x=nan)), dict(s=sensor(ang_res_y=inf)),
           dict(s=sensor(ang_bottom=nan)), dict(s=sensor(min_range=inf)),
           dict(o=opt(window_rows=-1)), dict(o=opt(window_rows=5)), dict(o=opt(window_cols=-1)), dict(o=opt(window_cols=9)),
           dict(o=opt(margin_abs=-0.1)), dict(o=opt(margin_abs=nan)), dict(o=opt(margin_rel=-0.1)), dict(o=opt(margin_rel=inf)),
           dict(o=opt(max_range=0.0)), dict(o=opt(max_range=-1.0)), dict(o=opt(max_range=inf)), dict(o=opt(max_range=nan))]
    for kw in bad:
        assert call(**kw) == ERR_INVALID, kw
    dm.get_map()
    assert np.array_equal(dm.download(), before)               # nothing was enqueued
    # n = 0 and an empty map: success, zero statistics
    st.points_removed = 7
    assert call(n=0) == 0 and (st.pixels_filled, st.points_tested, st.points_removed, st.voxels_emptied) == (0, 0, 0, 0)
    empty = pl.DeviceVoxelHashMap(1.0, 100.0, 20, device=0, capacity_voxels=1)
    assert empty.clear_seen_through(scan, np.eye(4), mv.tiny_sensor(pl)) == dict.fromkeys(pl.VISIBILITY_STATS, 0)
    assert call() == 0 and st.points_removed == 1              # the good call does work
    empty.close(); dm.close()


def test_query_normals_refused_until_the_next_query_then_equal_to_the_restatement(hip):
    pl = hip.pipeline
    L = hip.load_library()
    sensor = pl.SEG_PRESETS["OS1-16"]
    (T0, s0), (T1, s1) = _drive(hip, "OS1-16", 8)[:2]
    hm = pl.VoxelHashMap(1.0, 100.0, 20)
    dm = pl.DeviceVoxelHashMap(1.0, 100.0, 20, device=0, capacity_voxels=1)
    hm.add_pointcloud(s0, T0); dm.add_pointcloud(s0, T0)
    dm.get_map()
    assert dm.get_map_normals(8)[1] > 0
    want = hm.clear_seen_through(s1, T1, sensor, window=(0, 0))
    assert dm.clear_seen_through(s1, T1, sensor, window=(0, 0)) == want and want["points_removed"] > 100
    n = C.c_int64(-1)
    assert L.svnicp_map_query_normals(dm._h, 8, C.byref(n)) == ERR_INVALID
    assert b"clear_seen_through" in L.svnicp_map_last_error(dm._h)
    assert not L.svnicp_map_normals_devptr(dm._h)
    _, M = dm.get_map()
    _, with_normal = dm.get_map_normals(8)
    n_dev = dm.download_normals()
    ref = mr.map_normals(hm._vox, 8)
    assert M == ref.points.shape[0] and np.array_equal(dm.download(), ref.points)
    near, low_gap = mc.left_out(ref)
    valid = (n_dev != 0.0).any(axis=1)
    assert np.array_equal(valid[~near], ref.valid[~near]) and near.sum() <= 0.01 * M
    cmp = valid & ref.valid & ~low_gap
    dev = 1.0 - np.abs((n_dev[cmp] * ref.normals[cmp]).sum(axis=1))
    print(f"normals on the cleared map: {M} rows, {with_normal} with a normal, compared {int(cmp.sum())}, max 1 - |n.n_ref| = {dev.max():.3e}")
    assert cmp.sum() > 1000 and dev.max() <= 1e-9
    assert with_normal == int(valid.sum())
    dm.close()


# ---------------------------------------------------------------------------------------------
# 6. the Python pipeline
# ---------------------------------------------------------------------------------------------
def _pipeline(hip, clear, gpu):
    pl = hip.pipeline
    kw = {} if clear == "absent" else dict(clear_seen_through=clear)
    cfg = pl.PipelineConfig(min_range=1.0, max_range=80.0, voxel_size=1.0, map_voxel_size=1.0, map_voxel_max_points=20, map_range=100.0,
                            particle_count=16, gpu_map=gpu, gpu_prep=gpu, seg_params=pl.SEG_PRESETS["OS1-16"],
                            solver=hip.SteinICPParam(iterations=10, lr=1.0, max_dist=1.0, KNN_count=20, SVN_full_grad=False), **kw)
    pipe = pl.RegistrationPipeline(cfg, device=0)
    res = [pipe.process_scan(scan, 0.1 * i) for i, (_, scan) in enumerate(_drive(hip, "OS1-16", 8)[:5])]
    if gpu:
        pipe.map.get_map()
        rows = pipe.map.download()
    else:
        rows = _host_rows(pipe.map)
    return res, rows


FIELDS = ("stamp", "pose", "initial_guess", "correction", "variance", "cov", "particles", "weights", "state", "with_normal", "fitness",
          "inlier_rmse", "plane_rmse", "plane_inliers", "information", "modes", "cleared")


def _equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_python_pipeline_clears_like_the_host_map_pipeline(hip):
    """gpu_map + gpu_prep (the cropped cloud never leaves HBM) against the host-map pipeline on the moving-box drive: the same
    ScanResult.cleared per scan and equal final maps.  (Both pipelines hand the solver the same rows, and the solver is
    reproducible, so the poses — which the clearing reads — are equal.)"""
    dev, dev_rows = _pipeline(hip, (1, 1, 0.3, 0.02), True)
    host, host_rows = _pipeline(hip, (1, 1, 0.3, 0.02), False)
    print("cleared per scan:", [r.cleared for r in dev], "host map:", [r.cleared for r in host])
    assert dev[0].cleared is None and all(r.cleared is not None for r in dev[1:])
    assert [r.cleared for r in dev] == [r.cleared for r in host]
    assert sum(r.cleared for r in dev[1:]) > 0
    assert np.array_equal(dev_rows, host_rows)


def test_python_pipeline_without_the_switch_is_unchanged(hip, monkeypatch):
    pl = hip.pipeline
    calls = []
    monkeypatch.setattr(pl.DeviceVoxelHashMap, "_clear_seen_through", lambda self, *a, **k: calls.append(a))
    off, off_rows = _pipeline(hip, None, True)
    absent, absent_rows = _pipeline(hip, "absent", True)
    assert not calls                                            # no call is made
    for a, b in zip(off, absent):
        for f in FIELDS:
            assert _equal(getattr(a, f), getattr(b, f)), f
        assert a.cleared is None
    assert np.array_equal(off_rows, absent_rows)


# ---------------------------------------------------------------------------------------------
# 7. the C++ drive
# ---------------------------------------------------------------------------------------------
def test_cpp_drive_clears_like_python(hip, tmp_path):
    """pipeline_drive with its clear switch (PipelineConfig::clear_seen_through, window 1 x 1, margins 0.3 m / 0.02, HDL-64E) with
    the host map and with the device map + device pre-processing, against pipeline.py on the same scans and particles: poses to
    1e-9 (the existing drive test's tolerance), the same points_removed per registered scan in all three."""
    from test_pipeline_gpu import _build_pipeline_drive
    pl, sc = hip.pipeline, hip.scans
    root = os.path.dirname(os.path.dirname(hip.library_path()))
    exe = _build_pipeline_drive(root)
    P, I, K, voxel, n_scans = 16, 10, 30, 0.5, 5
    base = sc.make_scene()
    rng = np.random.default_rng(5)
    scans, parts = [], []
    for k in range(n_scans):
        lo, hi = mv.box_bounds(k)
        lo[0] += 12.0; hi[0] += 12.0                          # the box 4 m ahead of the sensor, leaving at 1.3 m per scan
        scene = sc.Scene(np.vstack([base.boxes_lo, lo]), np.vstack([base.boxes_hi, hi]))
        t = np.array([0.2 * k, 0.0, 0.0])
        scans.append((0.1 * k, sc.lidar_scan(scene, np.eye(3), t, 16384, stream=900 + k).astype(np.float32)))
        parts.append(hip.initialize_particles(P, pl.PRIOR_UB, pl.PRIOR_LB, rng))
    with open(tmp_path / "scans.bin", "wb") as f:
        f.write(struct.pack("<i", n_scans))
        for stamp, pts in scans:
            f.write(struct.pack("<di", stamp, pts.shape[0])); f.write(np.ascontiguousarray(pts[:, :3], np.float32).tobytes())
    with open(tmp_path / "particles.bin", "wb") as f:
        for p in parts:
            f.write(np.ascontiguousarray(p, np.float64).tobytes())

    def run(gpu_map):
        out = tmp_path / f"out{gpu_map}.bin"
        r = subprocess.run([exe, str(tmp_path / "scans.bin"), str(out), str(P), str(I), str(K), str(voxel), str(tmp_path / "particles.bin"),
                            str(gpu_map), "0", "0", "0", "0", "off", "off", "0", "0", "1"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        cleared = {int(l.split()[1].rstrip(":")): int(l.split()[2]) for l in r.stdout.splitlines() if l.startswith("clear ")}
        raw = open(out, "rb").read()
        poses, off = [], 0
        for k in range(n_scans):
            off += 4
            poses.append(np.frombuffer(raw, "<f8", 12, off)); off += 8 * (12 + 12 + 6 + 6 + 36)
            B, M = (int(v) for v in np.frombuffer(raw, "<i8", 2, off)); off += 16 + 8 * (3 * B + 3 * M + 6 * P)
        assert off == len(raw)
        return cleared, poses

    c_host, p_host = run(0)
    c_dev, p_dev = run(2)
    print("C++ cleared per scan, host map:", c_host, "device map:", c_dev)
    assert sorted(c_host) == list(range(1, n_scans)) and c_host == c_dev
    assert all(np.array_equal(a, b) for a, b in zip(p_host, p_dev))
    cfg = pl.PipelineConfig(min_range=1.0, max_range=80.0, voxel_size=voxel, map_voxel_size=voxel, map_voxel_max_points=20, map_range=100.0,
                            particle_count=P, gpu_map=True, clear_seen_through=(1, 1, 0.3, 0.02),
                            solver=hip.SteinICPParam(iterations=I, lr=1.0, max_dist=1.0, KNN_count=K, SVN_full_grad=False))
    pipe = pl.RegistrationPipeline(cfg, device=0)
    it = iter(parts)
    pipe._particles = lambda: next(it)
    for k, (stamp, pts) in enumerate(scans):
        res = pipe.process_scan(pts, stamp)
        T = np.eye(4); T[:3, :3] = p_host[k][:9].reshape(3, 3); T[:3, 3] = p_host[k][9:]
        assert np.allclose(res.pose, T, rtol=0, atol=1e-9), k
        assert res.cleared == c_host.get(k), k
    assert sum(c_host.values()) > 0
