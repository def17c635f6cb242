"""Range-image segmentation on the device (svnicp_prep_segment, csrc/range_segment.hip) against the host restatement of LeGO-LOAM's
ImageProjection::cloudHandler in svn-icp_amd/pipeline.py (segment_scan / segment_images): the segmented cloud, its input
indices and the four images bit for bit, on dense, bin-edge, moving and degenerate scans and on every sensor preset; and the
scan-to-map loop with PipelineConfig.segmentation in the Python (host and device) and C++ pipelines."""
import importlib
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pl(hip):
    return importlib.import_module(hip.__name__ + ".pipeline")


@pytest.fixture(scope="module")
def prep(pl):
    p = pl.DevicePreprocessor(0)
    yield p
    p.close()


def _pose(yaw=0.4, t=(2.0, -1.0, 0.0)):
    R = np.eye(3)
    c, s = np.cos(yaw), np.sin(yaw)
    R[:2, :2] = [[c, -s], [s, c]]
    return R, np.asarray(t, float)


def _grid(hip, prm, stream=5, noise=0.02):
    R, t = _pose()
    return hip.scans.lidar_grid_scan(hip.scans.make_scene(), R, t, prm, stream, noise=noise)


def _bin_edge(hip, n, stream=3):
    R, t = _pose(-0.7, (1.0, 3.0, 0.2))
    return hip.scans.lidar_scan(hip.scans.make_scene(), R, t, n, stream)


def _sweep(hip, n, stream=9):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = _pose(0.2, (-3.0, 1.0, 0.1))
    return hip.scans.lidar_sweep(hip.scans.make_scene(), T, [0.004, -0.006, 0.05, 0.8, 0.1, -0.03], n, stream).points


def _check(pl, prep, pts, prm=None):
    """device cloud, indices and images == host, bit for bit"""
    prm = prm or pl.SegParams()
    n = prep.segment(pts, prm)
    xyz, idx = prep.download_segmented()
    hx, hi = pl.segment_scan(pts, prm)
    assert n == hx.shape[0] == xyz.shape[0]
    assert np.array_equal(idx, hi)
    assert np.array_equal(xyz.view(np.uint32), hx.view(np.uint32))
    for d, h, name in zip(prep.download_seg_images(), pl.segment_images(pts, prm), ("owner", "range", "ground", "label")):
        assert d.dtype == h.dtype and d.shape == h.shape, name
        assert np.array_equal(d.view(np.uint8), h.view(np.uint8)), (name, int((d != h).sum()))
    return n


@pytest.mark.parametrize("n", [1, 777, 65536, 131072, 288000])
def test_device_segment_equals_host_on_bin_edge_scans(hip, pl, prep, n):
    pts = _bin_edge(hip, n)
    if n == 1:
        pts = np.array([[10.0, 2.0, -1.0]])
    assert _check(pl, prep, pts) >= {1: 0, 777: 1}.get(n, 100)


def test_device_segment_equals_host_on_grid_and_sweep_scans(hip, pl, prep):
    prm = pl.SEG_PRESETS["HDL-64E"]
    assert _check(pl, prep, _grid(hip, prm), prm) > 10000
    assert _check(pl, prep, _sweep(hip, 131072), prm) > 1000


def test_device_segment_drops_non_finite_points_and_keeps_indices(hip, pl, prep):
    pts = _bin_edge(hip, 65536).astype(np.float32)
    rng = np.random.default_rng(4)
    bad = rng.choice(pts.shape[0], 3000, replace=False)
    pts[bad[:1000], 0] = np.nan
    pts[bad[1000:2000], 1] = np.inf
    pts[bad[2000:], 2] = -np.inf
    _check(pl, prep, pts)
    _, idx = prep.download_segmented()
    assert not np.isin(idx, bad).any()


def test_device_segment_everything_dropped(hip, pl, prep):
    pts = np.full((5000, 3), 0.1, np.float32)               # inside min_range
    assert _check(pl, prep, pts) == 0
    assert _check(pl, prep, np.zeros((0, 3), np.float32)) == 0


def test_device_segment_device_pointer_input(hip, pl, prep):
    import torch
    pts = _bin_edge(hip, 131072, stream=12).astype(np.float32)
    n = prep.segment(torch.from_numpy(pts).to("cuda:0"))
    assert prep.bytes_uploaded == 0
    hx, hi = pl.segment_scan(pts)
    xyz, idx = prep.download_segmented()
    assert n == hx.shape[0]
    assert np.array_equal(xyz, hx) and np.array_equal(idx, hi)


@pytest.mark.parametrize("name", ["VLP-16", "HDL-32E", "HDL-64E", "VLS-128", "RS-LIDAR-32", "OS1-16", "OS1-64", "OS0-128"])
def test_device_segment_every_preset(hip, pl, prep, name):
    prm = pl.SEG_PRESETS[name]
    assert _check(pl, prep, _grid(hip, prm, stream=21), prm) > 100


def test_device_segment_is_deterministic_and_reusable(hip, pl, prep):
    pts = _grid(hip, pl.SEG_PRESETS["HDL-64E"], stream=33)
    prep.segment(pts)
    first = prep.download_segmented(), prep.download_seg_images()
    for k in range(3):
        prep.segment(pts)
        again = prep.download_segmented(), prep.download_seg_images()
        assert all(np.array_equal(a, b) for a, b in zip(first[0] + first[1], again[0] + again[1]))
    # changing sizes and presets on one object
    for name, n in (("VLP-16", 777), ("OS0-128", 131072), ("HDL-64E", 4096), ("VLS-128", 288000), ("HDL-32E", 1)):
        pts = _bin_edge(hip, n, stream=40 + n % 7) if n > 1 else np.array([[5.0, 1.0, 0.0]])
        _check(pl, prep, pts, pl.SEG_PRESETS[name])


def test_device_segment_refuses_invalid_params(hip, pl, prep):
    from dataclasses import replace
    base = pl.SEG_PRESETS["HDL-64E"]
    bad = [replace(base, ground_scan_ind=0), replace(base, ground_scan_ind=64), replace(base, n_scan=129, ground_scan_ind=7),
           replace(base, horizon_scan=8193), replace(base, ang_res_x=0.0), replace(base, ang_res_y=float("nan")),
           replace(base, ang_res_y=-0.4), replace(base, segment_theta=float("inf"))]
    pts = _bin_edge(hip, 4096)
    for prm in bad:
        with pytest.raises(hip.SvnIcpError, match="svnicp_prep_segment"):
            prep.segment(pts, prm)
    import ctypes as C
    s = pl.seg_params_struct(base)
    s.struct_size = 44
    out = C.c_int64(0)
    assert prep._L.svnicp_prep_segment(prep._h, None, 0, 0, C.byref(s), C.byref(out)) == -1
    assert b"struct_size" in prep._L.svnicp_prep_last_error(prep._h)
    _check(pl, prep, pts, base)                                # a later valid call still works


def test_segmented_pointer_feeds_the_scan_preprocessing(hip, pl, prep):
    pts = _grid(hip, pl.SEG_PRESETS["HDL-64E"], stream=8)
    n = prep.segment(pts)
    smr = prep.scan_device(prep.segmented_ptr, n, 1.0, 80.0, 0.5, 3.0)
    hx, _ = pl.segment_scan(pts)
    cropped, smr_h = pl.crop_pointcloud(hx, 1.0, 80.0, 3.0)
    to_map = pl.downsample_uniform(cropped, 0.25)
    source = pl.downsample_uniform(to_map, 0.75)
    assert smr == smr_h
    assert np.array_equal(prep.download(0).astype(np.float64), cropped)
    assert np.array_equal(prep.download(1).astype(np.float64), to_map)
    assert np.array_equal(prep.download(2).astype(np.float64), source)
    xyz, _ = prep.download_segmented()                         # the pre-processing did not write the segment buffers
    assert np.array_equal(xyz, hx)


# ----------------------------------------------------------------------------- the pipelines with segmentation
P_, I_, K_, VOXEL = 16, 10, 20, 0.5


def _drive(hip, pl, n_scans=5):
    sc = hip.scans
    scene = sc.make_scene()
    prm = pl.SEG_PRESETS["HDL-64E"]
    rng = np.random.default_rng(23)
    scans, parts = [], []
    for k in range(n_scans):
        R, t = sc.rot_zyx(0.0, 0.0, np.radians(0.4 * k)), np.array([0.08 * k, 0.0, 0.0])
        scans.append((0.1 * k, sc.lidar_grid_scan(scene, R, t, prm, 800 + k).astype(np.float32)))
        parts.append(hip.initialize_particles(P_, pl.PRIOR_UB, pl.PRIOR_LB, rng))
    return scans, parts


def _cfg(hip, pl, **kw):
    return pl.PipelineConfig(min_range=1.0, max_range=80.0, voxel_size=VOXEL, map_voxel_size=VOXEL, map_voxel_max_points=20,
                             map_range=100.0, particle_count=P_,
                             solver=hip.SteinICPParam(iterations=I_, lr=1.0, max_dist=1.0, KNN_count=K_, SVN_full_grad=False), **kw)


def _run(pl, cfg, scans, parts):
    pipe = pl.RegistrationPipeline(cfg, device=0)
    it = iter(parts)
    pipe._particles = lambda: next(it)
    poses = [pipe.process_scan(pts, stamp).pose for stamp, pts in scans]
    return pipe, poses


@pytest.fixture(scope="module")
def drive(hip, pl):
    scans, parts = _drive(hip, pl)
    _, host = _run(pl, _cfg(hip, pl, segmentation=True), scans, parts)
    return scans, parts, host


def test_pipeline_segmentation_host_equals_device(hip, pl, drive):
    scans, parts, host = drive
    pipe, dev = _run(pl, _cfg(hip, pl, segmentation=True, gpu_map=True, gpu_prep=True), scans, parts)
    for k, (a, b) in enumerate(zip(host, dev)):
        assert np.allclose(a, b, rtol=0, atol=1e-9), k
    assert pipe.bytes_h2d == sum(pts.nbytes for _, pts in scans)          # the raw scans, once each
    seg, _ = pl.segment_scan(scans[-1][1])
    cropped, _ = pl.crop_pointcloud(seg, 1.0, 80.0)
    source = pl.downsample_uniform(pl.downsample_uniform(cropped, 0.5 * VOXEL), 1.5 * VOXEL)
    assert np.array_equal(pipe._prep.download(2).astype(np.float64), np.asarray(source, np.float64))
    assert pipe._prep.n_segmented == seg.shape[0]


def test_pipeline_segmentation_off_is_unchanged(hip, pl, drive):
    scans, parts, seg_poses = drive
    _, off = _run(pl, _cfg(hip, pl, segmentation=False), scans, parts)
    _, default = _run(pl, _cfg(hip, pl), scans, parts)
    assert all(np.array_equal(a, b) for a, b in zip(off, default))
    assert not all(np.array_equal(a, b) for a, b in zip(off[1:], seg_poses[1:]))   # segmentation changes the source clouds


def test_pipeline_drive_segment_equals_python(hip, pl, drive, tmp_path):
    scans, parts, host = drive
    exe = str(tmp_path / "pipeline_drive")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "svn-icp_amd", "host"), os.path.join(ROOT, "svn-icp_amd", "host", "pipeline_drive.cpp"),
                           "-L", os.path.join(ROOT, "svn-icp_amd"), "-lsvnicp_hip", "-Wl,-rpath," + os.path.join(ROOT, "svn-icp_amd"),
                           "-o", exe])
    with open(tmp_path / "scans.bin", "wb") as f:
        f.write(struct.pack("<i", len(scans)))
        for stamp, pts in scans:
            f.write(struct.pack("<di", stamp, pts.shape[0])); f.write(np.ascontiguousarray(pts, np.float32).tobytes())
    with open(tmp_path / "particles.bin", "wb") as f:
        for p in parts:
            f.write(np.ascontiguousarray(p, np.float64).tobytes())
    seg, _ = pl.segment_scan(scans[-1][1])
    cropped, _ = pl.crop_pointcloud(seg, 1.0, 80.0)
    source = np.asarray(pl.downsample_uniform(pl.downsample_uniform(cropped, 0.5 * VOXEL), 1.5 * VOXEL), np.float64)
    for gpu_map in ("0", "2"):
        out = tmp_path / f"out{gpu_map}.bin"
        r = subprocess.run([exe, str(tmp_path / "scans.bin"), str(out), str(P_), str(I_), str(K_), str(VOXEL), str(tmp_path / "particles.bin"),
                            gpu_map, "0", "1"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        raw, off = open(out, "rb").read(), 0
        for k in range(len(scans)):
            off += 4
            pose = np.frombuffer(raw, "<f8", 12, off); off += 96 + 96 + 48 + 48 + 288
            B, M = (int(v) for v in np.frombuffer(raw, "<i8", 2, off)); off += 16
            src = np.frombuffer(raw, "<f8", 3 * B, off).reshape(B, 3); off += 24 * B + 24 * M + 48 * P_
            T = np.eye(4); T[:3, :3] = pose[:9].reshape(3, 3); T[:3, 3] = pose[9:]
            assert np.allclose(T, host[k], rtol=0, atol=1e-9), (gpu_map, k)
            if k == len(scans) - 1:
                assert np.array_equal(src, source), gpu_map
        assert off == len(raw)
