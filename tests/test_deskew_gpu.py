"""Deskew on the device (svnicp_prep_scan_deskew, csrc/scan_prep.hip: k_deskew_stamps + k_deskew_crop) against the host
restatement of OdometryPipeline::deskew_pointcloud (OdometryPipeline.cpp:357-447) in svn-icp_amd/pipeline.py, and the whole
scan-to-map loop with PipelineConfig.deskew on a drive whose sweeps are skewed by the sensor's own motion."""
import importlib
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DELTA = np.array([0.004, -0.006, 0.05, 0.8, 0.1, -0.03])   # [omega, v] over one sweep


@pytest.fixture(scope="module")
def pl(hip):
    return importlib.import_module(hip.__name__ + ".pipeline")


def _sweep(hip, n, stream, delta=DELTA, noise=0.02):
    sc = hip.scans
    T = np.eye(4)
    T[:3, :3] = sc.rot_zyx(0.0, 0.0, 0.4)
    T[:3, 3] = [2.0, -1.0, 0.0]
    return sc.lidar_sweep(sc.make_scene(), T, delta, n, stream=stream, noise=noise, t0=1234.5)


def _ulp_err(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    u = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / u


def _check(pl, prep, pts, stamps, delta, kitti, rmin=1.0, rmax=80.0, voxel=0.5, smr0=3.0):
    """device deskew + crop + samplings vs host: the tap within 1 ulp of deskew_pointcloud, everything downstream of the tap
    bit for bit equal to crop_pointcloud + downsample_uniform of the tap"""
    smr_d = prep.scan(pts, rmin, rmax, voxel, smr0, stamps=stamps, delta=delta, kitti=kitti)
    tap = prep.download_deskewed()
    host = pl.deskew_pointcloud(pts, None if stamps is None or kitti else np.asarray(stamps), delta, kitti)
    assert tap.shape == host.shape
    assert np.array_equal(np.isnan(tap), np.isnan(host))
    fin = ~np.isnan(tap)
    e = _ulp_err(tap[fin], host[fin])
    assert e.size == 0 or e.max() <= 1.0, e.max()
    cropped, smr = pl.crop_pointcloud(tap, rmin, rmax, smr0)
    to_map = pl.downsample_uniform(cropped, 0.5 * voxel)
    source = pl.downsample_uniform(to_map, 1.5 * voxel)
    assert smr_d == smr
    assert (prep.n_cropped, prep.n_map, prep.n_source) == (cropped.shape[0], to_map.shape[0], source.shape[0])
    assert np.array_equal(prep.download(0).astype(np.float64), cropped)
    assert np.array_equal(prep.download(1).astype(np.float64), to_map)
    assert np.array_equal(prep.download(2).astype(np.float64), source)
    return tap, int((e > 0).sum())


@pytest.mark.parametrize("n", [777, 4096, 65536, 131072])
def test_device_deskew_equals_host(hip, pl, n):
    sw = _sweep(hip, n, 600 + n % 89)
    pts = sw.points.astype(np.float32)
    prep = pl.DevicePreprocessor(device=0)
    diffs = {}
    for name, st in (("f64", sw.stamps), ("f32", sw.stamps.astype(np.float32)), ("u32", sw.stamps_ns)):
        tap, diffs[name] = _check(pl, prep, pts, st, DELTA, False)
        assert not np.array_equal(tap, pts)
    _, diffs["kitti"] = _check(pl, prep, pts, None, DELTA, True)
    print(f"n={n}: coordinates 1 ulp off the host restatement: {diffs}")


def test_device_deskew_degenerate_stamps_and_nan_points(hip, pl):
    sw = _sweep(hip, 8192, 611)
    pts = sw.points.astype(np.float32)
    prep = pl.DevicePreprocessor(device=0)
    # min == max: the raw scan (:418), in KITTI mode without the correction
    tap, _ = _check(pl, prep, pts, np.full(pts.shape[0], 5.0), DELTA, False)
    assert np.array_equal(tap, pts)
    tap, _ = _check(pl, prep, pts, np.full(pts.shape[0], 17, np.uint32), DELTA, False)
    assert np.array_equal(tap, pts)
    same = np.tile(np.array([[10.0, 10.0, 1.0]], np.float32), (300, 1))
    tap, _ = _check(pl, prep, same, None, DELTA, True)
    assert np.array_equal(tap, same)
    # no stamp field: the raw scan
    tap, _ = _check(pl, prep, pts, None, DELTA, False)
    assert np.array_equal(tap, pts)
    # NaN points and non-finite stamps: out of min / max, NaN after the deskew, dropped by the crop
    bad = pts.copy()
    bad[[7, 700, 7000]] = np.nan
    st = sw.stamps.copy()
    st[[9, 900]] = [np.nan, np.inf]
    tap, _ = _check(pl, prep, bad, st, DELTA, False)
    assert np.isnan(tap[[7, 700, 7000, 9, 900]]).all()
    _check(pl, prep, bad, None, DELTA, True)
    # every stamp non-finite: nothing to normalise by, the raw scan
    tap, _ = _check(pl, prep, pts, np.full(pts.shape[0], np.nan), DELTA, False)
    assert np.array_equal(tap, pts)


def test_invalid_arguments_are_refused(hip, pl):
    import ctypes as C
    prep = pl.DevicePreprocessor(device=0)
    L = prep._L
    pts = np.ones((10, 3), np.float32)
    st = np.arange(10, dtype=np.float64)
    smr = C.c_double(0.0)
    cnt = [C.c_int64(0) for _ in range(3)]

    def call(stype, delta, flags=0):
        dp = None if delta is None else np.ascontiguousarray(delta, np.float64).ctypes.data_as(C.POINTER(C.c_double))
        return L.svnicp_prep_scan_deskew(prep._h, pts.ctypes.data_as(C.c_void_p), st.ctypes.data_as(C.c_void_p), stype, 10, 0, dp, flags,
                                         1.0, 100.0, 1.0, C.byref(smr), *(C.byref(c) for c in cnt))
    assert call(3, np.zeros(6)) == -1 and call(-1, np.zeros(6)) == -1
    assert call(0, None) == -1
    assert call(0, np.array([0, 0, np.nan, 0, 0, 0])) == -1 and call(0, np.array([0, 0, 0, np.inf, 0, 0])) == -1
    assert call(0, np.zeros(6), flags=2) == -1
    assert call(0, np.zeros(6)) == 0


def test_zero_motion_equals_prep_scan_and_alternating_calls(hip, pl):
    """δ = 0 gives svnicp_prep_scan's outputs bit for bit; alternating the two entry points on one object with changing sizes
    gives each its own result."""
    prep = pl.DevicePreprocessor(device=0)
    ref = pl.DevicePreprocessor(device=0)
    for k, n in enumerate((65536, 3000, 131072, 777, 20000)):
        sw = _sweep(hip, n, 620 + k)
        pts = sw.points.astype(np.float32)
        smr_a = ref.scan(pts, 1.0, 80.0, 0.5, 2.0)
        smr_b = prep.scan(pts, 1.0, 80.0, 0.5, 2.0, stamps=sw.stamps, delta=np.zeros(6))
        assert smr_a == smr_b and (ref.n_cropped, ref.n_map, ref.n_source) == (prep.n_cropped, prep.n_map, prep.n_source)
        for w in (0, 1, 2):
            assert np.array_equal(ref.download(w), prep.download(w))
        # alternate on ONE object: plain scan, then a deskew, then a plain scan of a different size
        smr_c = prep.scan(pts, 1.0, 80.0, 0.5, 2.0)
        assert smr_c == smr_a and np.array_equal(prep.download(2), ref.download(2))
        _check(pl, prep, pts, sw.stamps, DELTA, False, smr0=2.0)
        other = pts[: max(64, n // 3)]
        cropped, smr = pl.crop_pointcloud(other, 1.0, 80.0, 2.0)
        assert prep.scan(other, 1.0, 80.0, 0.5, 2.0) == smr
        assert np.array_equal(prep.download(2).astype(np.float64), pl.downsample_uniform(pl.downsample_uniform(cropped, 0.25), 0.75))


def test_device_resident_inputs(hip, pl):
    import torch
    sw = _sweep(hip, 65536, 630)
    pts = sw.points.astype(np.float32)
    prep = pl.DevicePreprocessor(device=0)
    for st in (sw.stamps, sw.stamps.astype(np.float32), sw.stamps_ns):
        smr_h = prep.scan(pts, 1.0, 80.0, 0.5, 0.0, stamps=st, delta=DELTA)
        assert prep.bytes_uploaded == pts.nbytes + st.nbytes
        host = [prep.download(w) for w in (0, 1, 2)] + [prep.download_deskewed()]
        tp = torch.from_numpy(pts).cuda()
        ts = torch.from_numpy(st).cuda()
        smr_d = prep.scan(tp, 1.0, 80.0, 0.5, 0.0, stamps=ts, delta=DELTA)
        assert prep.bytes_uploaded == 0
        assert smr_d == smr_h
        dev = [prep.download(w) for w in (0, 1, 2)] + [prep.download_deskewed()]
        for a, b in zip(host, dev):
            assert np.array_equal(a, b)
    prep.scan(torch.from_numpy(pts).cuda(), 1.0, 80.0, 0.5, 0.0, delta=DELTA, kitti=True)
    dev = [prep.download(w) for w in (0, 1, 2)] + [prep.download_deskewed()]
    _check(pl, prep, pts, None, DELTA, True, smr0=0.0)
    for a, b in zip(dev, [prep.download(w) for w in (0, 1, 2)] + [prep.download_deskewed()]):
        assert np.array_equal(a, b)


# ----------------------------------------------------------------------------- end to end
# The sweep period equals the frame gap.  The sensor stands still for two frames (the map is seeded with an unskewed scan and
# the first deskew sees zero motion), then its twist per sweep ramps up to DRIVE_DELTA over RAMP frames and stays there: the
# constant-velocity prediction is off by one ramp increment per frame, which the solver recovers (a full step from rest it
# does not: 3 deg of yaw is 1.5 m at 30 m, beyond max_dist).  Frame k's columns fire from T_k · Exp((s_c − 0.5)·δ_k), and
# T_{k+1} = T_k · Exp(δ_k / 2) · Exp(δ_{k+1} / 2): the sensor path is continuous across sweeps.
DRIVE_DELTA = np.array([0.0, 0.0, np.radians(3.0), 0.6, 0.0, 0.0])
N_FRAMES, RAMP, N_POINTS, P, ITERS, KNN, VOXEL = 12, 6, 32768, 24, 20, 40, 0.5
PERIOD = 0.1


def _twists(delta, ramp):
    return [delta * min(1.0, max(0.0, (k - 1) / ramp)) for k in range(N_FRAMES)]


def _drive(hip, delta=None, ramp=None):
    sc = hip.scans
    pl = importlib.import_module(hip.__name__ + ".pipeline")
    scene = sc.make_scene()
    frames, truth = [], []
    d = _twists(DRIVE_DELTA if delta is None else delta, RAMP if ramp is None else ramp)
    T = np.eye(4)
    for k in range(N_FRAMES):
        if k:
            T = T @ pl.se3_exp(0.5 * d[k - 1]) @ pl.se3_exp(0.5 * d[k])
        sw = sc.lidar_sweep(scene, T, d[k], N_POINTS, stream=800 + k, period=PERIOD, t0=k * PERIOD)
        frames.append((k * PERIOD, sw.points.astype(np.float32), sw.stamps))
        truth.append(T.copy())
    rng = np.random.default_rng(5)
    parts = [hip.initialize_particles(P, pl.PRIOR_UB, pl.PRIOR_LB, rng) for _ in range(N_FRAMES)]
    return frames, truth, parts


def _cfg(hip, pl, **kw):
    return pl.PipelineConfig(min_range=1.0, max_range=80.0, voxel_size=VOXEL, map_voxel_size=VOXEL, map_voxel_max_points=20, map_range=100.0,
                             particle_count=P, solver=hip.SteinICPParam(iterations=ITERS, lr=1.0, max_dist=1.0, KNN_count=KNN, SVN_full_grad=False),
                             **kw)


def _run(hip, pl, frames, parts, **kw):
    pipe = pl.RegistrationPipeline(_cfg(hip, pl, **kw), device=0)
    it = iter(parts)
    pipe._particles = lambda: next(it)
    return [pipe.process_scan(pts, stamp, point_stamps=st).pose.copy() for stamp, pts, st in frames]


def _errors(pl, truth, poses):
    rot = [float(np.linalg.norm(pl.so3_log(T[:3, :3].T @ E[:3, :3]))) for T, E in zip(truth, poses)]
    tr = [float(np.linalg.norm(T[:3, 3] - E[:3, 3])) for T, E in zip(truth, poses)]
    return np.array(rot), np.array(tr)


def test_deskewed_drive_host_device_and_cpp_agree_and_beat_the_skewed_drive(hip, pl, tmp_path):
    frames, truth, parts = _drive(hip)
    host = _run(hip, pl, frames, parts, deskew=True)
    dev = _run(hip, pl, frames, parts, deskew=True, gpu_map=True, gpu_prep=True)
    raw = _run(hip, pl, frames, parts)
    for k, (a, b) in enumerate(zip(host, dev)):
        assert np.allclose(a, b, rtol=0, atol=1e-9), k
    # the C++ pipeline (registration_pipeline.hpp) on the same drive, host pre-processing and device pre-processing
    root = os.path.dirname(os.path.dirname(hip.library_path()))
    exe = str(tmp_path / "pipeline_drive")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-I",
                           os.path.join(root, "svn-icp_amd", "host"), os.path.join(root, "svn-icp_amd", "host", "pipeline_drive.cpp"),
                           "-L", os.path.join(root, "svn-icp_amd"), "-lsvnicp_hip", "-Wl,-rpath," + os.path.join(root, "svn-icp_amd"), "-o", exe])
    with open(tmp_path / "scans.bin", "wb") as f:
        f.write(struct.pack("<i", len(frames)))
        for stamp, pts, st in frames:
            f.write(struct.pack("<di", stamp, pts.shape[0])); f.write(np.ascontiguousarray(pts, "<f4").tobytes())
            f.write(np.ascontiguousarray(st, "<f8").tobytes())
    with open(tmp_path / "particles.bin", "wb") as f:
        for p in parts:
            f.write(np.ascontiguousarray(p, np.float64).tobytes())
    for mode in ("0", "2"):
        out = tmp_path / f"out{mode}.bin"
        r = subprocess.run([exe, str(tmp_path / "scans.bin"), str(out), str(P), str(ITERS), str(KNN), str(VOXEL), str(tmp_path / "particles.bin"),
                            mode, "1"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        raw_b = open(out, "rb").read()
        off = 0
        for k in range(len(frames)):
            off += 4
            pose = np.frombuffer(raw_b, "<f8", 12, off); off += 96 + 96 + 48 + 48 + 288
            B, M = np.frombuffer(raw_b, "<i8", 2, off); off += 16 + 24 * (int(B) + int(M)) + 48 * P
            T = np.eye(4); T[:3, :3] = pose[:9].reshape(3, 3); T[:3, 3] = pose[9:]
            assert np.allclose(T, host[k], rtol=0, atol=1e-9), (mode, k)
        assert off == len(raw_b)
    er_d, et_d = _errors(pl, truth, host)
    er_r, et_r = _errors(pl, truth, raw)
    print("rotation error per frame, deskew:", np.round(er_d, 5), " skewed:", np.round(er_r, 5))
    print("translation error per frame, deskew:", np.round(et_d, 4), " skewed:", np.round(et_r, 4))
    # measured (profiles/deskew_drive.log): final rotation error 0.00268 rad with deskew, 0.01012 without (ratio 0.26).  The
    # forward translation is tracked by neither run — both lose ~1 m of the 5.5 m travelled along the corridor, the same way
    # with and without deskew, while the twist ramps up (the point-to-point solver barely observes sliding along the walls,
    # test_pipeline_gpu.py) — so translation is held in the pure-yaw drive below.
    assert er_d[-1] < 0.5 * er_r[-1]


def test_deskew_reduces_the_error_of_a_turning_drive(hip, pl):
    """The sensor turns on the spot at up to 3 deg per sweep: every quantity is observed, and the skew (up to 1.5 deg at the
    ends of a sweep, 0.8 m at 30 m) is the only difference between the runs.  Measured (profiles/deskew_drive.log): final
    translation error 0.0058 m with deskew, 0.026 m without (ratio 0.22); rotation 0.0019 rad, 0.0114 (ratio 0.17)."""
    frames, truth, parts = _drive(hip, delta=np.array([0.0, 0.0, np.radians(3.0), 0.0, 0.0, 0.0]), ramp=4)
    er_d, et_d = _errors(pl, truth, _run(hip, pl, frames, parts, deskew=True))
    er_r, et_r = _errors(pl, truth, _run(hip, pl, frames, parts))
    print("rotation error per frame, deskew:", np.round(er_d, 5), " skewed:", np.round(er_r, 5))
    print("translation error per frame, deskew:", np.round(et_d, 4), " skewed:", np.round(et_r, 4))
    assert et_d[-1] < 0.5 * et_r[-1]
    assert er_d[-1] < 0.5 * er_r[-1]
