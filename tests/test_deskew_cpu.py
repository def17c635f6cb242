"""Motion compensation (deskew) ahead of the crop: the host restatements of OdometryPipeline::deskew_pointcloud
(OdometryPipeline.cpp:357-447) in svn-icp_amd/pipeline.py and svn-icp_amd/host/registration_pipeline.hpp, and the moving-sensor
scan generator scans.lidar_sweep.  Parity unpinned (GTSAM / Eigen / PCL absent): the tests check the cited rules, the
convention against a sweep whose geometry is known exactly, and the two restatements against each other."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest


@pytest.fixture(scope="module")
def pl(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".pipeline")


DELTA = np.array([0.004, -0.006, 0.05, 0.8, 0.1, -0.03])   # [omega, v] over one sweep: ~3 deg of yaw, 0.8 m forward


def _sweep(pkg, n=8192, delta=DELTA, noise=0.0, stream=41):
    sc = pkg.scans
    T_mid = np.eye(4)
    T_mid[:3, :3] = sc.rot_zyx(0.01, -0.02, 0.3)
    T_mid[:3, 3] = [1.5, -0.7, 0.2]
    return T_mid, sc.lidar_sweep(sc.make_scene(), T_mid, delta, n, stream=stream, noise=noise)


def _ulp_err(a, b):
    """max |a - b| in float32 ulps of the larger magnitude, per coordinate"""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    u = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / u


# ----------------------------------------------------------------------------- identity cases
def test_zero_motion_midpoint_and_constant_stamps_leave_points_unchanged(pl, pkg):
    _, sw = _sweep(pkg, 2048, noise=0.02)
    pts = sw.points.astype(np.float32)
    out = pl.deskew_pointcloud(pts, sw.stamps, np.zeros(6))
    assert out.dtype == np.float32 and np.array_equal(out, pts)                          # delta = 0: bit for bit
    # a point whose normalised stamp is exactly 0.5 is not moved, whatever the motion
    st = np.linspace(0.0, 1.0, pts.shape[0])
    st[100] = 0.5
    out = pl.deskew_pointcloud(pts, st, DELTA)
    assert np.array_equal(out[100], pts[100]) and not np.array_equal(out[0], pts[0])
    # min == max: *frame (:418) — the raw points, in KITTI mode WITHOUT the vertical correction
    assert np.array_equal(pl.deskew_pointcloud(pts, np.full(pts.shape[0], 7.0), DELTA), pts)
    assert np.array_equal(pl.deskew_pointcloud(pts, np.full(pts.shape[0], 9, np.uint32), DELTA), pts)
    assert np.array_equal(pl.deskew_pointcloud(pts, None, DELTA), pts)                    # no stamp field: zeros, raw frame
    same = np.tile(np.array([[10.0, 10.0, 1.0]], np.float32), (50, 1))                   # one yaw -> one KITTI stamp
    assert np.array_equal(pl.deskew_pointcloud(same, None, DELTA, kitti=True), same)


def test_stamp_types_widen_to_double_and_nonfinite_stamps_give_nan(pl, pkg):
    _, sw = _sweep(pkg, 4096)
    pts = sw.points.astype(np.float32)
    # the same instants as float64 seconds, float32 seconds and uint32 nanoseconds give the same normalised times up to the
    # rounding of the type
    a = pl.deskew_pointcloud(pts, sw.stamps, DELTA)
    b = pl.deskew_pointcloud(pts, sw.stamps_ns, DELTA)
    c = pl.deskew_pointcloud(pts, sw.stamps.astype(np.float32), DELTA)
    assert np.abs(a - b).max() < 1e-4 and np.abs(a - c).max() < 1e-3
    with pytest.raises(ValueError):
        pl.deskew_pointcloud(pts, sw.stamps.astype(np.int64), DELTA)
    # deliberate deviation: non-finite stamps are left out of min / max, their points come out NaN and the crop drops them
    st = sw.stamps.copy()
    st[[3, 50]] = [np.nan, np.inf]
    out = pl.deskew_pointcloud(pts, st, DELTA)
    assert np.isnan(out[[3, 50]]).all() and np.isfinite(np.delete(out, [3, 50], 0)).all()
    assert np.array_equal(np.delete(out, [3, 50], 0), np.delete(a, [3, 50], 0))   # min / max untouched by the bad stamps
    kept, _ = pl.crop_pointcloud(out, 1.0, 100.0)
    assert np.isfinite(kept).all()


def test_vectorised_exp_matches_se3_exp(pl):
    rng = np.random.default_rng(3)
    xi = rng.normal(size=(200, 6)) * np.array([0.05, 0.05, 0.05, 1.0, 1.0, 1.0])
    xi[0] = 0.0
    xi[1, :3] = 1e-12
    R, t = pl._se3_exp_rows(xi)
    for k in range(xi.shape[0]):
        T = pl.se3_exp(xi[k])
        assert np.allclose(np.array([r[k] for r in R]).reshape(3, 3), T[:3, :3], rtol=0, atol=1e-15)
        assert np.allclose([v[k] for v in t], T[:3, 3], rtol=0, atol=1e-15)


# ----------------------------------------------------------------------------- convention
def test_deskew_maps_a_moving_sweep_to_the_mid_sweep_frame(pl, pkg):
    """lidar_sweep with noise 0: every point was fired from T(s) = T_mid · Exp((s − 0.5)·δ).  The stamps span
    [s_first, s_last] = (cols − 1)/cols of the period and the reference normalises by that span (:419-423), so the motion
    handed to the deskew is the motion over the span: δ·(cols − 1)/cols.  Then every deskewed point is T_mid⁻¹ · world hit
    up to float32 rounding; with −δ the error is of the order of the motion (pins the sign of s − 0.5 and the order of
    composition)."""
    n = 8192
    cols = n // 64
    T_mid, sw = _sweep(pkg, n)
    d_span = DELTA * (cols - 1) / cols
    want = (sw.world - T_mid[:3, 3]) @ T_mid[:3, :3]
    got = pl.deskew_pointcloud(sw.points, sw.stamps, d_span).astype(np.float64)
    err = np.linalg.norm(got - want, axis=1)
    norm = np.linalg.norm(want, axis=1)
    raw = np.linalg.norm(sw.points - want, axis=1)
    print(f"deskew residual max {err.max():.2e} m (|p| up to {norm.max():.1f} m), raw skew max {raw.max():.2f} m")
    assert np.all(err <= 8 * 2.0 ** -24 * norm + 1e-9)          # two float32 roundings (the sweep's points and the output)
    assert raw.max() > 0.5                                      # the sweep is really skewed
    bad = np.linalg.norm(pl.deskew_pointcloud(sw.points, sw.stamps, -d_span).astype(np.float64) - want, axis=1)
    assert bad.max() > 0.5 * 2 * raw.max() and np.median(bad) > 10 * np.median(err) + 1e-3
    # the uint32-nanosecond variant of the same stamps gives the same picture
    got_ns = pl.deskew_pointcloud(sw.points, sw.stamps_ns, d_span).astype(np.float64)
    assert np.linalg.norm(got_ns - want, axis=1).max() < 1e-4


# ----------------------------------------------------------------------------- KITTI
def test_kitti_correction_and_stamps(pl, pkg):
    _, sw = _sweep(pkg, 4096, noise=0.02)
    pts = np.concatenate([sw.points, [[0.0, 0.0, 5.0], [0.0, 0.0, -3.0], [0.0, 0.0, 0.0]]]).astype(np.float32)
    corr, st = pl.kitti_correct_and_stamp(pts)
    assert corr.dtype == np.float32 and st.dtype == np.float64
    assert st.min() >= 0.0 and st.max() <= 1.0
    a = math.radians(0.205)
    p = pts[:-3].astype(np.float64)
    q = corr[:-3].astype(np.float64)
    # each off-axis point is turned by 0.205 deg about (y, -x, 0)/|.|: the norm is kept, the angle between p and q is 0.205 deg,
    # and q - p is perpendicular to the axis
    npn, nq = np.linalg.norm(p, axis=1), np.linalg.norm(q, axis=1)
    assert np.all(np.abs(nq - npn) <= 4 * 2.0 ** -24 * npn)
    cosang = np.sum(p * q, axis=1) / (npn * nq)
    ang = np.arccos(np.clip(cosang, -1, 1))
    horiz = np.hypot(p[:, 0], p[:, 1]) > 1.0
    assert np.allclose(ang[horiz], a, rtol=0, atol=5e-6)
    axis = np.stack([p[:, 1], -p[:, 0], np.zeros(len(p))], 1)
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    assert np.abs(np.sum((q - p) * axis, axis=1)).max() < 1e-5
    # a point on the z axis has a zero axis: Eigen's normalized() keeps it zero, AngleAxis(angle, 0) is the identity
    # (cos·I + (1−cos)·0 + sin·0 = cos·I): the point is scaled by cos(0.205°)
    assert np.allclose(corr[-3:], pts[-3:] * np.float32(math.cos(a)), rtol=0, atol=1e-6)
    # stamp = 0.5·(yaw/π + 1), yaw = −atan2(y, x) of the float32 corrected point, as a float
    yaw = (-np.arctan2(corr[:, 1].astype(np.float64), corr[:, 0].astype(np.float64))).astype(np.float32)
    assert np.array_equal(st, 0.5 * (yaw.astype(np.float64) / np.pi + 1.0))
    # deskew in KITTI mode: the stamps of the corrected points, applied to the corrected points
    out = pl.deskew_pointcloud(pts, None, DELTA, kitti=True)
    assert np.array_equal(out, pl.deskew_pointcloud(corr, st, DELTA))


# ----------------------------------------------------------------------------- C++ restatement vs numpy
def _build_driver(root, out):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-I",
                           os.path.join(root, "svn-icp_amd", "host"), os.path.join(root, "tests", "deskew_driver.cpp"), "-o", out])
    return out


@pytest.mark.parametrize("case", ["stamps", "kitti", "nan", "const", "none"])
def test_cpp_restatement_matches_numpy(pl, pkg, tmp_path, case):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = _build_driver(root, str(tmp_path / "deskew_driver"))
    _, sw = _sweep(pkg, 16384, noise=0.02, stream=77)
    pts = np.concatenate([sw.points, [[0.0, 0.0, 4.0]]]).astype(np.float32)
    st = np.append(sw.stamps, 0.05)
    if case == "nan":
        st[[5, 9]] = [np.nan, -np.inf]
    if case == "const":
        st[:] = 3.0
    kitti = case == "kitti"
    has = case not in ("kitti", "none")
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<iii", pts.shape[0], int(has), int(kitti)))
        f.write(DELTA.astype("<f8").tobytes()); f.write(pts.astype("<f4").tobytes())
        if has:
            f.write(st.astype("<f8").tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    n = pts.shape[0]
    cpp = raw[:12 * n].view("<f4").reshape(n, 3)
    py = pl.deskew_pointcloud(pts, st if has else None, DELTA, kitti=kitti)
    nan_c, nan_p = np.isnan(cpp), np.isnan(py)
    assert np.array_equal(nan_c, nan_p)
    e = _ulp_err(cpp[~nan_c], py[~nan_p])
    print(f"{case}: {int((e > 0).sum())} of {e.size} coordinates differ, max {e.max() if e.size else 0:.0f} ulp")
    assert e.size == 0 or e.max() <= 1.0
    if case in ("const", "none"):
        assert np.array_equal(cpp, pts)
    if kitti:
        corr = raw[12 * n:24 * n].view("<f4").reshape(n, 3)
        kst = raw[24 * n:].view("<f8")
        c_py, s_py = pl.kitti_correct_and_stamp(pts)
        assert _ulp_err(corr, c_py).max() <= 1.0
        assert np.abs(kst - s_py).max() <= 1e-7


# ----------------------------------------------------------------------------- the pipeline switch (host path, no solver)
def test_pipeline_config_defaults_keep_deskew_off(pl):
    cfg = pl.PipelineConfig()
    assert cfg.deskew is False and cfg.kitti is False


def test_lidar_sweep_without_motion_is_lidar_scan(pkg):
    sc = pkg.scans
    scene = sc.make_scene()
    T = np.eye(4)
    T[:3, :3] = sc.rot_zyx(0.0, 0.0, 0.2)
    T[:3, 3] = [0.5, 0.3, 0.0]
    sw = sc.lidar_sweep(scene, T, np.zeros(6), 4096, stream=5)
    ref = sc.lidar_scan(scene, T[:3, :3], T[:3, 3], 4096, stream=5)
    assert np.abs(sw.points - ref).max() < 1e-5
    assert sw.stamps.shape == (4096,) and sw.stamps_ns.dtype == np.uint32
    cols = 4096 // 64
    assert sw.s[0] == 0.5 / cols and sw.s[-1] == (cols - 0.5) / cols and np.all(np.diff(sw.s) >= 0)
