"""Visibility-based clearing of the voxel map, host restatement (pipeline.VoxelHashMap.clear_seen_through):
the rule on hand-placed points with expectations written out by hand, the map bookkeeping, the moving-box drive, and the C++
restatement of registration_pipeline.hpp (tests/map_visibility_driver.cpp) bit for bit against the Python one.

The drive's bounds are caps, not measurements (the prototype of the rule measured 100 % of the ghost points removed and no
static point): at least 95 % of the ghost points go, at most 0.1 % of the static ones, with and without the box — and the
same drive with a single-pixel window must remove MORE than 1 % of the static points, which pins that the window matters."""
import functools

import numpy as np
import pytest

import __graft_entry__ as ge
import map_visibility_cases as mv

pkg = ge.load_package()
pl = pkg.pipeline
sc = pkg.scans

CASES = mv.crafted_cases()


def _host_map(points, pose, max_points=20):
    m = pl.VoxelHashMap(1.0, 100.0, max_points)
    m.add_pointcloud(mv.to_map_frame(points, pose), np.eye(4))
    return m


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_crafted_case(case):
    sensor = mv.tiny_sensor(pl)
    stored = mv.to_map_frame(case.points, case.pose)
    img = pl.visibility_image(case.scan, sensor)
    tested, removed = pl.visibility_test(stored, case.pose, img, sensor, case.window[0], case.window[1], case.margin[0], case.margin[1],
                                         case.max_range)
    assert removed.tolist() == case.removed
    assert int(tested.sum()) == case.tested
    m = _host_map(case.points, case.pose)
    st = m.clear_seen_through(case.scan, case.pose, sensor, window=case.window, margin=case.margin, max_range=case.max_range)
    keep = ~np.array(case.removed)
    assert st == {"pixels_filled": case.filled, "points_tested": case.tested, "points_removed": sum(case.removed),
                  "voxels_emptied": mv.voxels_emptied(stored, keep)}
    assert np.array_equal(mv.sorted_rows(m.get_map()), mv.sorted_rows(stored[keep]))


def test_image_keeps_the_minimum_and_marks_empty_pixels():
    sensor = mv.tiny_sensor(pl)
    img = pl.visibility_image(np.stack([mv.beam(5, 20, 20), mv.beam(5, 20, 10.5), mv.beam(5, 20, 30), mv.beam(0, 0, 7)]), sensor)
    assert img.shape == (8, 90) and img.dtype == np.float32
    assert abs(float(img[5, 20]) - 10.5) < 1e-5 and abs(float(img[0, 0]) - 7.0) < 1e-5
    assert np.count_nonzero(np.isinf(img)) == 8 * 90 - 2


def test_options_refused():
    sensor = mv.tiny_sensor(pl)
    m = _host_map(np.array([[10, 0, 0]], np.float32), np.eye(4))
    scan = np.array([[20, 0, 0]], np.float32)
    for kw in (dict(window=(5, 0)), dict(window=(0, 9)), dict(window=(-1, 0)), dict(margin=(-0.1, 0.0)), dict(margin=(0.1, float("nan"))),
               dict(margin=(float("inf"), 0.0)), dict(max_range=0.0), dict(max_range=float("inf")), dict(max_range=-3.0)):
        with pytest.raises(ValueError):
            m.clear_seen_through(scan, np.eye(4), sensor, **kw)
    with pytest.raises(ValueError):
        m.clear_seen_through(scan, np.eye(4), pl.SegParams(n_scan=129))
    with pytest.raises(ValueError):
        m.clear_seen_through(scan, np.eye(4), pl.SegParams(ang_res_y=0.0))
    assert len(m) == 1 and m.get_map().shape[0] == 1          # nothing was touched
    with pytest.raises(ValueError):
        pl.PipelineConfig(clear_seen_through=(1, 1, 0.3))
    with pytest.raises(ValueError):
        pl.PipelineConfig(clear_seen_through=(1, 9, 0.3, 0.02))
    with pytest.raises(ValueError):
        pl.PipelineConfig(clear_seen_through=(1, 1, 0.3, 0.02), clear_max_range=-1.0)
    assert pl.PipelineConfig().clear_seen_through is None


def test_empty_scan_and_empty_map_are_no_ops():
    sensor = mv.tiny_sensor(pl)
    zero = dict.fromkeys(pl.VISIBILITY_STATS, 0)
    m = _host_map(np.array([[10, 0, 0]], np.float32), np.eye(4))
    assert m.clear_seen_through(np.zeros((0, 3), np.float32), np.eye(4), sensor) == zero
    assert pl.VoxelHashMap(1.0, 100.0, 20).clear_seen_through(np.array([[20, 0, 0]], np.float32), np.eye(4), sensor) == zero
    assert len(m) == 1


# ------------------------------------------------------------------------------------------------ map bookkeeping
def test_removing_the_first_point_changes_what_get_map_and_remove_far_see():
    sensor = mv.tiny_sensor(pl)
    # one voxel (10, 0, 0) with first point A = (10.1, 0, 0) and second B = (10.9, 0.9, 0): B sits in another pixel column
    A, B = [10.1, 0.0, 0.0], [10.9, 0.9, 0.0]
    m = pl.VoxelHashMap(1.0, 10.5, 20)
    m.add_pointcloud(np.array([A, B], np.float32), np.eye(4))
    assert len(m) == 1
    centre = np.eye(4)
    assert m.get_map(centre, 10.5).shape[0] == 2               # selected through A: |A| = 10.1 < 10.5
    st = m.clear_seen_through(np.array([[20, 0, 0]], np.float32), np.eye(4), sensor, window=(0, 0))
    assert st["points_removed"] == 1 and st["voxels_emptied"] == 0
    assert np.array_equal(m.get_map(), np.array([B], np.float32).astype(np.float64))
    assert m.get_map(centre, 10.5).shape[0] == 0               # the first point is B now: |B| = 10.94 > 10.5
    m.remove_far(np.zeros(3))                                  # ... and the range cull (max_range 10.5) reads B too
    assert len(m) == 0


def test_emptied_voxel_disappears_and_freed_room_is_refilled_in_input_order():
    sensor = mv.tiny_sensor(pl)
    m = pl.VoxelHashMap(1.0, 100.0, 3)
    full = np.array([[10.1, 0, 0], [10.5, 0, 0], [10.9, 0, 0], [10.3, 0, 0]], np.float32)   # the fourth finds no room
    other = np.array([[0, 12.5, 0]], np.float32)                                           # another voxel, another pixel
    m.add_pointcloud(np.concatenate([full, other]), np.eye(4))
    assert len(m) == 2 and m.get_map().shape[0] == 4
    # a return at 10.7, margin 0.3: 10.1 is seen through (10.1 < 10.4), 10.5 and 10.9 are not
    st = m.clear_seen_through(np.array([[10.7, 0, 0]], np.float32), np.eye(4), sensor, window=(0, 0), margin=(0.3, 0.0))
    assert (st["points_removed"], st["voxels_emptied"]) == (1, 0)
    m.add_pointcloud(np.array([[10.2, 0, 0], [10.4, 0, 0]], np.float32), np.eye(4))          # room for one: the first of the two
    vox = mv.sorted_rows(m.get_map())
    assert np.array_equal(vox, mv.sorted_rows(np.array([[10.5, 0, 0], [10.9, 0, 0], [10.2, 0, 0], [0, 12.5, 0]], np.float32)))
    assert [float(v[0]) for v in m._vox[(10, 0, 0)]] == [float(np.float32(x)) for x in (10.5, 10.9, 10.2)]   # order: survivors, then the new point
    st = m.clear_seen_through(np.array([[30, 0, 0]], np.float32), np.eye(4), sensor, window=(0, 0))
    assert (st["points_removed"], st["voxels_emptied"]) == (3, 1)
    assert len(m) == 1 and np.array_equal(m.get_map(), other.astype(np.float64))


# ------------------------------------------------------------------------------------------------ the drive
@functools.lru_cache(maxsize=None)
def _scans(with_box):
    return mv.drive_scans(sc, pl.SEG_PRESETS["OS1-64"], 8, with_box)


def _drive(with_box, window):
    """The drive of DESIGN.md §4.15's table: the host map is fed the 0.5 m uniform sampling, the rule the cropped cloud, before
    each insert -> (static removed, static stored over the drive, ghost removed, ghost left)."""
    sensor = pl.SEG_PRESETS["OS1-64"]
    m = pl.VoxelHashMap(1.0, 100.0, 20)
    static_removed = ghost_removed = 0
    for i, (T, scan) in enumerate(_scans(with_box)):
        cropped, _ = pl.crop_pointcloud(scan, 1.0, 100.0)
        if i > 0:
            before = m.get_map()
            m.clear_seen_through(cropped, T, sensor, window=window, margin=(0.3, 0.02))
            after = m.get_map()
            gone = _rows_missing(before, after)
            ghost = mv.in_boxes(gone, range(i)) if with_box else np.zeros(gone.shape[0], bool)
            ghost_removed += int(ghost.sum())
            static_removed += int((~ghost).sum())
        m.add_pointcloud(pl.downsample_uniform(cropped, 0.5), T)
    final = m.get_map()
    n = len(_scans(with_box))
    past = mv.in_boxes(final, range(n)) if with_box else np.zeros(final.shape[0], bool)
    ghost_left = int((past & ~mv.in_boxes(final, [n - 1])).sum()) if with_box else 0
    static_total = int((~past).sum()) + static_removed
    return static_removed, static_total, ghost_removed, ghost_left


def _rows_missing(before, after):
    """Rows of ``before`` that are not in ``after`` (multiset difference)."""
    key = lambda a: np.ascontiguousarray(a).view([("", a.dtype)] * 3).reshape(-1)
    kb, ka = key(before), key(after)
    ub, cb = np.unique(kb, return_counts=True)
    ua, ca = np.unique(ka, return_counts=True)
    left = dict(zip(ua.tolist(), ca.tolist()))
    out = []
    for k, c in zip(ub.tolist(), cb.tolist()):
        out += [k] * (c - left.get(k, 0))
    return np.array(out, np.float64).reshape(-1, 3)


def test_drive_with_moving_box_removes_the_ghosts_and_keeps_the_scene():
    static_removed, static_total, ghost_removed, ghost_left = _drive(True, (1, 1))
    print(f"window (1,1), box: static removed {static_removed} of {static_total}, ghost removed {ghost_removed}, left {ghost_left}")
    assert ghost_removed + ghost_left > 100                    # the box did leave a trail to clear
    assert ghost_removed >= 0.95 * (ghost_removed + ghost_left)
    assert static_removed <= 0.001 * static_total


def test_drive_without_box_keeps_the_scene():
    static_removed, static_total, _, _ = _drive(False, (1, 1))
    print(f"window (1,1), no box: static removed {static_removed} of {static_total}")
    assert static_removed <= 0.001 * static_total


def test_drive_with_single_pixel_window_eats_the_scene():
    static_removed, static_total, _, _ = _drive(True, (0, 0))
    print(f"window (0,0), box: static removed {static_removed} of {static_total}")
    assert static_removed > 0.01 * static_total


# ------------------------------------------------------------------------------------------------ the C++ restatement
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path_factory.mktemp("vis") / "map_visibility_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(root, "include"), "-I",
                           os.path.join(root, "svn-icp_amd", "host"), os.path.join(root, "tests", "map_visibility_driver.cpp"), "-o", out])
    return out


def _cpp(driver, tmp_path, sensor, window, margin, max_range, pose, stored, scan, voxel=1.0, map_range=100.0, max_points=20):
    """-> (statistics, voxels, float32 rows) of registration_pipeline.hpp's VoxelHashMap after ClearSeenThrough."""
    import ctypes as C
    import struct
    import subprocess
    bd = pkg.binding
    opt = bd.VisibilityOptStruct(C.sizeof(bd.VisibilityOptStruct), window[0], window[1], margin[0], margin[1], max_range)
    T = np.asarray(pose, float)
    stored, scan = np.ascontiguousarray(stored, np.float32), np.ascontiguousarray(scan, np.float32)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(bytes(pl.seg_params_struct(sensor))); f.write(bytes(opt))
        f.write(struct.pack("<ddi", voxel, map_range, max_points))
        f.write(np.ascontiguousarray(T[:3, :3]).tobytes()); f.write(np.ascontiguousarray(T[:3, 3]).tobytes())
        f.write(struct.pack("<i", stored.shape[0])); f.write(stored.tobytes())
        f.write(struct.pack("<i", scan.shape[0])); f.write(scan.tobytes())
    r = subprocess.run([driver, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    head = np.frombuffer(raw, np.int64, 6)
    rows = np.frombuffer(raw, np.float32, 3 * int(head[5]), 48).reshape(-1, 3)
    return dict(zip(pl.VISIBILITY_STATS, head[:4].tolist())), int(head[4]), rows


def _python_rows(m):
    """The host map in ascending voxel index, as std::map iterates."""
    rows = [np.asarray(v, np.float32) for _, v in sorted(m._vox.items())]
    return np.concatenate(rows, 0) if rows else np.zeros((0, 3), np.float32)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cpp_restatement_on_the_crafted_cases(driver, tmp_path, case):
    sensor = mv.tiny_sensor(pl)
    stored = mv.to_map_frame(case.points, case.pose)
    m = _host_map(case.points, case.pose)
    want = m.clear_seen_through(case.scan, case.pose, sensor, window=case.window, margin=case.margin, max_range=case.max_range)
    got, voxels, rows = _cpp(driver, tmp_path, sensor, case.window, case.margin, case.max_range, case.pose, stored, case.scan)
    assert got == want and voxels == len(m)
    assert np.array_equal(rows, _python_rows(m))


def test_cpp_restatement_on_a_drive_step(driver, tmp_path):
    """One OS1-64 step of the drive with each window, under a pose that also turns: map and statistics bit for bit."""
    sensor = pl.SEG_PRESETS["OS1-64"]
    (T0, s0), (T1, s1) = _scans(True)[:2]
    stored = pl.transform_f32(pl.downsample_uniform(pl.crop_pointcloud(s0, 1.0, 100.0)[0], 0.5), T0)
    yaw = np.eye(4); yaw[:3, :3] = sc.rot_zyx(0.01, -0.02, 0.3)
    for window, pose, scan in (((1, 1), T1, s1), ((0, 0), T1, s1), ((2, 3), T1 @ yaw, s1)):
        m = pl.VoxelHashMap(1.0, 100.0, 20)
        m.add_pointcloud(stored, np.eye(4))
        want = m.clear_seen_through(scan, pose, sensor, window=window, margin=(0.3, 0.02))
        got, voxels, rows = _cpp(driver, tmp_path, sensor, window, (0.3, 0.02), 100.0, pose, stored, scan)
        assert want["points_tested"] > 10000 and want["points_removed"] > 0
        assert got == want and voxels == len(m)
        assert np.array_equal(rows, _python_rows(m))
