"""Range-image segmentation (LeGO-LOAM ImageProjection::cloudHandler, include/segmentation/ImageProjection.h) on the host:
pipeline.py's segment_images / segment_scan on hand-built images with labels written out by hand, its BFS against scipy's
connected components, the sensor presets, the C++ restatement in registration_pipeline.hpp bit for bit against the Python one,
and the C ABI pieces that need no device."""
import ctypes as C
import math
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def pl(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".pipeline")


@pytest.fixture(scope="module")
def small(pl):
    """8 x 16 image: 22.5 degree columns, 2 degree rows from -8 degrees, ground rows 0..3"""
    return pl.SegParams(n_scan=8, horizon_scan=16, ground_scan_ind=3, ang_res_x=22.5, ang_res_y=2.0, ang_bottom=8.0)


def _at(pl, prm, row, col, r, frac=0.5):
    """a float32 point of range r whose projection is pixel (row, col); frac places it inside the row"""
    el = math.radians(-prm.ang_bottom + (row + frac) * prm.ang_res_y)
    h = math.radians(90.0 - (col - prm.horizon_scan // 2) * prm.ang_res_x)
    p = np.array([[r * math.cos(el) * math.sin(h), r * math.cos(el) * math.cos(h), r * math.sin(el)]], F)
    owner, _ = pl._seg_project(p, prm)
    assert owner[row * prm.horizon_scan + col] == 0, (row, col)
    return p[0]


def _ground_pt(pl, prm, row, col, height=1.0):
    """a point of the plane z = -height in pixel (row, col) (row centre below the horizon)"""
    el = -prm.ang_bottom + (row + 0.5) * prm.ang_res_y
    return _at(pl, prm, row, col, height / math.sin(math.radians(-el)))


def _images(pl, prm, pts):
    owner, rng, ground, label = pl.segment_images(np.array(pts, F), prm)
    return owner, ground, label


# ----------------------------------------------------------------------------- hand-built images
def test_component_joined_across_the_column_wrap(pl, small):
    pix = [(r, c) for r in (4, 5, 6) for c in (15, 0, 1)]
    _, ground, label = _images(pl, small, [_at(pl, small, r, c, 10.0) for r, c in pix])
    for r, c in pix:
        assert label[r, c] == 1                                   # one component; seed (4, 0), 9 pixels on 3 rows
    assert (label == 0).sum() == 0 and label.max() == 1


def test_four_pixel_component_is_invalid(pl, small):
    pix = [(4, 3), (4, 4), (5, 3), (5, 4)]
    _, _, label = _images(pl, small, [_at(pl, small, r, c, 10.0) for r, c in pix])
    assert all(label[r, c] == 999999 for r, c in pix)
    xyz, idx = pl.segment_scan(np.array([_at(pl, small, r, c, 10.0) for r, c in pix]), small)
    assert xyz.shape == (0, 3) and idx.size == 0


def test_seed_alone_in_its_row_does_not_count_as_a_line(pl, small):
    pix = [(4, 5), (5, 5), (5, 6), (6, 6), (6, 7)]               # 5 pixels on 3 rows; the seed (4, 5) is alone in row 4
    _, _, label = _images(pl, small, [_at(pl, small, r, c, 10.0) for r, c in pix])
    assert all(label[r, c] == 999999 for r, c in pix)             # lineCountFlag: rows 5 and 6 only


def test_seed_row_shared_makes_the_component_valid(pl, small):
    pix = [(4, 5), (4, 6), (5, 6), (6, 6), (6, 7)]               # (4, 6) is pushed and flags row 4
    pts = [_at(pl, small, r, c, 10.0) for r, c in pix]
    _, _, label = _images(pl, small, pts)
    assert all(label[r, c] == 1 for r, c in pix)
    xyz, idx = pl.segment_scan(np.array(pts, F), small)
    assert idx.tolist() == [0, 1, 2, 3, 4]                        # row-major order of the pixels


def test_single_row_components_of_30_and_29_pixels(pl, small):
    prm = replace(small, horizon_scan=64, ang_res_x=360.0 / 64)
    pts = [_at(pl, prm, 5, c, 10.0) for c in range(30)] + [_at(pl, prm, 7, c, 10.0) for c in range(29)]
    _, _, label = _images(pl, prm, pts)
    assert (label[5, :30] == 1).all()                             # >= 30 pixels: valid on one row
    assert (label[7, :29] == 999999).all()


def test_ground_overwrite_leaves_a_pixel_to_the_segmentation(pl, small):
    j = 10
    pts = [_ground_pt(pl, small, 0, j), _ground_pt(pl, small, 1, j)]   # flat pair (0, 1); pixel (2, j) empty
    _, ground, label = _images(pl, small, pts)
    assert ground[0, j] == 1 and ground[1, j] == -1               # pair (1, 2) invalid overwrites the 1 of pair (0, 1)
    assert label[0, j] == -1
    assert label[1, j] == 999999                                  # segmented like any other point (a singleton)
    _, idx = pl.segment_scan(np.array(pts, F), small)
    assert idx.tolist() == [0]                                    # ground pixel at j % 5 == 0 is kept


def test_ground_decimation(pl, small):
    pts = [_ground_pt(pl, small, r, j) for r in range(4) for j in range(16)]
    _, ground, label = _images(pl, small, pts)
    assert (ground[:4] == 1).all() and (label[:4] == -1).all()
    _, idx = pl.segment_scan(np.array(pts, F), small)
    kept = sorted({int(i) % 16 for i in idx})
    assert kept == [0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14, 15]     # j <= 5, j % 5 == 0, j >= H - 5
    assert idx.size == 4 * 12


def test_last_point_in_a_pixel_wins(pl, small):
    a, b = _at(pl, small, 5, 3, 10.0, 0.3), _at(pl, small, 5, 3, 12.5, 0.7)
    owner, rng, _, _ = pl.segment_images(np.array([a, b], F), small)
    assert owner[5, 3] == 1 and rng[5, 3] == np.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
    owner, rng, _, _ = pl.segment_images(np.array([b, a], F), small)
    assert owner[5, 3] == 1 and rng[5, 3] == np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    assert (owner >= 0).sum() == 1 and rng[0, 0] == F(-100000.0)


def test_row_conversion_of_negative_q(pl, small):
    def pt(va, along_x):
        el = math.radians(va)
        d = 10 * math.cos(el)
        return np.array([d if along_x else 0.0, 0.0 if along_x else d, 10 * math.sin(el)], F)
    owner, _, _, _ = pl.segment_images(np.array([pt(-9.0, True), pt(-10.5, True), pt(-7.5, False)], F), small)
    assert (owner >= 0).sum() == 2                                # q = -1.25 is dropped
    assert owner[0, 8] == 0                                       # q = -0.5: size_t 0, row 0 (column 8: along +x)
    assert owner[0, 12] == 2                                      # q = 0.25: row 0 (column 12: along +y)


def test_points_inside_the_minimum_range_are_dropped(pl, small):
    near = _at(pl, small, 5, 2, 10.0) * F(0.05)                  # range 0.5 < sensorMinimumRange
    owner, _, _, _ = pl.segment_images(np.array([near, _at(pl, small, 5, 4, 1.5)], F), small)
    assert (owner >= 0).sum() == 1 and owner[5, 4] == 1


def test_non_finite_points_are_dropped_and_indices_kept(pl, small):
    pix = [(4, 5), (4, 6), (5, 6), (6, 6), (6, 7)]
    good = [_at(pl, small, r, c, 10.0) for r, c in pix]
    pts = [[np.nan, 1, 1]] + good[:2] + [[1, np.inf, 1], [1, 1, -np.inf]] + good[2:]
    xyz, idx = pl.segment_scan(np.array(pts, F), small)
    assert idx.tolist() == [1, 2, 5, 6, 7]
    assert np.array_equal(xyz, np.array(good, F))


# ----------------------------------------------------------------------------- the BFS against scipy
def test_bfs_partition_equals_connected_components(pl, pkg):
    from scipy import sparse
    from scipy.sparse.csgraph import connected_components
    prm = pl.SEG_PRESETS["HDL-64E"]
    sc = pkg.scans
    pts = sc.lidar_grid_scan(sc.make_scene(), sc.rot_zyx(0, 0, 0.3), np.array([1.0, -2.0, 0.0]), prm, 17)
    owner, rng, ground, label = pl.segment_images(pts, prm)
    N, H = label.shape
    init0 = ((ground != 1) & (owner >= 0)).reshape(-1)
    sx, cx, sy, cy = prm.alphas()

    def link(a, b, s, c):
        d1, d2 = np.maximum(a, b), np.minimum(a, b)
        return pl._atan2_f32(d2 * s, d1 - d2 * c) > F(prm.segment_theta)

    p = np.arange(N * H).reshape(N, H)
    r = rng
    right = link(r, np.roll(r, -1, 1), sx, cx) & init0.reshape(N, H) & np.roll(init0.reshape(N, H), -1, 1)
    down = link(r[:-1], r[1:], sy, cy) & init0.reshape(N, H)[:-1] & init0.reshape(N, H)[1:]
    a = np.concatenate([p[right], p[:-1][down]])
    b = np.concatenate([np.roll(p, -1, 1)[right], p[1:][down]])
    g = sparse.coo_matrix((np.ones(a.size), (a, b)), shape=(N * H, N * H))
    _, comp = connected_components(g, directed=False)
    lab = label.reshape(-1)
    assert (lab[init0] != 0).all() and (lab[~init0] == -1).all()
    comp = comp[init0]
    idx = np.flatnonzero(init0)
    # the same partition: every component of scipy maps to one BFS label and vice versa (valid labels are unique per component)
    valid = lab[init0] != 999999
    pairs = set(zip(comp[valid].tolist(), lab[init0][valid].tolist()))
    assert len(pairs) == len({c for c, _ in pairs}) == len({l for _, l in pairs})
    for c in np.unique(comp[~valid]):                             # an invalid component is entirely 999999
        assert (lab[idx[comp == c]] == 999999).all()
    # roots: labels 1, 2, ... in the order of each component's row-major minimum pixel
    first = {}
    for i, c in zip(idx.tolist(), comp.tolist()):
        first.setdefault(c, i)
    order = [lab[first[c]] for c in sorted(first, key=first.get) if lab[first[c]] != 999999]
    assert order == list(range(1, len(order) + 1))
    assert len(order) > 100


# ----------------------------------------------------------------------------- presets and the C ABI
def test_presets_equal_the_header_expressions(pl):
    P = pl.SEG_PRESETS
    exp = {   # ImageProjection.h:46-110: (N_SCAN, Horizon_SCAN, ang_res_x, ang_res_y, ang_bottom, groundScanInd)
        "VLP-16": (16, 1800, F(0.2), F(2.0), F(15.0 + 0.1), 7),
        "HDL-32E": (32, 1800, F(360.0 / 1800.0), F(41.33 / 31.0), F(30.67), 20),
        "HDL-64E": (64, 2250, F(360.0 / 2250.0), F(26.8 / 63.0), F(24.8), 7),
        "VLS-128": (128, 1800, F(0.2), F(0.3), F(25.0), 10),
        "RS-LIDAR-32": (32, 2000, F(0.18), F(40) / F(31), F(25.0), 2),
        "OS1-16": (16, 1024, F(360.0 / 1024.0), F(33.2 / 15.0), F(16.7), 7),
        "OS1-64": (64, 1024, F(360.0 / 1024.0), F(33.2 / 63.0), F(16.6 + 0.1), 15),
        "OS0-128": (128, 1024, F(360.0 / 1024.0), F(90) / F(127), F(45.1), 11),
    }
    assert list(P) == list(exp)
    for name, (n, h, rx, ry, bottom, g) in exp.items():
        p = P[name]
        assert (p.n_scan, p.horizon_scan, p.ground_scan_ind) == (n, h, g)
        assert (F(p.ang_res_x), F(p.ang_res_y), F(p.ang_bottom)) == (rx, ry, bottom), name
        assert (p.min_range, p.mount_angle, p.valid_point_num, p.valid_line_num) == (1.0, 0.0, 5, 3)
        assert F(p.segment_theta) == F(60.0 / 180.0 * math.pi)
    sx, cx, sy, cy = P["HDL-64E"].alphas()
    ax = F(float(F(360.0 / 2250.0)) / 180.0 * math.pi)
    assert sx == F(math.sin(float(ax))) and cx == F(math.cos(float(ax)))


def test_seg_params_struct_and_default_params_through_ctypes(pl, pkg):
    b = pkg.binding
    L = pkg.load_library()
    assert C.sizeof(b.SegParamsStruct) == 48
    for name, k in pl.SEG_PRESET_IDS.items():
        s = b.SegParamsStruct()
        assert L.svnicp_seg_default_params(k, C.byref(s)) == 0
        ref = pl.seg_params_struct(pl.SEG_PRESETS[name])
        assert bytes(s) == bytes(ref), name
    assert pl.SEG_PRESET_IDS["HDL-64E"] == 2
    assert L.svnicp_seg_default_params(8, C.byref(b.SegParamsStruct())) == -1
    assert L.svnicp_seg_default_params(-1, C.byref(b.SegParamsStruct())) == -1


# ----------------------------------------------------------------------------- C++ restatement
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("seg") / "segment_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "svn-icp_amd", "host"), os.path.join(ROOT, "tests", "segment_driver.cpp"), "-o", out])
    return out


def _cpp(pl, driver, tmp_path, pts, prm):
    pts = np.ascontiguousarray(np.asarray(pts, F))
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(bytes(pl.seg_params_struct(prm)))
        f.write(np.int32(pts.shape[0]).tobytes())
        f.write(pts.tobytes())
    r = subprocess.run([driver, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(tmp_path / "out.bin", "rb").read()
    m = int(np.frombuffer(raw, np.int64, 1)[0])
    o = 8
    xyz = np.frombuffer(raw, F, 3 * m, o).reshape(m, 3); o += 12 * m
    idx = np.frombuffer(raw, np.int64, m, o); o += 8 * m
    NP = prm.n_scan * prm.horizon_scan
    owner = np.frombuffer(raw, np.int32, NP, o); o += 4 * NP
    rng = np.frombuffer(raw, F, NP, o); o += 4 * NP
    ground = np.frombuffer(raw, np.int8, NP, o); o += NP
    label = np.frombuffer(raw, np.int32, NP, o); o += 4 * NP
    assert o == len(raw)
    return xyz, idx, [a.reshape(prm.n_scan, prm.horizon_scan) for a in (owner, rng, ground, label)]


def _scans(pkg, prm):
    sc = pkg.scans
    scene = sc.make_scene()
    R, t = sc.rot_zyx(0.0, 0.01, -0.5), np.array([2.0, 1.0, 0.1])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return {"grid": sc.lidar_grid_scan(scene, R, t, prm, 3),
            "bin_edge": sc.lidar_scan(scene, R, t, 131072, 4),
            "sweep": sc.lidar_sweep(scene, T, [0.004, -0.006, 0.05, 0.8, 0.1, -0.03], 65536, 5).points}


def test_cpp_and_python_restatements_are_bit_identical(pl, pkg, driver, tmp_path):
    prm = pl.SEG_PRESETS["HDL-64E"]
    for name, pts in _scans(pkg, prm).items():
        pts = np.asarray(pts, F).copy()
        if name == "sweep":
            pts[::97, 1] = np.nan                                 # non-finite points keep the indices of the rest
        xyz, idx, imgs = _cpp(pl, driver, tmp_path, pts, prm)
        hx, hi = pl.segment_scan(pts, prm)
        assert hx.shape[0] > 1000, name
        assert np.array_equal(idx, hi), name
        assert np.array_equal(xyz.view(np.uint32), hx.view(np.uint32)), name
        for a, b, what in zip(imgs, pl.segment_images(pts, prm), ("owner", "range", "ground", "label")):
            assert np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), (name, what)


@pytest.mark.parametrize("name", ["VLP-16", "OS0-128", "RS-LIDAR-32"])
def test_cpp_and_python_agree_on_other_presets(pl, pkg, driver, tmp_path, name):
    prm = pl.SEG_PRESETS[name]
    pts = pkg.scans.lidar_grid_scan(pkg.scans.make_scene(), np.eye(3), np.zeros(3), prm, 6)
    xyz, idx, imgs = _cpp(pl, driver, tmp_path, pts, prm)
    hx, hi = pl.segment_scan(pts, prm)
    assert np.array_equal(idx, hi) and np.array_equal(xyz, hx)
    assert all(np.array_equal(a, b) for a, b in zip(imgs, pl.segment_images(pts, prm)))


def test_grid_scan_hits_every_pixel_once(pl, pkg):
    for name in ("HDL-64E", "VLP-16", "OS0-128"):
        prm = pl.SEG_PRESETS[name]
        pts = pkg.scans.lidar_grid_scan(pkg.scans.make_scene(), np.eye(3), np.zeros(3), prm, 6, noise=0.0)
        owner, _ = pl._seg_project(pts, prm)
        assert np.array_equal(np.sort(owner), np.arange(prm.n_scan * prm.horizon_scan)), name
