"""The limits the voxel map states (csrc/map_table.hip, include/svnicp_hip.h), hit exactly: the voxel index range [-2^20, 2^20)
at both bounds (storage, the skipped-points counter and the neighbour-range test of k_map_normals), points on voxel faces
(truncf of a float32 division), a distance equal to the radius in the cull (>) and in the range query (<), max_points 1 and
256 with a voxel that fills inside one run, and the degenerate calls.  Every map is compared bit for bit with
pipeline.VoxelHashMap fed the same rows (_host_rows of tests/test_voxel_map_gpu.py); normals with
tests/map_normals_reference.py under the rule of tests/test_map_normals_gpu.py (_compare, unchanged)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import map_normals_reference as mr
from test_map_normals_gpu import _check_queries
from test_voxel_map_gpu import _host_rows

pytestmark = pytest.mark.gpu

LIM = 1 << 20


def _same(tag, dm, hm, cut=None):
    assert len(dm) == len(hm), tag
    for args in ((),) + ((cut,) if cut else ()):
        ptr, M = dm.get_map(*args)
        want = _host_rows(hm, *args)
        assert M == want.shape[0], (tag, args)
        assert np.array_equal(dm.download(), want), (tag, args)


def _at(t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    T[:3, 3] = t
    return T


# ---------------------------------------------------------------------------------------------
# 1. the index range
# ---------------------------------------------------------------------------------------------
def index_range_cloud():
    """-> (cloud float32, stored mask).  Voxel 1.0.  On every axis four layers of voxels, indices -2^20, -2^20 + 1, 2^20 - 2 and
    2^20 - 1, each 3 x 3 voxels wide on the other two axes (indices 0..2) with 10 points per voxel; three corners where all three
    indices sit at a bound, 2 x 2 x 2 voxels of 8 points; and the points just outside.  Coordinates near 2^20 are multiples of
    0.125 (float32 spacing there), so every value is exact.  The other axes' indices 0..2 are shared by the low and the high layers:
    an index 2^20 packed into 21 bits sets the lowest bit of the next field, which names voxel (.., b | 1, -2^20) of the low layer.
    In k_map_locate that stores a point in the wrong voxel (the skipped count and the rows show it).  In k_map_normals such a
    neighbour is 2^21 voxels away: its points are never among the nearest of a block that has normal_k points of its own, and a
    block that has not gets the zero row either way (one far neighbour leaves lambda1 / lambda2 near 2^-42), so the normals here
    pin the rows of the bound voxels, not the neighbour-range test itself (measured: a build without it passes)."""
    rng = np.random.default_rng(20)
    eighth = lambda n: rng.integers(0, 8, size=n) * 0.125
    layers = {-LIM: lambda n: -(LIM + eighth(n)), -LIM + 1: lambda n: -(LIM - 1 + eighth(n)),
              LIM - 2: lambda n: LIM - 2 + eighth(n), LIM - 1: lambda n: LIM - 1 + eighth(n)}
    rows = []
    for axis in range(3):
        o1, o2 = [a for a in range(3) if a != axis]
        for layer, draw in layers.items():
            for b in range(3):
                for c in range(3):
                    p = np.zeros((10, 3))
                    p[:, axis] = draw(10)
                    p[:, o1] = b + rng.uniform(0.05, 0.95, 10)
                    p[:, o2] = c + rng.uniform(0.05, 0.95, 10)
                    rows.append(p)
    for signs in ((-1, -1, -1), (1, 1, 1), (-1, 1, -1)):
        for off in np.ndindex(2, 2, 2):
            p = np.zeros((8, 3))
            for d in range(3):
                p[:, d] = layers[(-LIM + off[d]) if signs[d] < 0 else (LIM - 1 - off[d])](8)
            rows.append(p)
    named = np.zeros((9, 3)) + 0.5                      # the values the contract names, on each axis
    for axis in range(3):
        named[3 * axis: 3 * axis + 3, axis] = [-1048576.0, -1048575.5, 1048575.5]
    rows.append(named)
    stored = np.concatenate(rows, 0)
    out = np.zeros((18, 3)) + 0.5
    for axis in range(3):
        out[6 * axis: 6 * axis + 6, axis] = [-1048577.0, 1048576.0, np.inf, -np.inf, -1048576.0 - 1.125, 1048576.0 + 0.125]
    corner_out = np.array([[1048576.0, 1048575.5, -1048576.0], [-1048577.0, -1048577.0, -1048577.0], [np.inf, -np.inf, 1048576.0]])
    cloud = np.concatenate([stored, out, corner_out], 0)
    mask = np.concatenate([np.ones(stored.shape[0], bool), np.zeros(out.shape[0] + 3, bool)])
    perm = rng.permutation(cloud.shape[0])
    cloud32 = cloud[perm].astype(np.float32)
    big = np.abs(cloud[perm]) > 1e6
    assert np.array_equal(cloud32.astype(np.float64)[big], cloud[perm][big])      # every coordinate near a bound is exact in float32
    return cloud32, mask[perm]


def test_index_range_bounds(hip):
    pl = importlib.import_module(hip.__name__ + ".pipeline")
    cloud, stored = index_range_cloud()
    assert int((~stored).sum()) == 21
    hm = pl.VoxelHashMap(1.0, 1e9, 20)
    dm = pl.DeviceVoxelHashMap(1.0, 1e9, 20, device=0, capacity_voxels=1)
    half = cloud.shape[0] // 2
    for part, keep in ((cloud[:half], stored[:half]), (cloud[half:], stored[half:])):
        dm.add_pointcloud(part, np.eye(4)); hm.add_pointcloud(part[keep], np.eye(4))
    assert dm.skipped_points() == 21
    keys = np.array(sorted(hm._vox))
    assert keys.min() == -LIM and keys.max() == LIM - 1
    for axis in range(3):
        assert {-LIM, -LIM + 1, LIM - 2, LIM - 1} <= set(keys[:, axis].tolist())
    for corner in ((-LIM,) * 3, (LIM - 1,) * 3, (-LIM, LIM - 1, -LIM)):
        assert corner in hm._vox
    bound = [k for k in hm._vox if min(k) == -LIM or max(k) == LIM - 1]
    near = [k for k in hm._vox if min(k) == -LIM + 1 or max(k) == LIM - 2]
    assert len(bound) >= 6 * 9 and min(len(hm._vox[k]) for k in bound + near) >= 8
    _same("index range", dm, hm, (_at(t=(-float(LIM), 1.5, 1.5)), 4.0))
    # a bound voxel as the centre of k_map_normals: neighbours beyond the range do not exist
    ref = mr.map_normals(hm._vox, 4)
    at_bound = np.repeat([min(k) == -LIM or max(k) == LIM - 1 for k in ref.keys], np.diff(ref.offs))
    print(f"index range: {len(hm)} voxels, {len(bound)} at a bound, rows of bound voxels {int(at_bound.sum())}, "
          f"with a normal {int(ref.valid[at_bound].sum())}")
    assert ref.valid[at_bound].sum() >= 0.9 * at_bound.sum()
    _check_queries("index range", dm, hm._vox, ref, 4, _at(t=(1.5, float(LIM - 1), 1.5)), 4.0)


# ---------------------------------------------------------------------------------------------
# 2. voxel faces
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v,axis,shift", [(0.1, 0, 0.0), (0.3, 1, 0.0), (0.1, 2, 0.5), (0.3, 0, 0.5)])
def test_points_on_voxel_faces(hip, v, axis, shift):
    """Lattice values float32(k * v), k = -3000..3000, divided by float32(v) in float32: most quotients are exactly k, the
    others round to just inside the face and truncate to the index one nearer zero (788 of 6001 at v = 0.1, 2806 at 0.3).  A
    division that is not correctly rounded moves points between the two kinds.  shift: the pose's translation in voxels."""
    pl = importlib.import_module(hip.__name__ + ".pipeline")
    rng = np.random.default_rng(int(v * 10) + axis)
    k = np.arange(-3000, 3001)
    cloud = rng.uniform(-5, 5, size=(k.size, 3)).astype(np.float32)
    cloud[:, axis] = (k * v).astype(np.float32)
    tiny = rng.uniform(-1, 1, size=(200, 3)).astype(np.float32) * np.float32(v)      # (-v, v): the double-width voxel 0
    tiny[:4, axis] = [0.0, -0.0, np.nextafter(np.float32(v), np.float32(0)), -np.nextafter(np.float32(v), np.float32(0))]
    cloud = np.concatenate([cloud, tiny], 0)
    cloud = cloud[rng.permutation(cloud.shape[0])]
    if shift == 0.0:
        idx = np.trunc(cloud[:, axis] / np.float32(v)).astype(np.int64)
        lat = np.isin(cloud[:, axis], (k * v).astype(np.float32))
        kk = np.rint(cloud[lat, axis].astype(np.float64) / v).astype(np.int64)
        on_k = int((idx[lat] == kk).sum())
        nearer = int(((np.abs(idx[lat]) == np.abs(kk) - 1) & (kk != 0)).sum())
        print(f"voxel {v}: {on_k} lattice values land on k, {nearer} one index nearer zero")
        assert on_k > 500 and nearer > 500 and on_k + nearer == int(lat.sum())
    T = _at(t=tuple(shift * v if d == axis else 0.0 for d in range(3)))
    hm = pl.VoxelHashMap(v, 1e9, 20)
    dm = pl.DeviceVoxelHashMap(v, 1e9, 20, device=0, capacity_voxels=1)
    dm.add_pointcloud(cloud, T); hm.add_pointcloud(cloud, T)
    assert dm.skipped_points() == 0
    assert (0, 0, 0) in hm._vox
    _same(f"faces {v} axis {axis} shift {shift}", dm, hm, (_at(t=(1.0, -2.0, 0.5)), 60.0))


# ---------------------------------------------------------------------------------------------
# 3. a distance equal to the radius
# ---------------------------------------------------------------------------------------------
def test_distance_equal_to_the_radius(hip):
    pl = importlib.import_module(hip.__name__ + ".pipeline")
    on = np.array([[3, 4, 0], [0, -5, 0], [-4, 0, 3], [0, 0, 5], [5, 0, 0], [-3, 0, -4], [0, 3, -4], [4, -3, 0]], np.float32)
    inside = np.array([[0, 0, 0], [1, 1, 1], [4, 2, 2], [3, 3, 2], [-4, -2, -2], [2, -4, 2], [0, 4, -2]], np.float32)
    outside = np.array([[4, 3, 1], [5, 1, 0], [0, 0, 6], [-5, -1, 0], [3, -3, 3], [-4, 3, -1], [40, 0, 0]], np.float32)
    assert np.all((on.astype(int) ** 2).sum(1) == 25) and np.all((inside.astype(int) ** 2).sum(1) < 25)
    assert np.all((outside.astype(int) ** 2).sum(1) > 25) and (outside.astype(int) ** 2).sum(1).min() == 26
    assert (inside.astype(int) ** 2).sum(1).max() == 24
    rng = np.random.default_rng(5)
    cloud = np.concatenate([on, inside, outside], 0)[rng.permutation(22)]
    hm = pl.VoxelHashMap(1.0, 5.0, 1)
    dm = pl.DeviceVoxelHashMap(1.0, 5.0, 1, device=0, capacity_voxels=1)
    dm.add_pointcloud(cloud, np.eye(4)); hm.add_pointcloud(cloud, np.eye(4))
    assert len(hm) == 15
    assert len(dm) == 15                                  # the cull is >: distance 5 survives, distance sqrt(26) does not
    dm.get_map()
    got = dm.download()
    assert np.array_equal(got, _host_rows(hm))
    assert {tuple(r) for r in got.tolist()} == {tuple(r) for r in np.concatenate([on, inside]).astype(float).tolist()}
    ptr, M = dm.get_map(np.eye(4), 5.0)                   # the query is <: distance 5 is not returned
    assert M == 7
    assert np.array_equal(dm.download(), _host_rows(hm, np.eye(4), 5.0))
    assert {tuple(r) for r in dm.download().tolist()} == {tuple(r) for r in inside.astype(float).tolist()}
    ptr, M = dm.get_map(np.eye(4), 5.0000001)
    assert 5.0000001 ** 2 > 25.0 and M == 15
    assert np.array_equal(dm.download(), _host_rows(hm, np.eye(4), 5.0000001))
    dm.add_pointcloud(np.zeros((0, 3), np.float32), np.eye(4)); hm.add_pointcloud(np.zeros((0, 3), np.float32), np.eye(4))
    assert len(dm) == len(hm) == 15                       # a cull alone leaves distance 5 in place as well
    assert dm.table_info()[1] == 7                        # the seven voxels outside are the tombstones


# ---------------------------------------------------------------------------------------------
# 4. max_points 1 and 256
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mp", [1, 256])
def test_a_voxel_fills_inside_a_run(hip, mp):
    """Two clouds: one voxel takes 3000 points of the first (the run crosses max_points at once), twelve others take about 150
    points from each cloud (at max_points 256 counts + rank crosses the cut inside the second cloud's run)."""
    pl = importlib.import_module(hip.__name__ + ".pipeline")
    rng = np.random.default_rng(mp)
    hm = pl.VoxelHashMap(1.0, 1e9, mp)
    dm = pl.DeviceVoxelHashMap(1.0, 1e9, mp, device=0, capacity_voxels=1)
    corners = np.array([[5, 5, 5]] + [[a, b, 8] for a in range(4) for b in range(3)], float)
    sizes = []
    for call in range(2):
        n_per = [3000 if call == 0 else 10] + list(rng.integers(120, 180, size=12))
        cloud = np.concatenate([c + rng.uniform(0.01, 0.99, size=(n, 3)) for c, n in zip(corners, n_per)], 0)
        cloud = cloud[rng.permutation(cloud.shape[0])].astype(np.float32)
        dm.add_pointcloud(cloud, np.eye(4)); hm.add_pointcloud(cloud, np.eye(4))
        sizes.append([len(hm._vox[tuple(int(x) for x in c)]) for c in corners])
        _same(f"max_points {mp} call {call}", dm, hm, (_at(t=(2.0, 1.0, 8.0)), 2.0))
    assert len(hm) == 13 and sizes[1] == [mp] * 13
    assert sizes[0][0] == mp and (mp == 1 or max(sizes[0][1:]) < mp)      # the other voxels fill in the second call
    assert dm.skipped_points() == 0


# ---------------------------------------------------------------------------------------------
# 5. degenerate calls
# ---------------------------------------------------------------------------------------------
def test_empty_calls_and_refused_maps(hip):
    pl = importlib.import_module(hip.__name__ + ".pipeline")
    L = hip.load_library()
    dm = pl.DeviceVoxelHashMap(0.5, 10.0, 4, device=0, capacity_voxels=1)
    assert dm.get_map()[1] == 0 and dm.download().shape == (0, 3)       # a query on a map that was never filled
    dm.add_pointcloud(np.zeros((0, 3), np.float32), _at(t=(3.0, 0.0, 0.0)))
    assert len(dm) == 0 and dm.empty() and dm.skipped_points() == 0
    assert dm.table_info() == (1 << 16, 0, 0)
    assert dm.get_map()[1] == 0 and dm.download().shape == (0, 3)
    assert dm.get_map(np.eye(4), 100.0)[1] == 0 and dm.download().shape == (0, 3)
    nptr, with_normal = dm.get_map_normals(16)
    assert (nptr, with_normal) == (0, 0) and dm.download_normals().shape == (0, 3)
    dm.add_pointcloud(np.array([[1, 1, 1]], np.float32), np.eye(4))      # and it still takes points afterwards
    assert len(dm) == 1 and dm.get_map()[1] == 1
    assert np.array_equal(dm.download(), [[1.0, 1.0, 1.0]])
    for voxel, mp in ((0.5, 0), (0.5, 257), (0.0, 20), (-1.0, 20), (float("nan"), 20)):
        h = C.c_void_p()
        assert L.svnicp_map_create(0, voxel, 10.0, mp, 0, C.byref(h)) == -1 and not h.value
        text = L.svnicp_map_last_error(None).decode()
        assert "voxel_size > 0" in text and "max_points <= 256" in text
        with pytest.raises(hip.binding.SvnIcpError, match="max_points"):
            pl.DeviceVoxelHashMap(voxel, 10.0, mp, device=0)
    for mp in (1, 256):                                                   # the limits themselves are accepted
        pl.DeviceVoxelHashMap(0.5, 10.0, mp, device=0, capacity_voxels=1).close()
