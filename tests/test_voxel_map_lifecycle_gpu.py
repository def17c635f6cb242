"""The voxel map's table over a drive (csrc/map_table.hip, behind the entry points of csrc/voxel_map.hip): k_map_rehash moving
LIVE voxels, once at unchanged capacity because tombstones piled up and once into a table twice the size, then a cloud given by device pointer, svnicp_map_clear and a refill.
After every step the device map equals pipeline.VoxelHashMap bit for bit: len, the whole-map query and a range query that cuts
the map, in ascending voxel order (_host_rows of tests/test_voxel_map_gpu.py).

The sizes are chosen against the rule of svnicp_map_add_cloud — rebuild when (live + n) * 2 > capacity (growing) or when
tombstones * 4 > capacity — and the test asserts from svnicp_map_table_info and len(host map) that each rebuild happened where
it is meant to and moved more than 1000 live voxels, so a later change of sizes or of the rule cannot turn this back into a
rehash of an empty table.  Host model of this sequence (the host map and that rule): 18 301 live voxels and 2 764 tombstones
after step 1; 3 931 live and 17 134 tombstones before step 3 (4 * 17 134 > 65 536: rebuild at 65 536 slots); step 3's cloud meets
63 full voxels and 765 with room, re-creates 153 culled voxels and makes 13 346 new ones; 17 430 live before step 4
((17 430 + 30 000) * 2 > 65 536: rebuild into 131 072 slots).  On an MI355X: the same figures, table_info (65536, 2249, 1) after
the first rebuild and (131072, 3797, 2) after the second, 1.9 s.

Further down: every job of the map in turn on ONE map with all rows in host memory — query, normals, scoring, search, scoring
again, the taps — against each job run alone on a fresh identical map, bit for bit.  The jobs upload their rows into one shared
staging buffer and keep their results and validity flags apart (csrc/map_state.hpp); this is the test of that."""
import importlib
import math

import numpy as np
import pytest

from test_voxel_map_gpu import _host_rows

pytestmark = pytest.mark.gpu

VOXEL, MAX_POINTS, MAX_RANGE = 0.5, 3, 30.0
SLOTS = 1 << 16      # capacity_voxels=1: the smallest table


def _yaw_pose(yaw, t):
    T = np.eye(4)
    c, s = math.cos(yaw), math.sin(yaw)
    T[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = t
    return T


def _slab(rng, n, dense, centre):
    """n points of a +-28 x +-28 x +-2 m slab around the sensor, ``dense`` of them in a 4 x 4 x 1 m patch around ``centre``
    (64 voxels of 0.5 m, index 0 on z being double-width: they fill to max_points, and later clouds find them full), plus
    repeats of one point."""
    cloud = rng.uniform(-1, 1, size=(n, 3)) * [28.0, 28.0, 2.0]
    cloud[:dense] = np.asarray(centre) + rng.uniform(-1, 1, size=(dense, 3)) * [2.0, 2.0, 0.5]
    cloud = cloud.astype(np.float32)
    cloud[dense: dense + 40] = cloud[dense]
    return cloud


def sequence():
    """The clouds (sensor frame, float32) and poses of steps 1, 3, 4 and 5, and the pose of the empty step 2."""
    rng = np.random.default_rng(2024)
    P1 = _yaw_pose(0.0, [0.0, 0.0, 0.0])
    P2 = _yaw_pose(0.1, [40.0, 0.0, 0.0])                # 40 m on: everything farther than 30 m from here is culled
    P3 = _yaw_pose(0.15, [37.0, 1.0, 0.0])               # a little back: voxels culled in step 2 lie within range again
    P4 = _yaw_pose(0.2, [39.0, -1.0, 0.2])
    P5 = _yaw_pose(0.25, [42.0, 0.5, 0.0])
    c1 = _slab(rng, 26000, 1500, [20.0, 0.0, 0.0])       # the patch at world (20, 0, 0) survives step 2
    back = P3[:3, :3].T @ (np.array([20.0, 0.0, 0.0]) - P3[:3, 3])
    c3 = _slab(rng, 20000, 1500, back)                   # world (20, 0, 0) again: full voxels, and around them ones with room
    c4 = _slab(rng, 30000, 1500, [5.0, 5.0, 0.0])
    c5 = _slab(rng, 12000, 500, [-3.0, 2.0, 0.0])
    return dict(P1=P1, P2=P2, P3=P3, P4=P4, P5=P5, c1=c1, c3=c3, c4=c4, c5=c5)


def _check(tag, dm, hm, centre):
    assert len(dm) == len(hm), tag
    ptr, M = dm.get_map()
    want = _host_rows(hm)
    assert M == want.shape[0] and (ptr != 0 or M == 0), tag
    assert np.array_equal(dm.download(), want), tag
    Q = _yaw_pose(0.0, centre)
    ptr, M = dm.get_map(Q, 15.0)                         # a radius that cuts the map
    want = _host_rows(hm, Q, 15.0)
    assert 0 < want.shape[0] < _host_rows(hm).shape[0], tag
    assert M == want.shape[0], tag
    assert np.array_equal(dm.download(), want), tag


def test_rebuilds_with_live_voxels_and_tombstones(hip):
    import torch
    pl = importlib.import_module(hip.__name__ + ".pipeline")
    s = sequence()
    hm = pl.VoxelHashMap(VOXEL, MAX_RANGE, MAX_POINTS)
    dm = pl.DeviceVoxelHashMap(VOXEL, MAX_RANGE, MAX_POINTS, device=0, capacity_voxels=1)
    dm2 = pl.DeviceVoxelHashMap(VOXEL, MAX_RANGE, MAX_POINTS, device=0, capacity_voxels=1)   # step 5: fed from the host only
    empty = np.zeros((0, 3), np.float32)
    assert dm.table_info() == (SLOTS, 0, 0)

    def add(cloud, T):
        hm.add_pointcloud(cloud, T); dm.add_pointcloud(cloud, T); dm2.add_pointcloud(cloud, T)

    # 1. a slab around the sensor: no rebuild yet
    add(s["c1"], s["P1"])
    cap, tomb, reb = dm.table_info()
    print(f"step 1: live {len(hm)}, table_info {(cap, tomb, reb)}")
    assert (cap, reb) == (SLOTS, 0) and len(hm) > 15000 and tomb > 0
    _check("step 1", dm, hm, [10.0, 0.0, 0.0])

    # 2. an empty cloud 40 m on: only the cull runs
    before = len(hm)
    add(empty, s["P2"])
    cap, tomb, reb = dm.table_info()
    print(f"step 2: live {len(hm)} (was {before}), table_info {(cap, tomb, reb)}")
    assert (cap, reb) == (SLOTS, 0)
    assert 1000 < len(hm) < before // 3
    assert tomb * 4 > cap, "step 3 must find enough tombstones to rebuild at unchanged capacity"
    assert (len(hm) + s["c3"].shape[0]) * 2 <= cap, "step 3 must not grow the table"
    _check("step 2", dm, hm, [20.0, 0.0, 0.0])

    # 3. points into surviving voxels (with room, and full), into culled voxels, and into new ones: the rebuild for the
    #    tombstones moves the live voxels into a table of the same size
    old = {k: len(v) for k, v in hm._vox.items()}
    pts3 = pl.transform_f32(s["c3"], s["P3"])
    keys3 = set(map(tuple, np.trunc(pts3 / np.float32(VOXEL)).astype(np.int64).tolist()))
    hm1 = pl.VoxelHashMap(VOXEL, MAX_RANGE, MAX_POINTS); hm1.add_pointcloud(s["c1"], s["P1"])
    culled = set(hm1._vox) - set(old)
    live_at_rebuild = len(hm)
    add(s["c3"], s["P3"])
    n_full = sum(1 for k in keys3 if old.get(k) == MAX_POINTS)
    n_room = sum(1 for k in keys3 if 0 < old.get(k, 0) < MAX_POINTS)
    n_back = sum(1 for k in keys3 if k in culled and k in hm._vox)
    n_new = sum(1 for k in keys3 if k not in old and k not in culled and k in hm._vox)
    cap, tomb, reb = dm.table_info()
    print(f"step 3: rebuild with {live_at_rebuild} live voxels, table_info {(cap, tomb, reb)}; the cloud met {n_full} full voxels, "
          f"{n_room} with room, re-created {n_back} culled ones, made {n_new} new ones; live {len(hm)}")
    assert (cap, reb) == (SLOTS, 1) and live_at_rebuild > 1000
    assert tomb < live_at_rebuild + s["c3"].shape[0]     # the counter was reset: only this call's cull is in it
    assert min(n_full, n_room, n_back, n_new) >= 50
    _check("step 3", dm, hm, [30.0, 0.0, 0.0])

    # 4. growth: (live + n) * 2 > capacity
    live_at_rebuild = len(hm)
    assert (live_at_rebuild + s["c4"].shape[0]) * 2 > cap and live_at_rebuild > 1000
    add(s["c4"], s["P4"])
    cap, tomb, reb = dm.table_info()
    print(f"step 4: rebuild with {live_at_rebuild} live voxels, table_info {(cap, tomb, reb)}; live {len(hm)}")
    assert (cap, reb) == (2 * SLOTS, 2)
    _check("step 4", dm, hm, [35.0, 5.0, 0.0])

    # 5. a cloud that already lives in device memory; the other map gets the same rows from the host
    dev = torch.from_numpy(s["c5"]).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    hm.add_pointcloud(s["c5"], s["P5"])
    dm.add_pointcloud_device(dev.data_ptr(), dev.shape[0], s["P5"])
    dm2.add_pointcloud(s["c5"], s["P5"])
    _check("step 5", dm, hm, [45.0, -5.0, 0.0])
    _check("step 5, from the host", dm2, hm, [45.0, -5.0, 0.0])
    assert dm.table_info() == dm2.table_info()
    dm.get_map(); rows = dm.download()
    dm2.get_map()
    assert np.array_equal(rows, dm2.download())
    dm2.close()

    # 6. clear: empty, counters reset, capacity and rebuild count kept
    dm.add_pointcloud(np.array([[np.nan, 0, 0], [1e9, 0, 0]], np.float32), s["P5"])      # something for clear to reset
    hm.remove_far(s["P5"][:3, 3])
    assert dm.skipped_points() == 2 and len(dm) == len(hm)
    assert hip.load_library().svnicp_map_clear(dm._h) == 0
    assert len(dm) == 0 and dm.empty()
    assert dm.get_map()[1] == 0 and dm.download().shape == (0, 3)
    assert dm.get_map(s["P5"], 1e9)[1] == 0 and dm.download().shape == (0, 3)
    assert dm.skipped_points() == 0
    assert dm.table_info() == (2 * SLOTS, 0, 2)

    # 7. refill: equal to a fresh host map
    fresh = pl.VoxelHashMap(VOXEL, MAX_RANGE, MAX_POINTS)
    fresh.add_pointcloud(s["c1"], s["P1"]); dm.add_pointcloud(s["c1"], s["P1"])
    _check("step 7", dm, fresh, [10.0, 0.0, 0.0])
    assert dm.table_info()[0] == 2 * SLOTS and dm.table_info()[2] == 2


# ---------------------------------------------------------------------------------------------
# One map, every job in turn, all rows from host memory: the jobs share ONE staging buffer for uploaded rows
# (stage_rows, csrc/map_state.hpp) and each keeps its own results and validity flag, so no job may disturb what another left.
# ---------------------------------------------------------------------------------------------
NORMALS_REFUSAL = ("svnicp_map_query_normals: no svnicp_map_query yet, or the map changed (add_cloud / clear_seen_through / clear) "
                   "since the last one")


def _two_scans():
    """Two synthetic scans of 2048 points (a 10 x 10 x 2 m slab: three to four points per 0.5 m voxel) and their poses."""
    rng = np.random.default_rng(77)
    clouds = [(rng.uniform(-1, 1, size=(2048, 3)) * [5.0, 5.0, 1.0]).astype(np.float32) for _ in range(2)]
    return clouds, [_yaw_pose(0.0, [0.0, 0.0, 0.0]), _yaw_pose(0.05, [0.5, 0.0, 0.0])]


def _poses(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([_yaw_pose(rng.uniform(-0.05, 0.05), rng.uniform(-0.3, 0.3, size=3)) for _ in range(n)])


def _search_bytes(top, level):
    return b"".join(d[k].tobytes() for d, keys in ((top, ("lattice", "corrections", "poses", "records")),
                                                   (level, ("lattice", "poses", "records", "kept"))) for k in keys)


def test_jobs_share_the_staging_buffer_and_keep_their_own_results(hip):
    pl = importlib.import_module(hip.__name__ + ".pipeline")
    binding = importlib.import_module(hip.__name__ + ".binding")
    clouds, poses = _two_scans()
    gate = 0.4
    search_args = (_yaw_pose(0.02, [0.1, 0.0, 0.0]), [0.6, 0, 0, 0, 0, 0], [0.3, 0, 0, 0, 0, 0], 2, 4, gate)   # x alone: m = 2

    def fresh():
        dm = pl.DeviceVoxelHashMap(0.5, 100.0, 20, device=0, capacity_voxels=1)
        for c, T in zip(clouds, poses):
            dm.add_pointcloud(c, T)                                           # 1.
        return dm

    # each job alone on a freshly built identical map
    dm = fresh(); ref_score = dm.score_poses(clouds[0], _poses(9, 1), gate); dm.close()
    dm = fresh(); dm.search_poses(clouds[0], *search_args); ref_search = _search_bytes(dm.search_top(), dm.search_level(0)); dm.close()
    dm = fresh()
    _, ref_M = dm.get_map(); _, ref_with = dm.get_map_normals()
    ref_rows, ref_normals = dm.download(), dm.download_normals()
    dm.close()
    assert ref_M > 1000 and ref_with > 100 and ref_rows.shape == ref_normals.shape == (ref_M, 3)
    assert len(ref_search) == 4 * (6 * 4 + 6 * 8 + 12 * 8 + 4 * 8) + 5 * (6 * 4 + 12 * 8 + 4 * 8) + 4 * 4   # 4 kept, 5 nodes at level 0

    # the sequence on one map
    dm = fresh()
    _, M = dm.get_map()                                                       # 2.
    _, with_normal = dm.get_map_normals()                                     # 3.
    score = dm.score_poses(clouds[0], _poses(9, 1), gate)                     # 4.
    res = dm.search_poses(clouds[0], *search_args)                            # 5.
    assert res["level_count"] == [5, 12] and res["level_kept"] == [4, 4]
    other = dm.score_poses(clouds[1], _poses(9, 2), gate)                     # 6. other rows, other poses
    top = dm.search_top()                                                     # 7.
    level0 = dm.search_level(0)                                               # 8.
    rows = dm.download()                                                      # 9.
    normals = dm.download_normals()                                           # 10.
    assert (M, with_normal) == (ref_M, ref_with)
    assert rows.tobytes() == ref_rows.tobytes() and normals.tobytes() == ref_normals.tobytes()
    assert _search_bytes(top, level0) == ref_search
    assert score.tobytes() == ref_score.tobytes() and other.tobytes() != score.tobytes()

    # a further cloud: the selection and the normals are dropped, the search's results do not depend on the table
    dm.add_pointcloud(clouds[0], _yaw_pose(0.1, [1.0, 0.0, 0.0]))
    with pytest.raises(binding.SvnIcpError) as e:
        dm.get_map_normals()
    assert str(e.value).endswith(NORMALS_REFUSAL)
    assert dm.download_normals().shape == (0, 3)
    assert _search_bytes(dm.search_top(), dm.search_level(0)) == ref_search
    dm.close()
