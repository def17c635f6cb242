"""svnicp_map_score_poses on the device against the numpy restatement (pipeline.VoxelHashMap.score_poses), DESIGN.md §4.16.
Standing rule (map_score_cases.assert_scores_match): located and inliers exactly equal, sum_d2 and cost within 1e-12 relative
-- the restatement adds in row order, the device in a fixed tree over 256-row chunks; at most a few thousand terms of like sign."""
import ctypes as C
import importlib

import numpy as np
import pytest

import map_normals_cases as mn
import map_score_cases as ms

pytestmark = pytest.mark.gpu
INVALID = -1   # SVNICP_ERR_INVALID


@pytest.fixture(scope="module")
def pl(hip):
    return importlib.import_module(hip.__name__ + ".pipeline")


def _device_map(pl, voxel, max_range, max_points, steps, capacity_voxels=0):
    dm = pl.DeviceVoxelHashMap(voxel, max_range, max_points, device=0, capacity_voxels=capacity_voxels)
    for cloud, T in steps:
        dm.add_pointcloud(cloud, T)
    return dm


@pytest.fixture(scope="module")
def drive(pl):
    voxel, mp, max_range, steps = ms.drive_steps()
    dm = _device_map(pl, voxel, max_range, mp, steps)
    hm = mn.host_map("drive")
    assert len(dm) == len(hm)
    yield dm, hm
    dm.close()


# ------------------------------------------------------------------------------------------------ 1. the crafted case
@pytest.mark.parametrize("voxel", [1.0, 0.5])
@pytest.mark.parametrize("max_points", [3, 20])
def test_crafted_case_with_odd_rows_and_poses(pl, voxel, max_points):
    stored, rows, poses = ms.crafted(voxel)
    odd = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e6, 0, 0], [0, -3e6, 0]], np.float32)   # not located, any pose
    rows = np.concatenate([rows[:100], odd, rows[100:]], 0)
    bad = np.eye(4)[None].copy()
    bad[0, 2, 0] = np.nan
    poses = np.concatenate([poses, bad, ms.pose(t=(1e6, 0, 0))[None]], 0)
    hm = ms.crafted_host_map(voxel, max_points)
    dm = _device_map(pl, voxel, 1e9, max_points, [(stored, np.eye(4))])
    for gate in ms.crafted_gates(voxel):
        want = hm.score_poses(rows, poses, gate)
        got = dm.score_poses(rows, poses, gate)
        ms.assert_scores_match(got, want, f"gate {gate}")
        assert np.array_equal(got, want)                      # these inputs are exact in float64: no rounding in any order
        assert got[-2].tolist() == [0.0, 0.0, 0.0, gate * gate] and got[-1].tolist() == [0.0, 0.0, 0.0, gate * gate]
        assert 0 < got[0, 1] < got[0, 0] <= rows.shape[0] - odd.shape[0]
    dm.close()


# ------------------------------------------------------------------------------------------------ 2. chunk boundaries
def test_row_counts_across_the_chunk_boundaries(pl, drive):
    dm, hm = drive
    R = ms.ROWS_PER_WORKGROUP
    poses = ms.drive_poses(65)
    for n in sorted({0, 1, 63, 64, 65, 255, 256, 257, R - 1, R, R + 1, 3 * R + 7}):
        rows = ms.drive_rows(n)
        want = hm.score_poses(rows, poses, 0.5)
        for Cn in (1, 2, 65):
            ms.assert_scores_match(dm.score_poses(rows, poses[:Cn], 0.5), want[:Cn], f"n {n} C {Cn}")
        assert n == 0 or want[0, 1] > 0.4 * n                 # the true pose: the rows do find the map
        if n == 0:
            assert dm.score_poses(rows, poses[:2], 0.5).tolist() == [[0.0, 0.0, 0.0, 0.25]] * 2


# ------------------------------------------------------------------------------------------------ 3. batch independence
class _DeviceDoubles:
    """Library-owned float64 device memory as torch sees it (__cuda_array_interface__)."""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f8", "data": (int(ptr), False), "version": 2, "strides": None}


def test_batch_independence_and_determinism(pl, drive):
    import torch
    dm, hm = drive
    rows, poses = ms.drive_rows(800), ms.drive_poses(64)
    batch = dm.score_poses(rows, poses, 0.5)
    ms.assert_scores_match(batch, hm.score_poses(rows, poses, 0.5))
    assert dm.score_poses(rows, poses, 0.5).tobytes() == batch.tobytes()                                    # two calls in a row
    for c in range(64):
        assert dm.score_poses(rows, poses[c:c + 1], 0.5).tobytes() == batch[c:c + 1].tobytes(), c            # alone = in the batch
    assert dm.score_poses(rows, poses[40:], 0.5).tobytes() == batch[40:].tobytes()
    d_rows = torch.from_numpy(rows).to("cuda:0").contiguous()
    d_poses = torch.from_numpy(pl.pose_rows(poses)).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    assert dm.score_poses_device(d_rows.data_ptr(), 800, poses, 0.5).tobytes() == batch.tobytes()          # rows on the device
    assert dm.score_poses(rows, d_poses, 0.5).tobytes() == batch.tobytes()                                  # poses on the device
    assert dm.score_poses_device(d_rows.data_ptr(), 800, d_poses, 0.5).tobytes() == batch.tobytes()
    # outCx4 may be NULL: the records are read through the device pointer
    rc = dm._L.svnicp_map_score_poses(dm._h, rows.ctypes.data_as(C.c_void_p), 800, 0, C.c_void_p(d_poses.data_ptr()), 64, 1, 0.5, None)
    assert rc == 0 and dm.scores_ptr != 0
    view = torch.as_tensor(_DeviceDoubles(dm.scores_ptr, (64, 4)), device="cuda:0")
    assert view.cpu().numpy().tobytes() == batch.tobytes()


# ------------------------------------------------------------------------------------------------ 4. tombstones, rebuilt table
def test_table_with_tombstones_and_a_rebuilt_table(pl):
    rng = np.random.default_rng(4)
    steps = [((rng.uniform(-10, 10, size=(40000, 3))).astype(np.float32), np.eye(4))]       # more than half the 65536 slots could be needed: growth
    for x in (4.0, 8.0):                                                                    # along a line: the range cull leaves tombstones behind
        steps.append(((rng.uniform(-10, 10, size=(2000, 3))).astype(np.float32), ms.pose(t=(x, 0, 0))))
    dm = _device_map(pl, 1.0, 15.0, 5, steps, capacity_voxels=1)
    hm = pl.VoxelHashMap(1.0, 15.0, 5)
    for cloud, T in steps:
        hm.add_pointcloud(cloud, T)
    cap, tomb, rebuilds = dm.table_info()
    assert cap > 65536 and rebuilds >= 1 and tomb > 0, (cap, tomb, rebuilds)
    assert len(dm) == len(hm)
    rows = rng.uniform(-10, 10, size=(700, 3)).astype(np.float32)
    poses = np.array([ms.pose(t=(x, 0, 0)) for x in (8.0, 4.0, 0.0, -4.0)] + [ms.pose(ms.rot90(2, 1), (8.0, 0.5, 0))])
    want = hm.score_poses(rows, poses, 1.0)
    assert want[0, 1] > 300 and want[3, 0] < want[0, 0]                                     # rows over live voxels | over the culled end
    ms.assert_scores_match(dm.score_poses(rows, poses, 1.0), want)
    ms.assert_scores_match(dm.score_poses(rows, poses, 0.3), hm.score_poses(rows, poses, 0.3))
    assert dm.table_info() == (cap, tomb, rebuilds)
    dm.close()


# ------------------------------------------------------------------------------------------------ 5. index-range edges
def test_index_range_edges(pl):
    hi, lo = float(2 ** 20 - 1), float(-2 ** 20)                                             # voxel 1.0 keeps these exact in float32
    stored = np.array([[hi + 0.5, 0.5, 0.5], [lo - 0.5, 0.5, 0.5], [0.5, hi + 0.25, lo - 0.25], [lo - 0.5, lo - 0.5, lo - 0.5],
                       [lo - 0.25, 0.5, 0.5], [0.5, 0.5, 0.5], [hi + 0.5, hi + 0.5, hi + 0.5]], np.float32)
    rows = np.array([[hi + 0.75, 0.5, 0.5], [hi - 0.25, 0.75, 0.5], [hi - 1.5, 0.5, 0.5], [lo - 0.25, 0.25, 0.5], [lo + 0.5, 0.5, 0.5],
                     [lo + 1.5, 0.5, 0.5], [hi + 1.0, 0.5, 0.5], [lo - 1.0, 0.5, 0.5], [0.5, hi + 0.5, lo - 0.5], [0.25, hi - 0.5, lo + 0.5],
                     [lo - 0.25, lo - 0.25, lo - 0.25], [hi + 0.25, hi + 0.25, hi + 0.25], [0.25, 0.25, 0.25], [-0.75, 0.5, 0.5]], np.float32)
    poses = np.array([ms.pose(), ms.pose(t=(1.0, 0, 0)), ms.pose(t=(-1.0, 0, 0)), ms.pose(t=(0, -0.5, 0.5)), ms.pose(ms.rot90(2, 2), (0, 1.0, 0))])
    hm = pl.VoxelHashMap(1.0, 1e12, 20)
    hm.add_pointcloud(stored, np.eye(4))
    dm = _device_map(pl, 1.0, 1e12, 20, [(stored, np.eye(4))])
    assert len(dm) == len(hm) and dm.skipped_points() == 0
    for gate in (1.0, 0.5):
        want = hm.score_poses(rows, poses, gate)
        got = dm.score_poses(rows, poses, gate)
        ms.assert_scores_match(got, want, f"gate {gate}")
        assert np.array_equal(got, want)                                                     # exact inputs again
    assert hm.score_poses(rows, poses, 1.0)[0, 0] == 10     # identity: all but the two rows outside and the two rows two voxels from an edge point
    one = dm.score_poses(rows[6:8], poses[:1], 1.0)                                          # rows outside +-2^20: not located,
    assert one[0].tolist() == [0.0, 0.0, 0.0, 1.0]                                           # and no neighbour index wraps into a key
    dm.close()


# ------------------------------------------------------------------------------------------------ 6. a dense map
@pytest.mark.parametrize("max_points", [1, 256])
def test_dense_map_at_the_full_gate(pl, max_points):
    voxel, _, max_range, steps = mn.case_inputs("dense256")
    hm = pl.VoxelHashMap(voxel, max_range, max_points)
    for cloud, T in steps:
        hm.add_pointcloud(cloud, T)
    dm = _device_map(pl, voxel, max_range, max_points, steps)
    rng = np.random.default_rng(6)
    cloud = np.concatenate([c for c, _ in steps], 0)
    rows = (cloud[rng.choice(cloud.shape[0], 500, replace=False)] + rng.normal(size=(500, 3)) * 0.3).astype(np.float32)
    rows[:8] = [[0.999, 0.5, 0.5], [-0.999, 0.5, 0.5], [0.001, -0.001, 0.5], [1.001, 0.999, -0.999], [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0],
                [0.0, 0.0, 0.0], [1.999, -1.999, 0.0]]                                        # around the double-width voxel 0
    poses = np.array([ms.pose(), ms.pose(t=(0.37, -0.81, 0.22)), ms.pose(ms.rot90(2, 1), (-0.9, 0.4, 0.0)),
                      ms.pose(t=(0.999, 0.999, -0.999))])
    for gate in (voxel, 0.4 * voxel):                          # every one of the 27 voxels matters | most lie beyond the gate
        want = hm.score_poses(rows, poses, gate)
        assert 0 < want[0, 1] <= want[0, 0]
        ms.assert_scores_match(dm.score_poses(rows, poses, gate), want, f"gate {gate}")
    dm.close()


# ------------------------------------------------------------------------------------------------ 7. side effects
def test_no_side_effects_on_the_map(pl):
    voxel, mp, max_range, steps = ms.drive_steps()
    dm = _device_map(pl, voxel, max_range, mp, steps[:3])
    twin = _device_map(pl, voxel, max_range, mp, steps[:3])
    centre, radius = ms.drive_scan(4)[1], 30.0
    _, M = dm.get_map(centre, radius)
    _, with_normal = dm.get_map_normals(16)
    rows0, nrm0, info0, size0 = dm.download(), dm.download_normals(), dm.table_info(), len(dm)
    assert M > 1000 and with_normal > 0
    scores = dm.score_poses(ms.drive_rows(800), ms.drive_poses(16), 0.5)
    assert scores[0, 1] > 0
    assert np.array_equal(dm.download(), rows0) and np.array_equal(dm.download_normals(), nrm0)
    assert dm.get_map_normals(16)[1] == with_normal            # still accepted: the query is still valid
    assert np.array_equal(dm.download_normals(), nrm0)
    assert dm.table_info() == info0 and len(dm) == size0
    cloud, T = steps[3]
    dm.add_pointcloud(cloud, T); twin.add_pointcloud(cloud, T)
    dm.get_map(); twin.get_map()
    assert dm.table_info() == twin.table_info() and len(dm) == len(twin)
    assert dm.download().tobytes() == twin.download().tobytes()
    dm.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 8. refusals and empties
def test_refusals_and_empties(pl, drive):
    dm, _ = drive
    L, h = dm._L, dm._h
    rows = ms.drive_rows(100)
    P = pl.pose_rows(ms.drive_poses(3))
    out = np.zeros((3, 4))
    rp, pp, op = rows.ctypes.data_as(C.c_void_p), P.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.POINTER(C.c_double))

    def refused(*args):
        rc = L.svnicp_map_score_poses(*args)
        return rc == INVALID and len(L.svnicp_map_last_error(h).decode()) > 10

    assert refused(h, rp, 100, 0, pp, 3, 0, 0.5 + 1e-9, op)    # gate above the voxel (0.5)
    assert refused(h, rp, 100, 0, pp, 3, 0, 0.0, op)
    assert refused(h, rp, 100, 0, pp, 3, 0, -0.25, op)
    assert refused(h, rp, 100, 0, pp, 3, 0, float("nan"), op)
    assert refused(h, rp, 100, 0, pp, 3, 0, float("inf"), op)
    assert refused(h, rp, 100, 0, pp, 0, 0, 0.5, op)           # C < 1
    assert refused(h, rp, 100, 0, pp, (1 << 20) + 1, 0, 0.5, op)
    assert refused(h, rp, -1, 0, pp, 3, 0, 0.5, op)            # n < 0
    assert refused(h, None, 100, 0, pp, 3, 0, 0.5, op)         # NULL rows with n > 0
    assert refused(h, rp, 100, 0, None, 3, 0, 0.5, op)         # NULL poses
    assert L.svnicp_map_score_poses(None, rp, 100, 0, pp, 3, 0, 0.5, op) == INVALID
    assert L.svnicp_map_score_poses(h, None, 0, 0, pp, 3, 0, 0.5, op) == 0     # n == 0 needs no rows
    assert out.tolist() == [[0.0, 0.0, 0.0, 0.25]] * 3
    empty = pl.DeviceVoxelHashMap(0.5, 100.0, 20, device=0)
    assert L.svnicp_map_scores_devptr(empty._h) is None        # NULL before a scoring
    assert empty.score_poses(rows, P, 0.5).tolist() == [[0.0, 0.0, 0.0, 0.25]] * 3      # an empty map: nothing is located
    assert empty.scores_ptr != 0
    empty.close()


# ------------------------------------------------------------------------------------------------ 9. the grid search
def test_grid_search_on_the_device_agrees_with_the_host(pl, drive):
    dm, _ = drive
    _, nodes, zero, poses, true_node = ms.grid_search()
    want = ms.grid_host_scores(0.5)
    got = dm.score_poses(ms.drive_scan(4)[0], poses, 0.5)
    ms.assert_scores_match(got, want)
    assert pl.seed_from_scores(got, nodes, 1)[2][0] == true_node == pl.seed_from_scores(want, nodes, 1)[2][0]


# ------------------------------------------------------------------------------------------------ 10. / 11. the pipeline
def _drive_truth(sc, k):
    """The six-scan drive of tests/test_voxel_map_gpu.py; from scan 3 on the true pose is off the constant-velocity track by JUMP."""
    t = np.array([0.0, 0.0, 0.05 * k])
    yaw = np.radians(0.3 * k)
    if k >= 3:
        t = t + ms.JUMP[:3]
        yaw += ms.JUMP[5]
    return ms.pose(sc.rot_zyx(0.0, 0.0, yaw), t)


@pytest.fixture(scope="module")
def jump_scans(hip):
    sc = hip.scans
    scene = sc.make_scene()
    out = []
    for k in range(6):
        T = _drive_truth(sc, k)
        out.append((T, sc.lidar_scan(scene, T[:3, :3], T[:3, 3], 32768, stream=900 + k)))
    return out


def _run(hip, pl, scans, **kw):
    cfg = pl.PipelineConfig(min_range=1.0, max_range=80.0, voxel_size=0.5, map_voxel_size=0.5, map_voxel_max_points=20, map_range=100.0,
                            particle_count=32, seed=5,
                            solver=hip.SteinICPParam(iterations=20, lr=1.0, max_dist=1.0, KNN_count=50, SVN_full_grad=False), **kw)
    pipe = pl.RegistrationPipeline(cfg, device=0)
    return pipe, [pipe.process_scan(pts, stamp=0.1 * k) for k, (_, pts) in enumerate(scans)]


def _errors(pl, T, E):
    return float(np.linalg.norm(T[:3, 3] - E[:3, 3])), float(np.linalg.norm(pl.so3_log(T[:3, :3].T @ E[:3, :3])))


def _nearest_node(pl, prediction, truth):
    """Index of the grid node nearest the true pose, in the correction coordinates of the grid around `prediction`."""
    D = np.linalg.inv(prediction) @ truth
    x = np.concatenate([D[:3, 3], pl.so3_log(D[:3, :3])])
    idx = 0
    for e, s, v in zip(ms.GRID_EXTENT, ms.GRID_STEP, x):
        m = int(np.floor(e / s + 1e-9)) if e else 0
        k = int(np.clip(np.round(v / s), -m, m)) if m else 0
        idx = idx * (2 * m + 1) + (k + m)
    return idx


def test_pipeline_seeded_with_the_best_node_recovers_a_jump(hip, pl, jump_scans, monkeypatch):
    """The grid is an input, not a tolerance: at its step of 0.5 m / 2.5 degrees the solver does converge from the nearest node
    (measured at scan 3: 0.016 m and 1.8 mrad from the truth; the run without seeding, printed next to it and not asserted,
    ends 0.90 m and 68 mrad off).  The bounds are those tests/test_pipeline_gpu.py asserts for this scene."""
    grid =(ms.GRID_EXTENT, ms.GRID_STEP)
    runs = {}
    for gpu_map in (False, True):
        _, runs[gpu_map] = _run(hip, pl, jump_scans, gpu_map=gpu_map, seed_grid=grid, seed_mode="best")
    # without seeding no new call is made: the scoring is made to raise, and the drive still runs
    def boom(*a, **k):
        raise AssertionError("score_poses called although seed_grid is None")
    monkeypatch.setattr(pl.DeviceVoxelHashMap, "_score_poses", boom)
    monkeypatch.setattr(pl.VoxelHashMap, "score_poses", boom)
    _, plain = _run(hip, pl, jump_scans, gpu_map=True)
    assert all(r.seed is None for r in plain)
    truth = [T for T, _ in jump_scans]
    for k in range(1, 6):
        r = runs[True][k]
        et, er = _errors(pl, truth[k], r.pose)
        pt, pr = _errors(pl, truth[k], plain[k].pose)
        print(f"scan {k}: seeded node {r.seed['index']} cost {r.seed['cost']:.4f} (zero correction {r.seed['cost_zero']:.4f}) "
              f"error {et:.4f} m {er:.5f} rad | unseeded error {pt:.4f} m {pr:.5f} rad")
    for gpu_map in (False, True):
        r3 = runs[gpu_map][3]
        assert r3.seed["index"] == _nearest_node(pl, r3.seed["prediction"], truth[3])
        assert np.array_equal(r3.initial_guess, r3.seed["prediction"] @ pl.correction_to_pose(r3.seed["correction"]))
        et, er = _errors(pl, truth[3], r3.pose)
        assert et < 0.05 and er < 0.01, (gpu_map, et, er)
    dev, host = (np.array([r.pose for r in runs[g]]) for g in (True, False))
    assert np.allclose(dev, host, rtol=0, atol=1e-9)
    assert runs[True][0].seed is None and runs[False][0].seed is None          # scan 0 seeds the map: nothing to score against
    assert [r.seed["index"] for r in runs[True][1:]] == [r.seed["index"] for r in runs[False][1:]]


def test_unseeded_pipeline_is_unchanged(hip, pl, jump_scans):
    """seed_grid=None: the drive is bit for bit that of a configuration that never heard of seeding -- the defaults are the
    same object state, the particle stream is drawn identically, and ScanResult.seed stays None."""
    _, a = _run(hip, pl, jump_scans[:4], gpu_map=True)
    _, b = _run(hip, pl, jump_scans[:4], gpu_map=True, seed_grid=None, seed_gate=0.0, seed_mode="best")
    assert all(x.pose.tobytes() == y.pose.tobytes() for x, y in zip(a, b))
    assert all(x.seed is None for x in a + b)


def test_pipeline_seeded_with_the_top_nodes(hip, pl, jump_scans, monkeypatch):
    handed = []
    real = hip.SVNICP.add_cloud_device_target

    def spy(self, new_cloud, target_devptr, M, init_pose):
        handed.append(np.array(init_pose, float))
        return real(self, new_cloud, target_devptr, M, init_pose)

    monkeypatch.setattr(hip.SVNICP, "add_cloud_device_target", spy)
    pipe, res = _run(hip, pl, jump_scans[:4], gpu_map=True, seed_grid=(ms.GRID_EXTENT, ms.GRID_STEP), seed_mode="top")
    nodes, zero = pipe.cfg.seed_nodes()
    assert len(handed) == 3
    for k in (1, 2, 3):
        r = res[k]
        assert np.array_equal(r.initial_guess, r.seed["prediction"]) and not r.seed["correction"].any()   # the mean stays the prediction
        order = r.seed["nodes"]                                # the nodes reported are the particles the solver was given
        assert order.shape == (32,) and order[0] == r.seed["index"]
        assert np.array_equal(handed[k - 1], nodes[order].T)
    # scan 3 jumped: the best node is the one nearest the truth, and it is a particle
    assert res[3].seed["index"] == _nearest_node(pl, res[3].seed["prediction"], jump_scans[3][0])
    # the order is (cost, index): recompute the scoring of scan 3 against a map rebuilt from the results
    twin = pl.DeviceVoxelHashMap(0.5, 100.0, 20, device=0)
    for k in range(3):
        cropped = pl.crop_pointcloud(jump_scans[k][1], 1.0, 80.0)[0]
        to_map = pl.downsample_uniform(cropped, 0.25)
        twin.add_pointcloud(to_map if k == 0 else pl.downsample_uniform(to_map, 0.75), res[k].pose)
    to_map = pl.downsample_uniform(pl.crop_pointcloud(jump_scans[3][1], 1.0, 80.0)[0], 0.25)
    scores = twin.score_poses(pl.downsample_uniform(to_map, 0.75), pl.correction_poses(res[3].seed["prediction"], nodes), 0.5)
    want = np.lexsort((np.arange(729), scores[:, 3]))[:32]
    assert np.array_equal(res[3].seed["nodes"], want)
    assert res[3].seed["cost_zero"] == scores[zero, 3] and res[3].seed["cost"] == scores[want[0], 3]
    twin.close()


def test_pipeline_seeded_with_device_preprocessing_uploads_nothing_more(hip, pl, jump_scans):
    """gpu_prep: the rows scored are the solver cloud already in HBM (source_f32_ptr); the scan is not uploaded a second time."""
    grid = (ms.GRID_EXTENT, ms.GRID_STEP)
    plain_pipe, _ = _run(hip, pl, jump_scans[:4], gpu_map=True, gpu_prep=True)
    pipe, res = _run(hip, pl, jump_scans[:4], gpu_map=True, gpu_prep=True, seed_grid=grid, seed_mode="best")
    assert pipe.bytes_h2d == plain_pipe.bytes_h2d
    truth = jump_scans[3][0]
    assert res[3].seed["index"] == _nearest_node(pl, res[3].seed["prediction"], truth)
    et, er = _errors(pl, truth, res[3].pose)
    assert et < 0.05 and er < 0.01, (et, er)
