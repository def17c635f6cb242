"""Scoring candidate poses against the voxel map, host side: the numpy restatement
(pipeline.VoxelHashMap.score_poses) against a brute-force search of the whole map on exact-quotient inputs, the C++ restatement
(registration_pipeline.hpp, tests/map_score_driver.cpp) bit for bit against the numpy one, the grid and seed helpers, the
declarations, and the grid search on the drive map."""
import os
import struct
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import map_normals_cases as mn
import map_score_cases as ms

pkg = ge.load_package()
pl = pkg.pipeline
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ (a) against brute force
@pytest.mark.parametrize("voxel", [1.0, 0.5])
@pytest.mark.parametrize("max_points", [3, 20])
def test_restatement_equals_brute_force_on_exact_quotients(voxel, max_points):
    _, rows, poses = ms.crafted(voxel)
    hm = ms.crafted_host_map(voxel, max_points)
    assert any(k[0] == 0 for k in hm._vox) and any(k[0] < 0 for k in hm._vox)          # voxel 0 and both sides of it
    for gate in ms.crafted_gates(voxel):
        got = hm.score_poses(rows, poses, gate)
        want = ms.brute_force(hm, rows, poses, gate)
        assert np.array_equal(got, want), (gate, got, want)                             # all four fields, exactly
        assert 0 < got[0, 1] < got[0, 0] <= rows.shape[0]


@pytest.mark.parametrize("voxel", [1.0, 0.5])
def test_a_pair_at_exactly_the_gate_is_located_but_no_inlier(voxel):
    _, rows, _ = ms.crafted(voxel)
    hm = ms.crafted_host_map(voxel, 20)
    exact = rows[-ms.N_EXACT_ROWS:]
    for gi, gate in enumerate(ms.crafted_gates(voxel)):
        thr2 = gate * gate
        for r in exact[2 * gi:2 * gi + 2]:                                             # d2 == thr2: the comparison is strict
            assert hm.score_poses(r[None], np.eye(4)[None], gate)[0].tolist() == [1.0, 0.0, 0.0, thr2]
        near = hm.score_poses(exact[6:7], np.eye(4)[None], gate)[0]                    # d2 = 2 / 4096
        assert near.tolist() == ([1.0, 1.0, 2 / 4096, 2 / 4096] if 2 / 4096 < thr2 else [1.0, 0.0, 0.0, thr2])
        assert hm.score_poses(exact[7:8], np.eye(4)[None], gate)[0].tolist() == [1.0, 1.0, 0.0, 0.0]


def test_refusals_and_empties_of_the_restatement():
    hm = ms.crafted_host_map(1.0, 20)
    rows = ms.crafted(1.0)[1]
    for gate in (1.0 + 1e-9, 0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            hm.score_poses(rows, np.eye(4)[None], gate)
    with pytest.raises(ValueError):
        hm.score_poses(rows, np.zeros((0, 12)), 0.5)
    bad = np.eye(4)[None].repeat(2, 0)
    bad[1, 0, 3] = np.nan                                                              # never an error: nothing is located
    far = ms.pose(t=(1e6, 0, 0))[None]
    out = hm.score_poses(rows, np.concatenate([bad, far]), 0.5)
    assert out[1].tolist() == [0.0, 0.0, 0.0, 0.25] and out[2].tolist() == [0.0, 0.0, 0.0, 0.25] and out[0, 0] > 0
    assert hm.score_poses(np.zeros((0, 3), np.float32), bad, 0.5).tolist() == [[0.0, 0.0, 0.0, 0.25]] * 2
    assert pl.VoxelHashMap(1.0, 1e9, 20).score_poses(rows, bad, 0.5).tolist() == [[0.0, 0.0, 0.0, 0.25]] * 2
    odd = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [3e6, 0, 0], [0.5, 0.5, 0.5]], np.float32)
    assert hm.score_poses(odd, np.eye(4)[None], 1.0)[0, 0] == hm.score_poses(odd[3:], np.eye(4)[None], 1.0)[0, 0]


# ------------------------------------------------------------------------------------------------ (b) the C++ restatement
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("score") / "map_score_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "svn-icp_amd", "host"), os.path.join(ROOT, "tests", "map_score_driver.cpp"), "-o", out])
    return out


def _cpp(driver, tmp_path, voxel, max_points, steps, rows, poses, gate, map_range=1e9):
    rows = np.ascontiguousarray(rows, np.float32)
    P = pl.pose_rows(poses)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<ddidi", voxel, map_range, max_points, gate, len(steps)))
        for cloud, T in steps:
            cloud = np.ascontiguousarray(cloud, np.float32)
            f.write(np.ascontiguousarray(np.asarray(T, float)[:3, :3]).tobytes()); f.write(np.ascontiguousarray(np.asarray(T, float)[:3, 3]).tobytes())
            f.write(struct.pack("<i", cloud.shape[0])); f.write(cloud.tobytes())
        f.write(struct.pack("<i", rows.shape[0])); f.write(rows.tobytes())
        f.write(struct.pack("<i", P.shape[0])); f.write(P.tobytes())
    r = subprocess.run([driver, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(tmp_path / "out.bin", np.float64).reshape(-1, 4)


@pytest.mark.parametrize("voxel,max_points", [(1.0, 3), (0.5, 20)])
def test_cpp_restatement_on_the_crafted_case(driver, tmp_path, voxel, max_points):
    stored, rows, poses = ms.crafted(voxel)
    odd = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -3e6]], np.float32)
    rows = np.concatenate([rows, odd], 0)
    bad = np.eye(4)[None].copy()
    bad[0, 1, 1] = np.nan
    poses = np.concatenate([poses, bad, ms.pose(t=(1e6, 0, 0))[None]], 0)
    hm = ms.crafted_host_map(voxel, max_points)
    for gate in ms.crafted_gates(voxel):
        want = hm.score_poses(rows, poses, gate)
        got = _cpp(driver, tmp_path, voxel, max_points, [(stored, np.eye(4))], rows, poses, gate)
        assert got.tobytes() == want.tobytes(), gate


def test_cpp_restatement_on_a_drive_step(driver, tmp_path):
    voxel, max_points, map_range, steps = ms.drive_steps()
    rows, _ = ms.drive_scan(4)
    poses = ms.drive_poses(12)
    want = mn.host_map("drive").score_poses(rows, poses, 0.5)
    got = _cpp(driver, tmp_path, voxel, max_points, steps, rows, poses, 0.5, map_range)
    assert want[0, 1] > 0.5 * rows.shape[0]                                            # the true pose: most rows are inliers
    assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------ (c) grid and seed helpers
def test_correction_grid_nodes_order_and_zero():
    nodes, zero = pl.correction_grid(ms.GRID_EXTENT, ms.GRID_STEP)
    assert nodes.shape == (729, 6) and zero == 364 and not nodes[zero].any()
    assert nodes[0].tolist() == [-2.0, -2.0, 0.0, 0.0, 0.0, -4 * np.radians(2.5)]
    assert nodes[1].tolist() == [-2.0, -2.0, 0.0, 0.0, 0.0, -3 * np.radians(2.5)]      # the last axis runs fastest
    assert nodes[9].tolist() == [-2.0, -1.5, 0.0, 0.0, 0.0, -4 * np.radians(2.5)]
    assert nodes[81].tolist() == [-1.5, -2.0, 0.0, 0.0, 0.0, -4 * np.radians(2.5)]     # x slowest
    assert nodes[-1].tolist() == [2.0, 2.0, 0.0, 0.0, 0.0, 4 * np.radians(2.5)]
    nodes, zero = pl.correction_grid((1.0, 0, 0, 0, 0, 0), (0.4, 0, 0, 0, 0, 0))       # m = floor(2.5) = 2
    assert nodes[:, 0].tolist() == [-0.8, -0.4, 0.0, 0.4, 0.8] and zero == 2
    nodes, zero = pl.correction_grid(np.zeros(6), np.zeros(6))                         # every axis fixed: the zero correction alone
    assert nodes.tolist() == [[0.0] * 6] and zero == 0
    nodes, zero = pl.correction_grid((0, 0, 0.3, 0, 0.1, 0), (1, 1, 0.1, 1, 0.1, -1))  # a step is not looked at where the extent is 0
    assert nodes.shape == (21, 6) and not nodes[zero].any()
    for ext, stp in (((1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0)), ((1, 0, 0, 0, 0, 0), (-0.5, 0, 0, 0, 0, 0)), ((-1, 0, 0, 0, 0, 0), (0.5,) * 6),
                     ((np.nan, 0, 0, 0, 0, 0), (0.5,) * 6), ((1, 1, 1, 1, 0, 0), (0.05,) * 6), ((1, 1, 1), (1, 1, 1))):
        with pytest.raises(ValueError):
            pl.correction_grid(ext, stp)                                               # 41^4 nodes > 2^20 among them


def test_seed_from_scores_orders_by_cost_then_index():
    nodes, _ = pl.correction_grid((1, 0, 0, 0, 0, 1), (0.5, 0, 0, 0, 0, 0.5))          # 25 nodes
    scores = np.zeros((25, 4))
    scores[:, 3] = 1.0
    scores[[17, 4, 9], 3] = 0.25                                                       # a three-way tie for the best
    scores[20, 3] = 0.5
    best, top, order = pl.seed_from_scores(scores, nodes, 6)
    assert order.tolist() == [4, 9, 17, 20, 0, 1]
    assert np.array_equal(best, nodes[4]) and np.array_equal(top, nodes[order])
    assert pl.seed_from_scores(scores, nodes, 1)[2].tolist() == [4]
    for P in (0, 26):
        with pytest.raises(ValueError):
            pl.seed_from_scores(scores, nodes, P)
    with pytest.raises(ValueError):
        pl.seed_from_scores(scores[:24], nodes, 1)


def test_correction_poses_compose_like_a_particle():
    guess = ms.drive_scan(4)[1] @ pl.correction_to_pose([0.3, -0.2, 0.1, 0.01, -0.02, 0.4])
    nodes, _ = pl.correction_grid((0.5, 0, 0, 0.1, 0, 0.2), (0.5, 0, 0, 0.1, 0, 0.1))
    P = pl.correction_poses(guess, nodes)
    for x, row in zip(nodes, P):
        T = guess @ pl.correction_to_pose(x)
        assert np.array_equal(row[:9].reshape(3, 3), T[:3, :3]) and np.array_equal(row[9:], T[:3, 3])
    assert np.array_equal(pl.pose_rows(np.array([guess]))[0], pl.correction_poses(guess, np.zeros((1, 6)))[0])


def test_pipeline_config_refuses_inconsistent_seed_fields():
    grid = (ms.GRID_EXTENT, ms.GRID_STEP)
    cfg = pl.PipelineConfig(seed_grid=grid, map_voxel_size=0.5)
    assert cfg.seed_mode == "best" and cfg.seed_gate == 0.0 and pl.PipelineConfig().seed_grid is None
    for kw in (dict(seed_mode="all"), dict(seed_grid=grid, seed_mode="top", particle_count=730), dict(seed_grid=grid, seed_gate=0.6, map_voxel_size=0.5),
               dict(seed_gate=-0.1), dict(seed_gate=float("nan")), dict(seed_grid=((1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0))),
               dict(seed_grid=((1, 1, 1, 1, 0, 0), (0.05,) * 6)), dict(seed_grid=(ms.GRID_EXTENT,))):
        with pytest.raises(ValueError):
            pl.PipelineConfig(**kw)
    pl.PipelineConfig(seed_grid=grid, seed_mode="top", particle_count=729)


# ------------------------------------------------------------------------------------------------ (d) the declarations
def test_header_and_binding_declare_the_scoring():
    txt = open(os.path.join(ROOT, "include", "svnicp_hip.h")).read()
    assert "#define SVNICP_MAP_SCORE_FIELDS 4" in txt and "#define SVNICP_ABI_VERSION 1\n" in txt
    names = pkg.binding.declared_symbols()
    assert "svnicp_map_score_poses" in names and "svnicp_map_scores_devptr" in names
    src = open(os.path.join(ROOT, "svn-icp_amd", "binding.py")).read()
    assert "L.svnicp_map_score_poses.argtypes" in src and "L.svnicp_map_scores_devptr.restype" in src
    assert len(pl.SCORE_FIELDS) == 4


# ------------------------------------------------------------------------------------------------ (e) the grid search
def test_grid_search_on_the_host_finds_the_true_node():
    """Mean truncated squared distance at gate 0.5 m: a feasibility probe measured 0.0327 at the true node and 0.0736 at the
    runner-up, 0.5 m away."""
    _, nodes, zero, _, true_node = ms.grid_search()
    scores = ms.grid_host_scores(0.5)
    best, top, order = pl.seed_from_scores(scores, nodes, 2)
    print(f"rows {ms.drive_scan(4)[0].shape[0]}, best node {order[0]} cost {scores[order[0], 3]:.4f}, runner-up {order[1]} cost "
          f"{scores[order[1], 3]:.4f} at {np.round(top[1] - top[0], 3).tolist()}, zero correction cost {scores[zero, 3]:.4f}")
    assert order[0] == true_node and np.array_equal(best, nodes[true_node])
