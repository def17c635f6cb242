"""Inputs shared by tests/test_map_normals_cpu.py and tests/test_map_normals_gpu.py: each map is described by the clouds
and poses that build it (so the host map and the device map can be fed the same sequence), and the numpy restatement of its
normals (tests/map_normals_reference.py) is computed once per (case, normal_k) and never modified."""
import functools

import numpy as np

import map_normals_reference as mr

SHIFT = np.array([3000.0, -2000.0, 50.0])
DRIVE_VOXEL, DRIVE_MAX_POINTS = 0.5, 20
DENSE = {"dense65": (65, 6000), "dense130": (130, 9000), "dense256": (256, 12000)}      # name -> (max_points, points drawn)


def _pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def drive_pose(sc, k):
    """True pose of scan k of tests/test_pipeline_gpu.py's drive: climb 0.05 m and yaw 0.3 degrees per scan."""
    return _pose(sc.rot_zyx(0.0, 0.0, np.radians(0.3 * k)), np.array([0.0, 0.0, 0.05 * k]))


@functools.lru_cache(maxsize=None)
def _drive_scan(k):
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pl, sc = pkg.pipeline, pkg.scans
    T = drive_pose(sc, k)
    pts = sc.lidar_scan(sc.make_scene(), T[:3, :3], T[:3, 3], 32768, stream=300 + k)
    cropped, _ = pl.crop_pointcloud(pts, 1.0, 80.0)
    to_map = pl.downsample_uniform(cropped, 0.5 * DRIVE_VOXEL)
    source = pl.downsample_uniform(to_map, 1.5 * DRIVE_VOXEL)
    return to_map, source, T


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """-> (voxel, max_points, max_range, [(cloud float32 [n,3], pose 4x4), ...])"""
    if name in ("drive", "drive_shifted"):
        # four scans at their true poses: seeded with the 0.5-voxel sampling, updated with the 1.5-voxel one, as the pipeline does
        off = SHIFT if name == "drive_shifted" else np.zeros(3)
        steps = []
        for k in range(4):
            to_map, source, T = _drive_scan(k)
            T = T.copy()
            T[:3, 3] += off
            steps.append(((to_map if k == 0 else source).astype(np.float32), T))
        return DRIVE_VOXEL, DRIVE_MAX_POINTS, 100.0, steps
    if name in ("uniform64", "uniform3"):
        # up to 27 * 64 = 1728 candidates per block (measured maximum 1542), 64 degenerate rows, ties among duplicates | a small cut
        ext, voxel, mp = (4.0, 1.0, 64) if name == "uniform64" else (3.0, 0.5, 3)
        rng = np.random.default_rng(64 if name == "uniform64" else 3)
        cloud = rng.uniform(-ext, ext, size=(20000, 3)).astype(np.float32)
        cloud[:2000] = cloud[0]
        return voxel, mp, 1e9, [(cloud, np.eye(4))]
    if name == "lattice":
        # distinct points at equal distances: the tie rule decides the neighbour set; also the double-width voxel 0 and the cut
        g = np.arange(-40, 40)
        nodes = np.stack(np.meshgrid(g, g, np.arange(2), indexing="ij"), -1).reshape(-1, 3)
        rng = np.random.default_rng(11)
        nodes = nodes[rng.random(nodes.shape[0]) < 0.5]
        rng.shuffle(nodes)
        return 1.0, 20, 1e9, [((nodes * 0.25).astype(np.float32), np.eye(4))]
    if name in DENSE:
        # voxels of more than 64 points (the second 64-point block of k_map_normals) up to max_points itself, filled over three
        # calls; blocks from a few dozen candidates (fewer than normal_k 64: no normal) to several 1024-candidate tiles
        mp, n = DENSE[name]
        rng = np.random.default_rng(mp)
        cloud = (rng.normal(size=(n, 3)) * [1.2, 1.2, 0.7]).astype(np.float32)
        cloud = cloud[np.abs(cloud).max(axis=1) < 2.9]
        cloud[:70] = cloud[0]
        return 1.0, mp, 1e9, [(part, np.eye(4)) for part in np.array_split(cloud, 3)]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def host_map(name):
    import __graft_entry__ as graft
    pl = graft.load_package().pipeline
    voxel, mp, max_range, steps = case_inputs(name)
    hm = pl.VoxelHashMap(voxel, max_range, mp)
    for cloud, T in steps:
        hm.add_pointcloud(cloud, T)
    if name in DENSE:      # what makes these cases a test of a voxel's second block of 64 points
        sizes = np.array([len(v) for v in hm._vox.values()])
        assert sizes.max() == mp and int((sizes > 64).sum()) >= 10, (name, sizes.max(), int((sizes > 64).sum()))
    return hm


@functools.lru_cache(maxsize=None)
def _neighbourhoods(name):
    return mr.neighbourhoods(host_map(name)._vox)


@functools.lru_cache(maxsize=None)
def reference(name, normal_k):
    return mr.map_normals(host_map(name)._vox, normal_k, _neighbourhoods(name))


def cut_query(name):
    """A range query whose radius cuts the map: (pose, radius).  Rows near the cut have neighbours outside the selection."""
    hm = host_map(name)
    first = np.array([np.asarray(v[0], np.float64) for v in hm._vox.values()])
    centre = np.median(first, axis=0)
    r = float(np.median(np.linalg.norm(first - centre, axis=1)))
    return _pose(np.eye(3), centre), r


GAP_FLOOR = 1e-3       # normals are compared where (lambda1 - lambda0) / lambda2 >= this (tests/test_plane_gpu.py's floor)
THRESHOLD_BAND = 1e-9  # flags are compared where |lambda1 - MIN_RATIO * lambda2| > this * lambda2


def left_out(ref):
    """(rows whose flag is not compared, rows whose normal is not compared) of a restatement."""
    l2 = np.where(ref.lam[:, 2] > 0, ref.lam[:, 2], 1.0)
    near = (ref.lam[:, 2] > 0) & (np.abs(ref.lam[:, 1] - mr.MIN_RATIO * ref.lam[:, 2]) <= THRESHOLD_BAND * l2)
    low_gap = ref.valid & ((ref.lam[:, 1] - ref.lam[:, 0]) / l2 < GAP_FLOOR)
    return near, low_gap
