"""Inputs shared by tests/test_map_score_cpu.py and tests/test_map_score_gpu.py (svnicp_map_score_poses): the
crafted map with exact quotients and its brute-force reference, the drive map with scan 4, the search grid of the issue, and the
comparison rule.  Everything is computed once and never modified."""
import functools

import numpy as np

import map_normals_cases as mn

ROWS_PER_WORKGROUP = 256          # kScoreRows of svn-icp_amd/csrc/map_score.hpp (documented in include/svnicp_hip.h)
GRID_EXTENT = (2.0, 2.0, 0.0, 0.0, 0.0, np.radians(10.0))
GRID_STEP = (0.5, 0.5, 0.0, 0.0, 0.0, np.radians(2.5))
JUMP = np.array([1.0, -0.5, 0.0, 0.0, 0.0, np.radians(5.0)])    # = node (k_x, k_y, k_yaw) = (+2, -1, +2) of the grid


def _pkg():
    import __graft_entry__ as graft
    return graft.load_package()


def pose(R=np.eye(3), t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def rot90(axis, quarter_turns):
    """Rotation by a multiple of 90 degrees about a coordinate axis: entries exactly 0 and +-1."""
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][quarter_turns % 4]
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


# ------------------------------------------------------------------------------------------------ the crafted case
ISOLATED = np.array([8.5, 8.5, 8.5])            # a stored point with nothing near it: rows at exactly the gate from it


def crafted_gates(voxel):
    return [voxel, voxel / 2, 2.0 ** -6]


@functools.lru_cache(maxsize=None)
def crafted(voxel):
    """-> (stored cloud float32 [m,3], rows float32 [n,3], poses [C,4,4]).  Every coordinate is a multiple of 1/64, points sit
    on both sides of zero (the double-width voxel 0 of the truncate-toward-zero index is in play), poses are the identity,
    translations by multiples of 1/64 and rotations by multiples of 90 degrees: every transformed coordinate and every
    quotient by the voxel (1.0 or 0.5) is exact in float32, every d2 and every sum exact in float64."""
    rng = np.random.default_rng(7)
    stored = rng.integers(-3 * 64, 3 * 64, size=(500, 3)) / 64.0
    stored[:40] = rng.integers(-20, 20, size=(40, 3)) / 64.0        # a cluster inside voxel 0 (more than 20 points: the cap cuts)
    stored = np.concatenate([stored, [ISOLATED]], 0)
    rows = rng.integers(-int(3.5 * 64), int(3.5 * 64), size=(300, 3)) / 64.0
    exact = []
    for g in crafted_gates(voxel):                                   # d2 == thr2 exactly: located, NOT an inlier
        exact += [ISOLATED + [g, 0, 0], ISOLATED - [0, g, 0]]
    exact += [ISOLATED + [1 / 64, 1 / 64, 0], ISOLATED]             # just inside every gate but 2^-6 | a distance of zero
    rows = np.concatenate([rows, np.array(exact)], 0)
    poses = [pose(), pose(t=(1 / 64, -3 / 64, 5 / 64)), pose(t=(-65 / 64, 0.5, 2.0)), pose(rot90(2, 1)), pose(rot90(0, 2), (0.25, 0, -1 / 64)),
             pose(rot90(1, 3), (-1.0, 1.0, 33 / 64)), pose(rot90(2, 2) @ rot90(0, 1))]
    return stored.astype(np.float32), rows.astype(np.float32), np.array(poses)


N_EXACT_ROWS = 8   # the rows `crafted` appends: 2 per gate at exactly the gate, then the near one and the coincident one


def crafted_host_map(voxel, max_points):
    pl = _pkg().pipeline
    hm = pl.VoxelHashMap(voxel, 1e9, max_points)
    hm.add_pointcloud(crafted(voxel)[0], np.eye(4))
    return hm


def brute_force(hm, rows, poses, gate):
    """The contract by brute force over the WHOLE map (exact-quotient inputs only): the nearest stored point of the whole map
    decides the inlier, voxel adjacency by comparing every stored point's voxel decides `located`."""
    pl = _pkg().pipeline
    stored = hm.get_map()                                            # float64 [m,3], the points the map kept
    vs = hm.voxel_size
    sv = np.trunc(stored / vs)
    thr2 = gate * gate
    out = np.zeros((len(poses), 4))
    n = rows.shape[0]
    for ci, T in enumerate(poses):
        c = pl.transform_f32(rows, T).astype(np.float64)
        cv = np.trunc(c / vs)
        d = c[:, None, :] - stored[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        near = np.all(np.abs(cv[:, None, :] - sv[None, :, :]) <= 1, axis=2)
        located = near.any(axis=1)
        dmin = d2.min(axis=1)
        inl = dmin < thr2
        assert not (inl & ~located).any()                            # gate <= voxel: the nearest point within the gate is in the block
        s = 0.0
        for v in dmin[inl]:
            s += v
        out[ci] = (located.sum(), inl.sum(), s, (s + (n - inl.sum()) * thr2) / n)
    return out


# ------------------------------------------------------------------------------------------------ the drive
@functools.lru_cache(maxsize=None)
def drive_scan(k=4):
    """-> (rows float32 [n,3]: the 1.5-voxel sampling the solver would register, true pose 4x4) of scan k of the drive."""
    _, source, T = mn._drive_scan(k)
    return np.ascontiguousarray(source, np.float32), T


def drive_steps():
    """(voxel, max_points, max_range, [(cloud, pose), ...]) of the four-scan `drive` map of tests/map_normals_cases.py."""
    return mn.case_inputs("drive")


@functools.lru_cache(maxsize=None)
def drive_rows(n):
    """n rows for the chunk-boundary test: scan 4's rows, continued with scan 5's when n asks for more."""
    rows = np.concatenate([drive_scan(4)[0], drive_scan(5)[0]], 0)
    assert n <= rows.shape[0]
    return np.ascontiguousarray(rows[:n])


@functools.lru_cache(maxsize=None)
def drive_poses(count, seed=0):
    """`count` random perturbations of scan 4's true pose (up to 0.6 m and 3 degrees), [count, 4, 4]."""
    pl = _pkg().pipeline
    rng = np.random.default_rng(100 + seed)
    T = drive_scan(4)[1]
    x = rng.uniform(-1, 1, size=(count, 6)) * [0.6, 0.6, 0.2, 0.02, 0.02, 0.05]
    x[0] = 0.0
    return np.array([T @ pl.correction_to_pose(v) for v in x])


@functools.lru_cache(maxsize=None)
def grid_search():
    """The issue's grid search: (centre pose, corrections [729,6], zero index, node poses [729,12], index of the true node).
    The centre is displaced from scan 4's true pose so that the truth is the node JUMP."""
    pl = _pkg().pipeline
    nodes, zero = pl.correction_grid(GRID_EXTENT, GRID_STEP)
    T = drive_scan(4)[1]
    centre = T @ np.linalg.inv(pl.correction_to_pose(JUMP))
    true_node = int(np.argmin(np.abs(nodes - JUMP).sum(axis=1)))
    assert np.allclose(nodes[true_node], JUMP, atol=1e-12)
    return centre, nodes, zero, pl.correction_poses(centre, nodes), true_node


@functools.lru_cache(maxsize=None)
def grid_host_scores(gate=0.5):
    return mn.host_map("drive").score_poses(drive_scan(4)[0], grid_search()[3], gate)


# ------------------------------------------------------------------------------------------------ the comparison rule
def assert_scores_match(got, want, what=""):
    """Device against the restatement: located and inliers EXACTLY equal; sum_d2 and cost within 1e-12 relative (the two add
    a few thousand non-negative terms in different orders)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got[:, :2], want[:, :2]), (what, np.flatnonzero((got[:, :2] != want[:, :2]).any(axis=1))[:8])
    for col in (2, 3):
        err = np.abs(got[:, col] - want[:, col])
        assert np.all(err <= 1e-12 * np.abs(want[:, col])), (what, col, float(err.max()))
