"""Crafted cases of the Gaussian pose prior (test infrastructure): particle sets, means, information matrices, 22-sum records,
the degenerate plane scene and the corridor of the pipeline test.  Everything is generated from fixed seeds."""
import numpy as np

SIGMA = 0.02                                   # the degenerate scene's prior: Lambda = diag(1 / 0.02^2)
SCENE_MU = np.array([0.05, 0.02, 0.0, 0.0, 0.0, 0.005])
SCENE_START = np.array([0.2, -0.1, 0.05, 0.01, -0.01, 0.02])
SCENE_K, SCENE_ITERS = 8, 15


# ---------------- information matrices ----------------
def lam_diag():
    return np.diag([2500.0, 2500.0, 400.0, 1e4, 1e4, 4e4])


def lam_full():
    """SPD with large off-diagonals: A A^T of a fixed dense matrix plus a small ridge."""
    rng = np.random.default_rng(11)
    A = rng.uniform(-1.0, 1.0, (6, 6)) + 0.9
    L = A @ A.T * 50.0 + 0.5 * np.eye(6)
    return 0.5 * (L + L.T)


def lam_rank1():
    v = np.zeros(6); v[5] = 1.0           # yaw only
    return 3e4 * np.outer(v, v)


def lam_zero():
    return np.zeros((6, 6))


def lam_huge():
    return np.diag([1e12] * 6) + 1e11 * (np.ones((6, 6)) - np.eye(6)) * 0.5


LAMBDAS = {"diag": lam_diag, "full": lam_full, "rank1": lam_rank1, "zero": lam_zero, "huge": lam_huge}
MU_NONZERO = np.array([0.05, -0.02, 0.03, 0.1, -0.2, 0.05])


# ---------------- particle sets ----------------
def particles(P, seed=5):
    """[6][P]: the first columns are the crafted rotation vectors — exactly zero, both sides of the series threshold 1e-2,
    2.5 rad — the rest a box of +-0.3 m, +-0.05 rad."""
    rng = np.random.default_rng(seed + P)
    x = np.concatenate([rng.uniform(-0.3, 0.3, (3, P)), rng.uniform(-0.05, 0.05, (3, P))])
    crafted = [np.zeros(3), np.array([3e-3, -4e-3, 0.0]), np.array([0.0, 1.2e-2, 1.6e-2]), np.array([1.5, -2.0, 0.0]),
               np.array([0.0, 0.0, 9.9e-3]), np.array([0.0, 1.01e-2, 0.0])]
    for i, r in enumerate(crafted[:P]):
        x[3:, i] = r
    if P >= 1:
        x[:3, 0] = 0.0      # with mu = 0: e exactly 0 for particle 0
    return np.ascontiguousarray(x)


def sums(P, seed=3):
    """[P][22] plausible Gauss-Newton sums: 40 unit-scale points with errors of 5 cm, unit weights (stein_iter.hip's layout)."""
    rng = np.random.default_rng(seed + 7 * P)
    out = np.zeros((P, 22))
    for p in range(P):
        s = rng.uniform(-1.0, 1.0, (40, 3)) * np.array([5.0, 5.0, 1.0])
        e = rng.normal(0.0, 0.05, (40, 3))
        out[p, 0] = 40.0
        out[p, 1:4] = s.sum(0)
        S = s.T @ s
        out[p, 4:10] = S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]
        out[p, 10:13] = e.sum(0)
        out[p, 13:22] = (e.T @ s).reshape(9)
    return out


def plane_records(P, seed=9):
    """[P][42]: a symmetric positive H with 1e-6 on the diagonal, and b (k_plane_finalize's layout)."""
    rng = np.random.default_rng(seed + P)
    out = np.zeros((P, 42))
    for p in range(P):
        j = rng.uniform(-1.0, 1.0, (30, 6))
        H = j.T @ j
        H = 0.5 * (H + H.T) + 1e-6 * np.eye(6)
        out[p, :36] = H.reshape(36)
        out[p, 36:] = j.T @ rng.normal(0.0, 0.05, 30)
    return out


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def far_mean():
    """R0 != I with t0 a kilometre away."""
    R0 = rot_z(0.7) @ np.array([[1.0, 0.0, 0.0], [0.0, np.cos(0.2), -np.sin(0.2)], [0.0, np.sin(0.2), np.cos(0.2)]])
    T = np.eye(4); T[:3, :3] = R0; T[:3, 3] = [1000.0, -400.0, 12.0]
    return T


# (name, P, options, Lambda, mean, far initial mean, particle with a NaN pose or None, plane record)
KERNEL_CASES = [
    ("p1", 1, (), "full", MU_NONZERO, False, None, False),
    ("p1_mu0", 1, (), "diag", np.zeros(6), False, None, False),
    ("p2", 2, (), "full", MU_NONZERO, False, None, False),
    ("p8_mu0_diag", 8, (), "diag", np.zeros(6), False, None, False),
    ("p8_rank1", 8, (), "rank1", MU_NONZERO, False, None, False),
    ("p8_zero", 8, (), "zero", MU_NONZERO, False, None, False),
    ("p8_huge", 8, (), "huge", np.zeros(6), False, None, False),
    ("p8_far", 8, (), "full", MU_NONZERO, True, None, False),
    ("p8_nan", 8, (), "full", MU_NONZERO, False, 3, False),
    ("p8_fused", 8, (("update", "fused"),), "full", np.zeros(6), False, None, False),
    ("p8_plane", 8, (), "full", MU_NONZERO, False, None, True),
    ("p63", 63, (), "full", MU_NONZERO, False, None, False),
    ("p64", 64, (), "diag", np.zeros(6), False, None, False),
    ("p65", 65, (), "full", MU_NONZERO, True, None, False),
    ("p128", 128, (), "full", np.zeros(6), False, None, False),
    ("p130", 130, (), "full", MU_NONZERO, False, 129, False),
]


# ---------------- the degenerate scene: a plane seen from above ----------------
def plane_scene():
    """target: z = 0, a 32 x 32 grid at 0.25 m with normals (0, 0, 1); source: the central 16 x 16 patch.  Only z, roll and
    pitch are constrained by the data."""
    g = (np.arange(32) - 15.5) * 0.25
    X, Y = np.meshgrid(g, g, indexing="ij")
    tgt = np.stack([X.ravel(), Y.ravel(), np.zeros(X.size)], 1)
    gs = (np.arange(16) - 7.5) * 0.25
    Xs, Ys = np.meshgrid(gs, gs, indexing="ij")
    src = np.stack([Xs.ravel(), Ys.ravel(), np.zeros(Xs.size)], 1)
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (tgt.shape[0], 1))
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt), np.ascontiguousarray(nrm)


def scene_lambda():
    return np.eye(6) / SIGMA ** 2


def scene_particles(P, seed=21):
    """[6][P]: P = 1 the scene's start; else a box of +-0.3 m, +-0.012 rad around zero (the width initialize_particles draws)."""
    if P == 1:
        return np.ascontiguousarray(SCENE_START.reshape(6, 1))
    rng = np.random.default_rng(seed)
    half = np.array([0.3, 0.3, 0.3, 0.012, 0.012, 0.012])[:, None]
    return np.ascontiguousarray(rng.uniform(-1.0, 1.0, (6, P)) * half)


# ---------------- the corridor: floor and two walls, no end walls ----------------
# PipelineConfig.prior_sigma / prior_point_sigma of the pipeline test: Lambda = 400 per m^2 and 1e4 per rad^2, as stiff along the
# corridor as the data is across it.  The two pipelines' host stages differ in the last bits of what they hand the solver, and a
# direction answers a difference in b with 1 / (H + Lambda): measured with Lambda = 4 (point sigma 0.1) the two poses were
# 2.2e-9 apart along x at the third scan where the other entries agreed to 4e-11; with Lambda = 400 they agree to 1e-14.
CORRIDOR_SIGMA = (0.05, 0.05, 0.05, 0.01, 0.01, 0.01)
CORRIDOR_POINT_SIGMA = 1.0


def corridor_scan(k, n=9000):
    """Scan k (float32 [n][3], sensor frame) in a corridor along x: floor z = -1.5, walls y = +-2 up to z = 1, seen within
    +-15 m of the sensor along x.  Every scan draws its own points uniformly on the three surfaces, so nothing in it says where
    along the corridor the sensor stands: x is the direction the data does not constrain."""
    rng = np.random.default_rng(4000 + k)
    x = rng.uniform(-15.0, 15.0, n)
    which = rng.integers(0, 3, n)
    u = rng.uniform(0.0, 1.0, n)
    y = np.where(which == 0, -2.0 + 4.0 * u, np.where(which == 1, -2.0, 2.0))
    z = np.where(which == 0, -1.5, -1.5 + 2.5 * u)
    p = np.stack([x, y, z], 1) + rng.normal(0.0, 0.004, (n, 3))
    return np.ascontiguousarray(p.astype(np.float32))
