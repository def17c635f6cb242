"""The clouds, particles and settings the particle-score tests share: tests/test_particle_score_cpu.py checks on the CPU oracle
the preconditions of what tests/test_particle_score_gpu.py compares exactly."""
import numpy as np

B_, M_ = 300, 3000
# every geometry of ParticleLanes: 1, 4, 9 -> 16 lanes; 25 -> 32; 64 -> 64 x 1 wave; 100 -> 64 x 2; 130 -> 64 x 4
# (appended, never inserted: cloud_of and iterations_of go by the position in PS).  25, not 24: in SVGD mode at K = 1 one
# of 24 particles (and of 18, 19, 21, 30, 31) ends without an inlier at the narrow gate, which the GPU test's cases exclude.
PS = (1, 4, 9, 64, 130, 25, 100)
KS = (1, 16, 128, 150)        # 150: the fused float32 stage B and the seeded scan
GATES = (0.3, 1.0)
CLOUDS = ("random", "sheets")
LR = 0.05                     # small enough that the particles of the prior stay apart over three iterations
T0_CORRECTION = (0.01, -0.02, 0.005, 0.001, 0.002, -0.001)    # a non-trivial initial mean
SEEDS = {"random": 3, "sheets": 20250718}
# the weights cases: 16 particles, K = 16, three iterations
WEIGHT_P, WEIGHT_K, WEIGHT_GATE, WEIGHT_T, COLD_T = 16, 16, 0.3, 1e-3, 1e-9


def clouds(pkg, name):
    if name == "random":
        return pkg.scans.random_clouds(B_, M_, seed=SEEDS[name])
    if name == "sheets":
        # whole columns of 64 beams (a scan of 300 points would repeat its head: duplicate target points), cut to size
        p = pkg.scans.make_pair(320, 3200, seed=SEEDS[name])
        return p.source[:B_].copy(), p.target[:M_].copy()
    raise ValueError(name)


def cloud_of(P, K):
    """Which cloud the parity case (P, K) runs on: both clouds meet every P and every K."""
    return CLOUDS[(PS.index(P) + KS.index(K)) % 2]


def iterations_of(P, K):
    return 1 + (PS.index(P) + 2 * KS.index(K)) % 3


def particles(pkg, P):
    return pkg.scans.make_particles(P, seed=3)


def initial_mean(pkg):
    return pkg.pipeline.correction_to_pose(T0_CORRECTION)


def total_poses(so3_exp, particles_6p, T0):
    """[P, 12]: T0 * Pose(Exp(r_p), t_p) of a get_particles() vector (SVN mode), R row-major then t."""
    x = np.asarray(particles_6p, np.float64).reshape(6, -1)
    out = np.zeros((x.shape[1], 12))
    for p in range(x.shape[1]):
        R = T0[:3, :3] @ so3_exp(x[3:, p])
        out[p, :9] = R.reshape(9)
        out[p, 9:] = T0[:3, 3] + T0[:3, :3] @ x[:3, p]
    return out
