"""The cases the objective-scoring tests share (tests/test_particle_score_objective_cpu.py, tests/test_particle_score_objective_gpu.py):
the clouds, particles and gates of tests/particle_score_cases.py, with normals for both clouds and the settings of the two
new forms."""
import numpy as np

import particle_score_cases as pc
import plane_reference as pr

B_, M_ = pc.B_, pc.M_
PS = (1, 4, 25, 64, 100, 130)       # every geometry of ParticleLanes (particle_score_cases.PS says which)
KS = (1, 16, 128)                   # plane and GICP mode refuse K > 128: K = 150 runs in point mode, K150_PS below
K150_PS = (4, 64)
GATES = pc.GATES
DELTAS = (0.05, float("inf"))
SOLVER_DELTA = 0.05                 # the registrations' huber_delta: form "solved" must equal the explicit form at this delta
EPS = 1e-3
FORMS = ("plane", "gicp")
SOURCE_NORMAL_SEED = {"random": 11, "sheets": 12}
# The registrations in plane and GICP mode run with a pose prior (svnicp_set_pose_prior; sigma 2 cm in x / y, 5 cm in z,
# 0.01 / 0.005 rad).  These clouds of 300 points leave the two residuals' normal matrices with directions that nothing but
# the 1e-6 damping holds — the single undulating sheet of "random", the ground and far walls of "sheets" — and without a prior
# the Stein step moves most particles kilometres out of the scene, where a scoring has no inlier left to check.
PRIOR_MEAN = np.zeros(6)
PRIOR_LAMBDA = np.diag([2500.0, 2500.0, 400.0, 1e4, 1e4, 4e4])
# the weights cases (cloud, K): 16 particles, three GICP iterations, gate and temperatures of particle_score_cases.WEIGHT_*.
# RANKS_DIFFERENTLY: on the sheet-dominated cloud the particle with the lowest GICP cost is not the one with the lowest point
# cost.  Chosen on the restatement at the CPU oracle's poses — tests/test_particle_score_objective_cpu.py re-derives both argmins
# (ARGMIN: GICP, point) and their margins — and asserted by the GPU test on the device's.
WEIGHT_CASES = (("random", 16), ("sheets", 16), ("sheets", 1))
RANKS_DIFFERENTLY = ("sheets", 1)
ARGMIN = {("sheets", 1): (4, 2)}


def iterations_of(P, K):
    return 1 + (PS.index(P) + 2 * KS.index(K)) % 3


def cloud_of(P, K, form):
    """Both clouds meet every P, every K and both forms."""
    return pc.CLOUDS[(PS.index(P) + KS.index(K) + FORMS.index(form)) % 2]


def source_normals(orc, src, name):
    """Unit normals of the source from its own 16 neighbours, about a tenth of the rows zeroed ("no normal here"): the GICP
    form then accepts fewer pairs than the plane form."""
    ns = pr.normals(orc, src, 16)[0].copy()
    rng = np.random.default_rng(SOURCE_NORMAL_SEED.get(name, 13))
    ns[rng.random(len(ns)) < 0.1] = 0.0
    return ns


def random_unit_normals(n, seed, zero_fraction=0.1):
    """For the edge clouds (B, M) = (1, 1), (70, 64), too small for a neighbourhood: random unit rows, some zeroed."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if n > 1:
        v[rng.random(n) < zero_fraction] = 0.0
    return v
