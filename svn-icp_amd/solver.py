"""Host-side mirror of the reference solver classes on top of the C ABI.

Same names, argument meaning and call sequence as ``svnicp::SVGDICP`` / ``svnicp::SVNICP``
(/root/reference/svn-icp/include/core/SVGDICP.h:64-110, SVNICP.h:29-43) as driven by
``OdometryPipeline::ICP_processing`` (src/core/OdometryPipeline.cpp:573-607):

    solver = SVNICP(param, init_pose, ParticleWeightOpt())
    solver.add_cloud(source, target, init_pose)       # [B,3], [M,3] float64, [6,P]
    solver.set_initial_mean(T_4x4)                    # gtsam::Pose3 in the reference
    state  = solver.stein_align()
    mean   = solver.get_transformation()              # [6]  (x,y,z, so(3) log)
    var    = solver.get_distribution()                # [6]
    cov    = solver.get_cov_matrix()                  # [36] row-major
    parts  = solver.get_particles()                   # [6*P]: x.., y.., z.., rx.., ry.., rz..
    w      = solver.get_particle_weight()             # [P]

Clouds may be numpy arrays (host, copied over PCIe) or float64 CUDA torch tensors (device
pointers are handed to the library, no host round trip).  All compute happens in
libsvnicp_hip.so; this file holds no arithmetic of the path.
"""
from __future__ import annotations

import ctypes as C
import enum
from dataclasses import InitVar, dataclass

import numpy as np

from . import binding
from .binding import Params, SvnIcpError

_OPT = {"Adam": 0, "RMSprop": 1, "SGD": 2, "Adagrad": 3}


class SteinICPState(enum.IntEnum):  # include/core/SVGDICP.h:59-62
    ALIGN_SUCCESS = 1
    NO_OPTIMIZER = 2


@dataclass
class SteinICPParam:  # include/core/SVGDICP.h:41-57 (same field names and defaults)
    iterations: int = 50
    use_minibatch: bool = False      # never set by the reference NODE; its solver acts on it (SVGDICP.cpp:176-199, :83; SVNICP.cpp:53)
    batch_size: int = 50             # rows per iteration when use_minibatch is set; else the reference uses N_src (SVGDICP.cpp:181)
    lr: float = 0.02
    max_dist: float = 1.0
    normalize_cloud: bool = True     # normalize_factor_ == 1 in the reference (SVGDICP.cpp:32)
    optimizer: str = "Adam"
    check_early_stop: bool = False
    convergence_steps: int = 5       # unused by the reference solver
    convergence_threshold: float = 1e-5
    KNN_count: int = 100
    SVN_full_grad: bool = True
    record_trace: bool = False       # test hook (not in the reference)
    minibatch_seed: int = 0          # seed of the generated mini-batch tables (not in the reference: see minibatch_indices)
    residual: str = "point"          # "point" (the reference) | "plane": Huber-weighted point-to-plane | "gicp": generalized ICP (neither in the reference)
    huber_delta: float = 0.1         # plane residual: weight 1 up to this |r|, huber_delta / |r| beyond (inf = unweighted)
    normal_k: int = 16               # plane residual: neighbours of a target point its normal is estimated from (4..64)
    gicp_epsilon: float = 1e-3       # gicp residual: a surface's covariance along its normal, in units of the in-plane one ([1e-6, 1])


@dataclass
class ParticleWeightOpt:  # include/core/SVNICP.h:25-27
    """``use_weight_mean`` alone is as inert as in the reference, whose particle_weight_ never leaves ones / P
    (SVNICP.cpp:32, :46).  With ``weight_dist > 0`` as well (not in the reference) every registration of an ``SVNICP`` ends
    with one scoring of the particles at the gate ``weight_dist`` (metres) and soft-min weights of temperature
    ``temperature`` (m^2, > 0), which get_transformation / get_distribution / get_cov_matrix / get_particle_weight then
    honour (include/svnicp_hip.h, "score and weight the particles").  ``weight_cost``: "point" (the mean truncated squared
    point distance) or "solved": the residual the registration ran with, plane or generalized-ICP, with the solver's own
    huber_delta and epsilon ("score and weight the particles in the objective the solver minimised")."""
    use_weight_mean: bool = False
    weight_dist: float = 0.0
    temperature: float = 0.0
    weight_cost: InitVar[str] = "point"   # an attribute, not one of the reference's three fields (fields() / asdict() keep those)

    def __post_init__(self, weight_cost):
        self.weight_cost = weight_cost


@dataclass
class ParticleScores:
    """svnicp_score_particles (include/svnicp_hip.h): every particle's final pose scored through the candidate table."""
    evaluated: np.ndarray      # [P] rows with a finite transformed point and a winner whose d2 is not NaN
    inliers: np.ndarray        # [P] evaluated rows with d2 < max_corr_dist^2
    plane_inliers: np.ndarray  # [P] inliers whose winner has a normal (0 without normals)
    sum_d2: np.ndarray         # [P] over the inliers
    sum_r2: np.ndarray         # [P] over the plane inliers
    cost: np.ndarray           # [P] (sum_d2 + (B - inliers) * max_corr_dist^2) / B; forms "plane", "gicp": (sum_h + (B - accepted) * h(max_corr_dist)) / B
    poses: np.ndarray          # [P, 3, 4] the total poses that were scored, [R | t]
    # The objective that was scored (svnicp_get_score_objective: resolved, never "solved"): attributes, not fields of the block.
    # In the forms "plane" and "gicp" fields 2 and 4 of the block are the accepted pairs and sum h: accepted / sum_h name them
    # (the same arrays as plane_inliers / sum_r2; at huber_delta = inf the plane form's equal the point form's bit for bit)
    form = "point"             # "point" | "plane" | "gicp"
    max_corr_dist = 0.0
    huber_delta = 0.0          # as used; 0 in the point form
    gicp_epsilon = 0.0         # as used; 0 unless the form is "gicp"

    @property
    def accepted(self) -> np.ndarray:
        return self.plane_inliers

    @property
    def sum_h(self) -> np.ndarray:
        return self.sum_r2


@dataclass
class RegistrationEval:
    """struct svnicp_eval (include/svnicp_hip.h, "evaluate a registration"): one pose against the whole target."""
    has_normals: bool          # the context holds normals of the current target: the plane figures are filled
    rows: int                  # B
    evaluated: int             # rows with a finite transformed point and a nearest target whose d2 is not NaN
    inliers: int               # evaluated rows with d2 < max_corr_dist^2
    plane_inliers: int         # inliers whose nearest target has a normal (0 without normals)
    sum_d2: float              # over the inliers
    sum_r2: float              # over the plane inliers
    fitness: float             # inliers / rows
    inlier_rmse: float         # sqrt(sum_d2 / inliers), 0 when there are none
    plane_rmse: float          # sqrt(sum_r2 / plane_inliers), 0 when there are none
    pose: np.ndarray           # 4x4, the pose that was evaluated (map <- sensor)


@dataclass
class RegistrationInformation:
    """struct svnicp_information (include/svnicp_hip.h, "information matrix of a registration"): the Gauss-Newton normal
    equations of the last ``evaluate``'s pairs, tangent T * Exp([v ; omega]) (translation first), and their eigen-structure."""
    form: str                  # "point" | "plane" | "gicp"
    pairs: int                 # contributing rows
    rank: int                  # eigenvalues above eig_floor_ratio * the largest
    huber_delta: float
    eig_floor_ratio: float
    max_corr_dist: float       # the gate of the evaluate the rows came from
    sum_w: float
    sum_wr2: float             # sum of w d2 (point), w r^2 (plane) or w rho^2 (gicp)
    sigma2: float              # sum_wr2 / (dim * pairs - rank), 0 when that is not positive
    H: np.ndarray              # [6, 6]
    b: np.ndarray              # [6]
    eigval: np.ndarray         # [6] ascending
    eigvec: np.ndarray         # [6, 6], row i = unit eigenvector i
    eig_t: np.ndarray          # [3], of H[0:3, 0:3]
    vec_t: np.ndarray          # [3, 3]
    eig_r: np.ndarray          # [3], of H[3:6, 3:6]
    vec_r: np.ndarray          # [3, 3]
    step: np.ndarray           # [6] -H+ b
    cov: np.ndarray            # [6, 6] sigma2 * H+
    pose: np.ndarray           # 4x4, the evaluated pose


@dataclass
class ParticleModes:
    """struct svnicp_modes (include/svnicp_hip.h, "particle modes"): the connected components of the particles' link graph,
    heaviest first; the per-mode arrays hold ``n_reported`` entries."""
    particles: int             # P of the set that was clustered
    nonfinite: int             # particles with a non-finite component: in no mode
    n_modes: int               # all modes
    n_reported: int            # min(n_modes, max_modes)
    has_scores: bool           # best / cost_min / cost_mean are filled
    label: np.ndarray          # [n] lowest particle index of the mode
    count: np.ndarray          # [n] members
    best: np.ndarray           # [n] member with the lowest cost, -1 without scores
    mass: np.ndarray           # [n] W / W_all
    cost_min: np.ndarray       # [n]
    cost_mean: np.ndarray      # [n]
    mean: np.ndarray           # [n, 6] correction coordinates, as get_transformation
    cov: np.ndarray            # [n, 6, 6]
    pose: np.ndarray           # [n, 4, 4] the mode's total pose (map <- sensor): what ``evaluate(pose=...)`` takes


def _modes_from_struct(o) -> ParticleModes:
    n = int(o.n_reported)
    arr = lambda name, dtype, *shape: np.array(getattr(o, name)[:], dtype).reshape((binding.MODES_MAX,) + shape)[:n].copy()   # noqa: E731
    T = np.tile(np.eye(4), (n, 1, 1))
    T[:, :3, :3] = arr("R", np.float64, 3, 3)
    T[:, :3, 3] = arr("t", np.float64, 3)
    return ParticleModes(int(o.particles), int(o.nonfinite), int(o.n_modes), n, bool(o.has_scores), arr("label", np.int32),
                         arr("count", np.int32), arr("best", np.int32), arr("mass", np.float64), arr("cost_min", np.float64),
                         arr("cost_mean", np.float64), arr("mean", np.float64, 6), arr("cov", np.float64, 6, 6), T)


_INFO_FORMS = {"point": binding.INFO_POINT, "plane": binding.INFO_PLANE, "gicp": binding.INFO_GICP}
_INFO_NAMES = {v: k for k, v in _INFO_FORMS.items()}


def _information_from_struct(o) -> RegistrationInformation:
    arr = lambda name, *shape: np.array(getattr(o, name)[:], np.float64).reshape(shape)   # noqa: E731
    T = np.eye(4)
    T[:3, :3] = arr("R", 3, 3)
    T[:3, 3] = arr("t", 3)
    return RegistrationInformation(_INFO_NAMES[int(o.form)], int(o.pairs), int(o.rank), float(o.huber_delta),
                                   float(o.eig_floor_ratio), float(o.max_corr_dist), float(o.sum_w), float(o.sum_wr2), float(o.sigma2),
                                   arr("H", 6, 6), arr("b", 6), arr("eigval", 6), arr("eigvec", 6, 6), arr("eig_t", 3), arr("vec_t", 3, 3),
                                   arr("eig_r", 3), arr("vec_r", 3, 3), arr("step", 6), arr("cov", 6, 6), T)


def information_solve(form, pairs: int, sum_wr2: float, H, b, eig_floor_ratio: float = 0.0, sum_w: float = 0.0,
                      huber_delta: float = float("inf"), max_corr_dist: float = 0.0, pose=None) -> RegistrationInformation:
    """svnicp_information_solve (host only, no device): rank, eigen-structure, step, sigma2 and cov of the normal equations
    ``H`` [6, 6], ``b`` [6] — for instance the sums of several row-sharded contexts added up."""
    o = binding.InformationStruct()
    o.struct_size = C.sizeof(binding.InformationStruct)
    o.form = int(_INFO_FORMS.get(form, form))
    o.pairs, o.sum_wr2, o.eig_floor_ratio = int(pairs), float(sum_wr2), float(eig_floor_ratio)
    o.sum_w, o.huber_delta, o.max_corr_dist = float(sum_w), float(huber_delta), float(max_corr_dist)
    o.H[:] = np.asarray(H, np.float64).reshape(36).tolist()
    o.b[:] = np.asarray(b, np.float64).reshape(6).tolist()
    T = np.eye(4) if pose is None else np.asarray(pose, np.float64).reshape(4, 4)
    o.R[:] = T[:3, :3].reshape(9).tolist()
    o.t[:] = T[:3, 3].tolist()
    if binding.load_library().svnicp_information_solve(C.byref(o)) != 0:
        raise binding.SvnIcpError("svnicp_information_solve: invalid input (form, eig_floor_ratio outside [0, 1), negative pairs, "
                                  "or a non-finite entry of H, b or sum_wr2)")
    return _information_from_struct(o)


def initialize_particles(particle_count: int, ub, lb, rng: np.random.Generator | None = None) -> np.ndarray:
    """svnicp::initialize_particles (src/core/ICPUtils.cpp:45-58): uniform in [lb, ub] per row,
    zeros for a single particle.  Returns [6, P] float64."""
    if particle_count == 1:
        return np.zeros((6, 1))
    rng = rng or np.random.default_rng()
    ub, lb = np.asarray(ub, np.float64).reshape(6, 1), np.asarray(lb, np.float64).reshape(6, 1)
    return (ub - lb) * rng.random((6, particle_count)) + lb


_M64 = (1 << 64) - 1


def _splitmix64_int(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def minibatch_indices(seed: int, registration: int, iterations: int, batch_size: int, n_source: int) -> np.ndarray:
    """The mini-batch table the library generates on the device for registration ``registration`` (0, 1, ...) after
    ``svnicp_set_minibatch(ctx, batch_size, seed)``, bit for bit (include/svnicp_hip.h): at flat position j

        base = splitmix64(seed * 1000003 + registration);  bits = splitmix64(base + j);  idx = floor(bits * B / 2^64)

    Returns int32 [iterations, batch_size] with values in [0, n_source)."""
    from .scans import _splitmix64
    I, b, B = int(iterations), int(batch_size), int(n_source)
    if I < 0 or b < 0 or not 1 <= B < (1 << 31):
        raise ValueError("need iterations >= 0, batch_size >= 0 and 1 <= n_source < 2^31")
    base = _splitmix64_int((int(seed) * 1000003 + int(registration)) & _M64)
    with np.errstate(over="ignore"):
        bits = _splitmix64(np.arange(I * b, dtype=np.uint64) + np.uint64(base))
    Bu, lo32, s32 = np.uint64(B), np.uint64(0xFFFFFFFF), np.uint64(32)
    idx = ((bits >> s32) * Bu + (((bits & lo32) * Bu) >> s32)) >> s32      # the high 64 bits of bits * B, for B < 2^32
    return idx.astype(np.int32).reshape(I, b)


def poses_3x4(poses12: np.ndarray) -> np.ndarray:
    """[P, 12] (R row-major, then t) as [P, 3, 4] = [R | t]."""
    p = np.asarray(poses12, np.float64).reshape(-1, 12)
    return np.concatenate([p[:, :9].reshape(-1, 3, 3), p[:, 9:].reshape(-1, 3, 1)], axis=2)


def _is_torch_cuda(x) -> bool:
    return hasattr(x, "is_cuda") and bool(x.is_cuda)


class _SolverBase:
    _mode = 0

    def __init__(self, parameters: SteinICPParam, init_pose, opt: ParticleWeightOpt | None = None, device: int = 0):
        self._L = binding.load_library()
        self._h = C.c_void_p()
        self.config = parameters
        self.weight_config = opt or ParticleWeightOpt()
        init = self._pose_arg(init_pose)
        self._P = init.shape[1]
        prm = Params(C.sizeof(Params), self._mode, int(parameters.iterations), int(parameters.KNN_count),
                     float(parameters.lr), float(parameters.max_dist), float(parameters.convergence_threshold),
                     int(parameters.check_early_stop), int(parameters.SVN_full_grad),
                     _OPT.get(parameters.optimizer, -1), int(parameters.record_trace))
        rc = self._L.svnicp_create(C.byref(prm), int(device), init.ctypes.data_as(C.POINTER(C.c_double)), self._P,
                                   C.byref(self._h))
        if rc != 0:
            raise SvnIcpError(f"svnicp_create failed ({rc}): {self._L.svnicp_last_error(None).decode()}")
        self._B = self._M = 0
        self._K = int(parameters.KNN_count)
        self._keep = None
        self._mb = 0      # rows per iteration in mini-batch mode, 0 = full batch
        if parameters.use_minibatch:
            self.set_minibatch(int(parameters.batch_size), int(parameters.minibatch_seed))
        if parameters.residual != "point":
            self.set_residual(parameters.residual, float(parameters.huber_delta), int(parameters.normal_k), float(parameters.gicp_epsilon))
        w = self.weight_config
        if self._mode == 0 and w.use_weight_mean and w.weight_dist > 0:   # the option belongs to SVNICP's constructor only
            self.set_particle_weighting("softmin", float(w.weight_dist), float(w.temperature), cost=w.weight_cost)

    # -- plumbing -------------------------------------------------------------------------
    @staticmethod
    def _pose_arg(init_pose) -> np.ndarray:
        if hasattr(init_pose, "detach"):
            init_pose = init_pose.detach().cpu().numpy()
        a = np.ascontiguousarray(np.asarray(init_pose, np.float64))
        if a.ndim == 3:
            a = a.reshape(a.shape[0], a.shape[1])
        if a.ndim != 2 or a.shape[0] != 6:
            raise ValueError("init_pose must be [6, P] (or [6, P, 1])")
        return np.ascontiguousarray(a)

    def _check(self, rc: int, what: str):
        if rc < 0:
            raise SvnIcpError(f"{what} failed ({rc}): {self._L.svnicp_last_error(self._h).decode()}")
        return rc

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.svnicp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # -- reference interface ----------------------------------------------------------------
    def add_cloud(self, new_cloud, target, init_pose):
        """SVGDICP::add_cloud (src/core/SVGDICP.cpp:46-62)."""
        if _is_torch_cuda(new_cloud) != _is_torch_cuda(target):
            raise ValueError("source and target must live on the same side (both host or both device)")
        if _is_torch_cuda(new_cloud):
            import torch
            src = new_cloud.to(torch.float64).contiguous()
            tgt = target.to(torch.float64).contiguous()
            torch.cuda.current_stream(src.device).synchronize()
            self._keep = (src, tgt)
            B, M = src.shape[0], tgt.shape[0]
            rc = self._L.svnicp_set_clouds(self._h, C.c_void_p(src.data_ptr()), B, C.c_void_p(tgt.data_ptr()), M, 1)
            self._check(rc, "svnicp_set_clouds")      # device-to-device copies queued on the library's stream; self._keep holds the
            #                                           tensors until the next add_cloud, and the caller must not write to them
            #                                           before stein_align has returned (include/svnicp_hip.h, svnicp_set_clouds)
        else:
            src = np.ascontiguousarray(np.asarray(new_cloud, np.float64).reshape(-1, 3))
            tgt = np.ascontiguousarray(np.asarray(target, np.float64).reshape(-1, 3))
            B, M = src.shape[0], tgt.shape[0]
            rc = self._L.svnicp_set_clouds(self._h, src.ctypes.data_as(C.c_void_p), B, tgt.ctypes.data_as(C.c_void_p),
                                           M, 0)
            self._check(rc, "svnicp_set_clouds")
        self._B, self._M = B, M
        init = self._pose_arg(init_pose)
        self._P = init.shape[1]
        self._check(self._L.svnicp_set_particles(self._h, init.ctypes.data_as(C.POINTER(C.c_double)), self._P),
                    "svnicp_set_particles")

    def set_source(self, new_cloud):
        """svnicp_set_source: a new source scan against the target, particles and initial mean already set (host array
        or CUDA tensor)."""
        if _is_torch_cuda(new_cloud):
            import torch
            src = new_cloud.to(torch.float64).contiguous()
            torch.cuda.current_stream(src.device).synchronize()
            self._keep_source = src                    # as in add_cloud: held until the next call replaces it
            rc = self._L.svnicp_set_source(self._h, C.c_void_p(src.data_ptr()), src.shape[0], 1)
        else:
            src = np.ascontiguousarray(np.asarray(new_cloud, np.float64).reshape(-1, 3))
            rc = self._L.svnicp_set_source(self._h, src.ctypes.data_as(C.c_void_p), src.shape[0], 0)
        self._check(rc, "svnicp_set_source")
        self._B = src.shape[0]

    def add_cloud_device_target(self, new_cloud, target_devptr: int, M: int, init_pose):
        """add_cloud with a host source scan and a target that already lives in HBM (DeviceVoxelHashMap.get_map):
        the source goes over PCIe, the target is copied device-to-device."""
        src = np.ascontiguousarray(np.asarray(new_cloud, np.float64).reshape(-1, 3))
        self._check(self._L.svnicp_set_source(self._h, src.ctypes.data_as(C.c_void_p), src.shape[0], 0), "svnicp_set_source")
        self._check(self._L.svnicp_set_target(self._h, C.c_void_p(int(target_devptr)), int(M), 1), "svnicp_set_target")
        self._B, self._M = src.shape[0], int(M)
        init = self._pose_arg(init_pose)
        self._P = init.shape[1]
        self._check(self._L.svnicp_set_particles(self._h, init.ctypes.data_as(C.POINTER(C.c_double)), self._P),
                    "svnicp_set_particles")

    def add_cloud_device(self, source_devptr: int, B: int, target_devptr: int, M: int, init_pose):
        """add_cloud with both clouds already in HBM (float64 rows: DevicePreprocessor.source, DeviceVoxelHashMap.get_map):
        two device-to-device copies, nothing crosses PCIe but the particle prior."""
        self._check(self._L.svnicp_set_source(self._h, C.c_void_p(int(source_devptr)), int(B), 1), "svnicp_set_source")
        self._check(self._L.svnicp_set_target(self._h, C.c_void_p(int(target_devptr)), int(M), 1), "svnicp_set_target")
        self._B, self._M = int(B), int(M)
        init = self._pose_arg(init_pose)
        self._P = init.shape[1]
        self._check(self._L.svnicp_set_particles(self._h, init.ctypes.data_as(C.POINTER(C.c_double)), self._P),
                    "svnicp_set_particles")

    def set_initial_mean(self, pose):
        """SVGDICP::set_initial_mean(gtsam::Pose3) (include/core/SVGDICP.h:102-110).
        ``pose``: 4x4 homogeneous matrix, or a (R[3,3], t[3]) pair."""
        if isinstance(pose, (tuple, list)) and len(pose) == 2:
            R, t = np.asarray(pose[0], np.float64).reshape(3, 3), np.asarray(pose[1], np.float64).reshape(3)
        else:
            T = np.asarray(pose, np.float64).reshape(4, 4)
            R, t = T[:3, :3], T[:3, 3]
        R = np.ascontiguousarray(R).reshape(9)
        t = np.ascontiguousarray(t)
        dp = C.POINTER(C.c_double)
        self._check(self._L.svnicp_set_initial_mean(self._h, R.ctypes.data_as(dp), t.ctypes.data_as(dp)),
                    "svnicp_set_initial_mean")

    def set_k(self, k: int):
        self._K = int(k)
        self._check(self._L.svnicp_set_k(self._h, int(k)), "svnicp_set_k")

    def set_option(self, name: str, value) -> None:
        """Test / profiling knob of this context (include/svnicp_hip.h: svnicp_set_option)."""
        self._check(self._L.svnicp_set_option(self._h, str(name).encode(), str(value).encode()), "svnicp_set_option")

    # -- mini-batch (SteinICPParam.use_minibatch / batch_size; include/svnicp_hip.h "mini-batch") -------------------------
    def set_minibatch(self, batch_size: int, seed: int = 0) -> None:
        """Rows per iteration from now on (0 = full batch); registration n after this call uses
        ``minibatch_indices(seed, n, iterations, batch_size, B)``."""
        self._check(self._L.svnicp_set_minibatch(self._h, int(batch_size), int(seed) & _M64), "svnicp_set_minibatch")
        self._mb = max(0, int(batch_size))

    def set_minibatch_indices(self, table) -> None:
        """An explicit table int32 [iterations, batch_size] (numpy, or an int32 CUDA torch tensor), used by every following
        registration until ``set_minibatch`` is called again."""
        if _is_torch_cuda(table):
            import torch
            t = table.to(torch.int32).contiguous()
            if t.dim() != 2:
                raise ValueError("the mini-batch table must be [iterations, batch_size]")
            torch.cuda.current_stream(t.device).synchronize()
            ptr, shape, kind = C.c_void_p(t.data_ptr()), t.shape, 1
        else:
            t = np.ascontiguousarray(np.asarray(table), np.int32)
            if t.ndim != 2:
                raise ValueError("the mini-batch table must be [iterations, batch_size]")
            ptr, shape, kind = t.ctypes.data_as(C.c_void_p), t.shape, 0
        self._check(self._L.svnicp_set_minibatch_indices(self._h, ptr, int(shape[0]), int(shape[1]), kind),
                    "svnicp_set_minibatch_indices")
        self._mb = int(shape[1])

    def get_minibatch_indices(self) -> np.ndarray:
        """The table the last registration used, int32 [iterations, batch_size]."""
        out = np.zeros((int(self.config.iterations), self._mb), np.int32)
        self._check(self._L.svnicp_get_minibatch_indices(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))),
                    "svnicp_get_minibatch_indices")
        return out

    def get_minibatch_candidates(self) -> np.ndarray:
        """Candidate target indices of every drawn position, int32 [iterations, batch_size, K]."""
        out = np.zeros((int(self.config.iterations), self._mb, self._K), np.int32)
        self._check(self._L.svnicp_get_minibatch_candidates(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))),
                    "svnicp_get_minibatch_candidates")
        return out

    def get_minibatch_rows(self) -> tuple:
        """(unique source rows drawn U, queries stage A ran n_q) of the last registration in mini-batch mode."""
        out = (C.c_int64 * 2)()
        self._check(self._L.svnicp_get_minibatch_rows(self._h, out), "svnicp_get_minibatch_rows")
        return int(out[0]), int(out[1])

    # -- point-to-plane residual (include/svnicp_hip.h "point-to-plane residual") ---------------------------------------------
    _RESIDUAL = {"point": 0, "plane": 1}

    def set_residual(self, residual: str = "plane", huber_delta: float = 0.1, normal_k: int = 16, gicp_epsilon: float = 1e-3) -> None:
        """"point" (the reference's residual), "plane" (Huber-weighted point-to-plane) or "gicp" (generalized ICP: both
        clouds' normals weigh every pair; ``gicp_epsilon`` is read in that mode only) from the next registration on."""
        if residual == "gicp":
            self._check(self._L.svnicp_set_residual_gicp(self._h, float(huber_delta), int(normal_k), float(gicp_epsilon)),
                        "svnicp_set_residual_gicp")
            return
        if residual not in self._RESIDUAL:
            raise ValueError('residual must be "point", "plane" or "gicp"')
        self._check(self._L.svnicp_set_residual(self._h, self._RESIDUAL[residual], float(huber_delta), int(normal_k)),
                    "svnicp_set_residual")

    def set_target_normals(self, normals) -> None:
        """Normals of the current target, [M, 3] (numpy, or a float64 CUDA torch tensor); call after ``add_cloud``.  Rows are
        normalised on upload; a zero or non-finite row means "no normal here"."""
        if _is_torch_cuda(normals):
            import torch
            n = normals.to(torch.float64).contiguous()
            if n.dim() != 2 or n.shape[1] != 3:
                raise ValueError("normals must be [M, 3]")
            torch.cuda.current_stream(n.device).synchronize()
            self._keep_normals = n
            ptr, M, kind = C.c_void_p(n.data_ptr()), int(n.shape[0]), 1
        else:
            n = np.ascontiguousarray(np.asarray(normals, np.float64))
            if n.ndim != 2 or n.shape[1] != 3:
                raise ValueError("normals must be [M, 3]")
            ptr, M, kind = n.ctypes.data_as(C.c_void_p), int(n.shape[0]), 0
        self._check(self._L.svnicp_set_target_normals(self._h, ptr, M, kind), "svnicp_set_target_normals")

    def set_target_normals_device(self, normals_devptr: int, M: int) -> None:
        """set_target_normals for float64 rows [M][3] that already live in HBM (DeviceVoxelHashMap.get_map_normals): one
        device-to-device copy, QUEUED on the context's stream like add_cloud_device's target copy (not complete when this
        returns): the rows must stay unchanged until stein_align or synchronize has returned."""
        self._check(self._L.svnicp_set_target_normals(self._h, C.c_void_p(int(normals_devptr)), int(M), 1),
                    "svnicp_set_target_normals")

    def get_target_normals(self) -> np.ndarray:
        """The supplied or estimated unit normals of the target, [M, 3]; rows without a normal are 0."""
        out = np.zeros((self._M, 3), np.float64)
        self._check(self._L.svnicp_get_target_normals(self._h, out.ctypes.data_as(C.POINTER(C.c_double))),
                    "svnicp_get_target_normals")
        return out

    def get_plane_stats(self, with_sums: bool = True) -> tuple:
        """(per particle [P, 2] = {accepted pairs, sum w r^2} of the last iteration run, normal passes run so far);
        ``with_sums=False`` returns (None, passes) and needs no registration."""
        out = np.zeros((self._P, 2), np.float64) if with_sums else None
        n = C.c_int64(0)
        self._check(self._L.svnicp_get_plane_stats(self._h, out.ctypes.data_as(C.POINTER(C.c_double)) if with_sums else None,
                                                   C.byref(n)), "svnicp_get_plane_stats")
        return out, int(n.value)

    # -- generalized-ICP residual (include/svnicp_hip.h "generalized-ICP residual") ---------------------------------------------
    def set_source_normals(self, normals) -> None:
        """Normals of the current source, [B, 3] (numpy, or a float64 CUDA torch tensor); call after ``add_cloud``.  The
        rules of ``set_target_normals``; read by the "gicp" residual only."""
        if _is_torch_cuda(normals):
            import torch
            n = normals.to(torch.float64).contiguous()
            if n.dim() != 2 or n.shape[1] != 3:
                raise ValueError("normals must be [B, 3]")
            torch.cuda.current_stream(n.device).synchronize()
            self._keep_source_normals = n
            ptr, B, kind = C.c_void_p(n.data_ptr()), int(n.shape[0]), 1
        else:
            n = np.ascontiguousarray(np.asarray(normals, np.float64))
            if n.ndim != 2 or n.shape[1] != 3:
                raise ValueError("normals must be [B, 3]")
            ptr, B, kind = n.ctypes.data_as(C.c_void_p), int(n.shape[0]), 0
        self._check(self._L.svnicp_set_source_normals(self._h, ptr, B, kind), "svnicp_set_source_normals")

    def get_source_normals(self) -> np.ndarray:
        """The supplied or estimated unit normals of the source, [B, 3]; rows without a normal are 0."""
        out = np.zeros((self._B, 3), np.float64)
        self._check(self._L.svnicp_get_source_normals(self._h, out.ctypes.data_as(C.POINTER(C.c_double))),
                    "svnicp_get_source_normals")
        return out

    def get_gicp_stats(self, with_sums: bool = True) -> tuple:
        """(per particle [P, 2] = {accepted pairs, sum w rho^2} of the last iteration run, (target, source) normal passes run
        so far); ``with_sums=False`` returns (None, passes) and needs no registration."""
        out = np.zeros((self._P, 2), np.float64) if with_sums else None
        n = (C.c_int64 * 2)(0, 0)
        self._check(self._L.svnicp_get_gicp_stats(self._h, out.ctypes.data_as(C.POINTER(C.c_double)) if with_sums else None, n),
                    "svnicp_get_gicp_stats")
        return out, (int(n[0]), int(n[1]))

    # -- Gaussian pose prior on the correction (include/svnicp_hip.h "pose prior") ---------------------------------------------
    def set_pose_prior(self, mean6=None, information=None) -> None:
        """A Gaussian prior on the correction pose from the next registration on: ``mean6`` = [t ; rotation vector] in the
        coordinates of ``get_transformation`` (None: zero), ``information`` the 6x6 matrix Lambda in the order (t, r) and in the
        units of the cost: for a metric covariance Sigma and a point noise sigma_pt, sigma_pt**2 * inv(Sigma).
        ``information=None`` turns the prior off.  SVGD mode refuses at ``stein_align``."""
        dp = C.POINTER(C.c_double)
        if information is None:
            self._check(self._L.svnicp_set_pose_prior(self._h, None, None), "svnicp_set_pose_prior")
            return
        m = np.ascontiguousarray(np.zeros(6) if mean6 is None else np.asarray(mean6, np.float64).reshape(6))
        lam = np.ascontiguousarray(np.asarray(information, np.float64).reshape(36))
        self._check(self._L.svnicp_set_pose_prior(self._h, m.ctypes.data_as(dp), lam.ctypes.data_as(dp)), "svnicp_set_pose_prior")

    def pose_prior(self):
        """(mean6, information [6, 6]) of the prior the next registration runs with, or None when it is off."""
        on, m, lam = C.c_int(0), np.zeros(6, np.float64), np.zeros((6, 6), np.float64)
        dp = C.POINTER(C.c_double)
        self._check(self._L.svnicp_get_pose_prior(self._h, C.byref(on), m.ctypes.data_as(dp), lam.ctypes.data_as(dp)), "svnicp_get_pose_prior")
        return (m, lam) if on.value else None

    # -- evaluate a registration (include/svnicp_hip.h "evaluate a registration") ---------------------------------------------
    def evaluate(self, max_corr_dist: float, pose=None) -> RegistrationEval:
        """Fitness, inlier RMSE and (with normals) plane RMSE of ``pose`` (4x4, map <- sensor) against the whole target, on
        the device; ``pose=None``: the last registration's result, initial mean times the mean correction."""
        e = binding.EvalStruct()
        e.struct_size = C.sizeof(binding.EvalStruct)
        dp = C.POINTER(C.c_double)
        if pose is None:
            R = t = None
        else:
            T = np.asarray(pose, np.float64).reshape(4, 4)
            Rk, tk = np.ascontiguousarray(T[:3, :3]).reshape(9), np.ascontiguousarray(T[:3, 3])
            R, t = Rk.ctypes.data_as(dp), tk.ctypes.data_as(dp)
        self._check(self._L.svnicp_evaluate(self._h, R, t, float(max_corr_dist), C.byref(e)), "svnicp_evaluate")
        T = np.eye(4)
        T[:3, :3] = np.array(e.R[:]).reshape(3, 3)
        T[:3, 3] = e.t[:]
        return RegistrationEval(bool(e.has_normals), int(e.rows), int(e.evaluated), int(e.inliers), int(e.plane_inliers),
                                float(e.sum_d2), float(e.sum_r2), float(e.fitness), float(e.inlier_rmse), float(e.plane_rmse), T)

    def information(self, form="plane", huber_delta: float = float("inf"), eig_floor_ratio: float = 0.0,
                    gicp_epsilon: float | None = None) -> RegistrationInformation:
        """The Gauss-Newton information matrix H, gradient b, their eigen-structure, rank, step -H+ b and covariance over the
        pairs of the last ``evaluate`` (include/svnicp_hip.h "information matrix of a registration"); ``form`` "point",
        "plane" or "gicp" is independent of the residual the solver ran.  "gicp" (svnicp_eval_information_gicp) is the
        generalized-ICP objective: it needs normals of both clouds in the context, and ``gicp_epsilon`` (None: this solver's
        ``SteinICPParam.gicp_epsilon``) is its surface regularisation."""
        o = binding.InformationStruct()
        o.struct_size = C.sizeof(binding.InformationStruct)
        code = int(_INFO_FORMS.get(form, form))
        if code == binding.INFO_GICP:
            eps = self.config.gicp_epsilon if gicp_epsilon is None else gicp_epsilon
            self._check(self._L.svnicp_eval_information_gicp(self._h, float(huber_delta), float(eps), float(eig_floor_ratio), C.byref(o)),
                        "svnicp_eval_information_gicp")
        else:
            self._check(self._L.svnicp_eval_information(self._h, code, float(huber_delta), float(eig_floor_ratio), C.byref(o)),
                        "svnicp_eval_information")
        return _information_from_struct(o)

    def get_eval_pairs(self) -> tuple:
        """Per source row of the last ``evaluate``: (nearest target row, int32 [B], -1 = not evaluated; its d2, float64 [B],
        NaN = not evaluated)."""
        idx, d2 = np.zeros(self._B, np.int32), np.zeros(self._B, np.float64)
        self._check(self._L.svnicp_get_eval_pairs(self._h, idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  d2.ctypes.data_as(C.POINTER(C.c_double))), "svnicp_get_eval_pairs")
        return idx, d2

    @property
    def eval_index_ptr(self) -> int:
        """Device address of the last evaluate's int32 [B] nearest target rows (0 before any)."""
        return int(self._L.svnicp_eval_index_devptr(self._h) or 0)

    @property
    def eval_dist2_ptr(self) -> int:
        """Device address of the last evaluate's float64 [B] squared distances (0 before any)."""
        return int(self._L.svnicp_eval_dist2_devptr(self._h) or 0)

    # -- score and weight the particles (include/svnicp_hip.h "score and weight the particles") -------------------------------
    _WEIGHTING = {"uniform": 0, "softmin": 1}

    _SCORE_FORM = {"solved": binding.SCORE_AS_SOLVED, "point": binding.SCORE_POINT, "plane": binding.SCORE_PLANE, "gicp": binding.SCORE_GICP}

    def _objective(self, form, max_corr_dist, huber_delta=None, gicp_epsilon=None) -> "binding.ScoreObjectiveStruct":
        if form not in self._SCORE_FORM and not isinstance(form, int):
            raise ValueError(f"form must be one of {sorted(self._SCORE_FORM)}")
        return binding.ScoreObjectiveStruct(C.sizeof(binding.ScoreObjectiveStruct), int(self._SCORE_FORM.get(form, form)), float(max_corr_dist),
                                            0.0 if huber_delta is None else float(huber_delta), 0.0 if gicp_epsilon is None else float(gicp_epsilon))

    def set_particle_weighting(self, kind="uniform", max_corr_dist: float = 0.0, temperature: float = 0.0, cost="point",
                               huber_delta=None, gicp_epsilon=None) -> None:
        """"uniform" (the reference) or "softmin": every following registration ends with one scoring at ``max_corr_dist``
        and the weights exp(-(cost - cost_min) / temperature) / Z.  ``cost``: "point" (svnicp_set_particle_weighting), or
        "plane" | "gicp" | "solved" (svnicp_set_particle_weighting_objective; ``huber_delta`` / ``gicp_epsilon`` None: the
        solver's own)."""
        k = self._WEIGHTING.get(kind, kind)
        if cost == "point":
            self._check(self._L.svnicp_set_particle_weighting(self._h, int(k), float(max_corr_dist), float(temperature)),
                        "svnicp_set_particle_weighting")
            return
        obj = self._objective(cost, max_corr_dist, huber_delta, gicp_epsilon)
        self._check(self._L.svnicp_set_particle_weighting_objective(self._h, int(k), C.byref(obj), float(temperature)),
                    "svnicp_set_particle_weighting_objective")

    def get_score_objective(self) -> "binding.ScoreObjectiveStruct":
        """The resolved objective of the last scoring (svnicp_get_score_objective)."""
        obj = binding.ScoreObjectiveStruct(C.sizeof(binding.ScoreObjectiveStruct))
        self._check(self._L.svnicp_get_score_objective(self._h, C.byref(obj)), "svnicp_get_score_objective")
        return obj

    def _scores(self, out: np.ndarray, poses: np.ndarray) -> ParticleScores:
        o = self.get_score_objective()
        form = {v: k for k, v in self._SCORE_FORM.items()}[int(o.form)]
        sc = ParticleScores(out[:, 0].astype(np.int64), out[:, 1].astype(np.int64), out[:, 2].astype(np.int64),
                            out[:, 3].copy(), out[:, 4].copy(), out[:, 5].copy(), poses_3x4(poses))
        sc.form, sc.max_corr_dist, sc.huber_delta, sc.gicp_epsilon = form, float(o.max_corr_dist), float(o.huber_delta), float(o.epsilon)
        return sc

    def score_particles(self, max_corr_dist: float, form="point", huber_delta=None, gicp_epsilon=None) -> ParticleScores:
        """Score every particle's final pose through the registration's candidate table at the gate ``max_corr_dist``.
        ``form``: "point" (svnicp_score_particles, the default), or "plane" | "gicp" | "solved": the Huber-weighted plane or
        generalized-ICP residual, or whichever the registration ran with (svnicp_score_particles_objective); ``huber_delta``
        and ``gicp_epsilon`` None: the solver's own."""
        out, poses = np.zeros((self._P, 6), np.float64), np.zeros((self._P, 12), np.float64)
        dp = C.POINTER(C.c_double)
        if form == "point" and huber_delta is None and gicp_epsilon is None:
            self._check(self._L.svnicp_score_particles(self._h, float(max_corr_dist), out.ctypes.data_as(dp), poses.ctypes.data_as(dp)),
                        "svnicp_score_particles")
            return self._scores(out, poses)
        obj = self._objective(form, max_corr_dist, huber_delta, gicp_epsilon)
        self._check(self._L.svnicp_score_particles_objective(self._h, C.byref(obj), out.ctypes.data_as(dp), poses.ctypes.data_as(dp)),
                    "svnicp_score_particles_objective")
        return self._scores(out, poses)

    def get_particle_scores(self) -> ParticleScores:
        """The last scoring, whoever ran it (``score_particles``, or a registration with weighting on)."""
        out, poses = np.zeros((self._P, 6), np.float64), np.zeros((self._P, 12), np.float64)
        dp = C.POINTER(C.c_double)
        self._check(self._L.svnicp_get_particle_scores(self._h, out.ctypes.data_as(dp), poses.ctypes.data_as(dp)),
                    "svnicp_get_particle_scores")
        return self._scores(out, poses)

    # -- particle modes (include/svnicp_hip.h "particle modes") --------------------------------------------------------------
    def particle_modes(self, link_trans: float, link_rot: float, max_modes: int = 8, particles=None, weights=None) -> ParticleModes:
        """Group the particles into modes: the connected components of the graph that links two particles whose translations
        differ by at most ``link_trans`` (m) and whose rotation vectors by at most ``link_rot`` (rad), heaviest first.
        ``particles=None``: the last registration's set with its weights; else a [6, P] array of your own (no registration
        needed) with ``weights`` [P] or equal weights."""
        opt, o = binding.ModesOptStruct(), binding.ModesStruct()
        opt.struct_size, o.struct_size = C.sizeof(binding.ModesOptStruct), C.sizeof(binding.ModesStruct)
        opt.max_modes, opt.link_trans, opt.link_rot = int(max_modes), float(link_trans), float(link_rot)
        dp = C.POINTER(C.c_double)
        keep = []
        if particles is not None:
            x = np.ascontiguousarray(np.asarray(particles, np.float64).reshape(6, -1))
            keep.append(x)
            opt.particles6xP, opt.P = x.ctypes.data_as(dp), x.shape[1]
        if weights is not None:
            w = np.ascontiguousarray(np.asarray(weights, np.float64).reshape(-1))
            if particles is not None and w.size != opt.P:
                raise ValueError("particle_modes: weights must hold one entry per particle")
            keep.append(w)
            opt.weightsP = w.ctypes.data_as(dp)
        self._check(self._L.svnicp_particle_modes(self._h, C.byref(opt), C.byref(o)), "svnicp_particle_modes")
        self._modes_P = int(o.particles)
        return _modes_from_struct(o)

    def get_mode_labels(self) -> np.ndarray:
        """Per particle of the last ``particle_modes``: the rank of its mode (0 = the heaviest, ranks beyond ``n_reported``
        included), -1 for a non-finite particle."""
        out = np.full(max(getattr(self, "_modes_P", 0), 1), -1, np.int32)
        self._check(self._L.svnicp_get_mode_labels(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))), "svnicp_get_mode_labels")
        return out[:getattr(self, "_modes_P", 0)]

    def set_threshold(self, max_dist: float):
        self._check(self._L.svnicp_set_max_dist(self._h, float(max_dist)), "svnicp_set_max_dist")

    def stein_align(self) -> SteinICPState:
        return SteinICPState(self._check(self._L.svnicp_align(self._h), "svnicp_align"))

    def stein_align_async(self):
        self._check(self._L.svnicp_align_async(self._h), "svnicp_align_async")

    def synchronize(self):
        self._check(self._L.svnicp_synchronize(self._h), "svnicp_synchronize")

    def _getd(self, name: str, n: int) -> np.ndarray:
        out = np.zeros(n, np.float64)
        self._check(getattr(self._L, "svnicp_get_" + name)(self._h, out.ctypes.data_as(C.POINTER(C.c_double))),
                    "svnicp_get_" + name)
        return out

    def get_transformation(self) -> np.ndarray:
        return self._getd("transformation", 6)

    def get_distribution(self) -> np.ndarray:
        return self._getd("distribution", 6)

    def get_cov_matrix(self) -> np.ndarray:
        return self._getd("cov_matrix", 36)

    def get_particles(self) -> np.ndarray:
        return self._getd("particles", 6 * self._P)

    def get_particle_weight(self) -> np.ndarray:
        return self._getd("particle_weight", self._P)

    def get_particle_history(self) -> np.ndarray:
        out = np.zeros((int(self.config.iterations), 6 * self._P), np.float32)
        self._check(self._L.svnicp_get_particle_history(self._h, out.ctypes.data_as(C.POINTER(C.c_float))),
                    "svnicp_get_particle_history")
        return out

    def get_runtime(self) -> np.ndarray:
        """{knn_duration_, update_duration_, finish_iter_} (include/core/SVGDICP.h:94-96), seconds on the GPU.
        finish_iter_ is the reference's: the constructor's ``iterations`` unless an SVGD-mode early stop changed it."""
        return self._getd("runtime", 3)

    # -- test / bench taps ------------------------------------------------------------------
    def get_gpu_ms(self) -> np.ndarray:
        return self._getd("gpu_ms", 3)

    KERNEL_CLASSES = ("stage_a_knn", "k_build_table", "k_stein_search", "k_stein_accumulate", "k_reduce_partials",
                      "k_particle_update")  # include/svnicp_hip.h SVNICP_KERNEL_CLASSES

    def set_profile(self, on, classes=None):
        """Bracket kernel launches with hipEvents: every class (on=True) or only the named ``classes``."""
        v = int(bool(on))
        if on and classes:
            v = 0
            for k in classes:
                v |= 1 << (self.KERNEL_CLASSES.index(k) + 1)
        self._check(self._L.svnicp_set_profile(self._h, v), "svnicp_set_profile")

    def get_kernel_ms(self) -> dict:
        """{kernel class: (total ms in the last align, launches)} — hipEvents on the library's stream."""
        ms = np.zeros(len(self.KERNEL_CLASSES), np.float64)
        n = np.zeros(len(self.KERNEL_CLASSES), np.int32)
        self._check(self._L.svnicp_get_kernel_ms(self._h, ms.ctypes.data_as(C.POINTER(C.c_double)),
                                                 n.ctypes.data_as(C.POINTER(C.c_int32))), "svnicp_get_kernel_ms")
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(self.KERNEL_CLASSES)}

    def get_candidates(self) -> np.ndarray:
        out = np.zeros((self._B, self._K), np.int32)
        self._check(self._L.svnicp_get_candidates(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))),
                    "svnicp_get_candidates")
        return out

    def get_knn_fallbacks(self) -> int:
        """Queries the pre-filtered stage-A kernel handed to the streaming fallback (-1: streaming kernel only)."""
        v = C.c_int(0)
        self._check(self._L.svnicp_get_knn_fallbacks(self._h, C.byref(v)), "svnicp_get_knn_fallbacks")
        return int(v.value)

    def get_knn_fallback_rows(self) -> np.ndarray:
        """Source rows the pruned stage-A kernel handed to the streaming fallback (unordered)."""
        n = C.c_int(0)
        out = np.zeros(max(1, self._B), np.int32)
        self._check(self._L.svnicp_get_knn_fallback_rows(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size,
                                                         C.byref(n)), "svnicp_get_knn_fallback_rows")
        return out[:max(0, min(int(n.value), out.size))].copy()

    def get_knn_survivors(self) -> np.ndarray:
        """Per source point: targets that survived the f32 pre-filter of the pruned stage-A kernel (record_trace)."""
        out = np.zeros(self._B, np.int32)
        self._check(self._L.svnicp_get_knn_survivors(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))),
                    "svnicp_get_knn_survivors")
        return out

    def get_iterations_run(self) -> int:
        """Iterations the last align executed (the early stop may end it before ``iterations``)."""
        v = C.c_int(0)
        self._check(self._L.svnicp_get_iterations_run(self._h, C.byref(v)), "svnicp_get_iterations_run")
        return int(v.value)

    def get_ambiguous_steps(self) -> int:
        """Wave steps whose float32 nearest-of-K search had to be redone in float64 (-1: f64 kernel only)."""
        v = C.c_int(0)
        self._check(self._L.svnicp_get_ambiguous_steps(self._h, C.byref(v)), "svnicp_get_ambiguous_steps")
        return int(v.value)

    def get_ambiguous_pairs(self) -> int:
        """(point, particle) pairs the bf16 matrix-pipe search handed to its exact float64 pass (-1: another search kernel)."""
        v = C.c_int64(0)
        self._check(self._L.svnicp_get_ambiguous_pairs(self._h, C.byref(v)), "svnicp_get_ambiguous_pairs")
        return int(v.value)

    def get_candidate_dist2(self) -> np.ndarray:
        return self._getd("candidate_dist2", self._B * self._K).reshape(self._B, self._K)

    def get_trace(self, with_corr: bool = True) -> dict:
        I, P, B = int(self.config.iterations), self._P, self._B
        if self._mb > 0 and I > 0:
            B = self._mb      # mini-batch: corr is [I][P][batch_size]
        d = dict(H=np.zeros((I, P, 36)), b=np.zeros((I, P, 6)), newton=np.zeros((I, P, 6)), phi=np.zeros((I, P, 6)),
                 h=np.zeros(I))
        corr = np.zeros((I, P, B), np.int32) if with_corr else None
        dp = C.POINTER(C.c_double)
        rc = self._L.svnicp_get_trace(self._h, corr.ctypes.data_as(C.POINTER(C.c_int32)) if with_corr else None,
                                      d["H"].ctypes.data_as(dp), d["b"].ctypes.data_as(dp),
                                      d["newton"].ctypes.data_as(dp), d["phi"].ctypes.data_as(dp),
                                      d["h"].ctypes.data_as(dp))
        self._check(rc, "svnicp_get_trace")
        if with_corr:
            d["corr"] = corr
        return d


class SVNICP(_SolverBase):
    """svnicp::SVNICP (include/core/SVNICP.h:29-78)."""
    _mode = 0


class SVGDICP(_SolverBase):
    """svnicp::SVGDICP (include/core/SVGDICP.h:64-210), first-order mode."""
    _mode = 1
