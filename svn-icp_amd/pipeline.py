"""Caller glue around the solver: the scan-to-map sequence of the reference's odometry node, ROS-free.

SURVEY.md §8(f)-1.  Mirrors ``OdometryPipeline::ICP_processing`` for the ``estimator == ICP`` configuration
(/root/reference/svn-icp/src/core/OdometryPipeline.cpp:556-647): crop -> uniform down-sample (map cloud at
0.5·voxel, solver cloud at 1.5·voxel of that) -> constant-velocity pose prediction -> particle prior ->
local-map query -> solver -> pose = prediction · correction -> map insert.  The pre-/post-processing is host
code (numpy), exactly as it is host code (PCL / GTSAM / tsl::robin_map) in the reference; only the solver call
touches the GPU, through the same ``SVNICP`` class the parity tests use.

Parity status: *unpinned*.  PCL, GTSAM and rclcpp are absent from this image, so the reference's pipeline cannot
be built or run here and it holds no fixtures for these helpers; every function below restates the cited
reference lines and is covered by property tests (tests/test_pipeline_cpu.py).  Where PCL leaves an order
unspecified (hash-map iteration) this code picks a deterministic one and says so.
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass, field

import numpy as np

from .solver import SVNICP, ParticleWeightOpt, SteinICPParam, SteinICPState, initialize_particles

# particle prior bounds, OdometryPipeline.cpp:661-667
PRIOR_UB = np.array([0.3, 0.2, 0.1, 0.004, 0.004, 0.012])
PRIOR_LB = -PRIOR_UB


# ----------------------------------------------------------------------------- SE(3) helpers (gtsam::Pose3 semantics)
def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def so3_exp(w) -> np.ndarray:
    w = np.asarray(w, float)
    th = float(np.linalg.norm(w))
    K = _hat(w)
    if th < 1e-10:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + (math.sin(th) / th) * K + ((1.0 - math.cos(th)) / th ** 2) * K @ K


def so3_log(R) -> np.ndarray:
    R = np.asarray(R, float)
    c = max(-1.0, min(1.0, 0.5 * (np.trace(R) - 1.0)))
    th = math.acos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if th < 1e-10:
        return 0.5 * v
    return (th / (2.0 * math.sin(th))) * v


def se3_exp(xi) -> np.ndarray:
    """gtsam::Pose3::Expmap, xi = [omega, v]."""
    xi = np.asarray(xi, float)
    w, v = xi[:3], xi[3:]
    th = float(np.linalg.norm(w))
    K = _hat(w)
    if th < 1e-10:
        V = np.eye(3) + 0.5 * K
    else:
        V = np.eye(3) + ((1.0 - math.cos(th)) / th ** 2) * K + ((th - math.sin(th)) / th ** 3) * K @ K
    T = np.eye(4)
    T[:3, :3] = so3_exp(w)
    T[:3, 3] = V @ v
    return T


def se3_log(T) -> np.ndarray:
    """gtsam::Pose3::Logmap -> [omega, v]."""
    T = np.asarray(T, float)
    w = so3_log(T[:3, :3])
    th = float(np.linalg.norm(w))
    K = _hat(w)
    if th < 1e-10:
        Vinv = np.eye(3) - 0.5 * K
    else:
        Vinv = np.eye(3) - 0.5 * K + (1.0 / th ** 2 - (1.0 + math.cos(th)) / (2.0 * th * math.sin(th))) * K @ K
    return np.concatenate([w, Vinv @ T[:3, 3]])


def correction_to_pose(x6) -> np.ndarray:
    """svnicp::tensor2gtsamPose3 (src/core/ICPUtils.cpp:84-98): [x,y,z,rx,ry,rz] -> Pose3(Rot3::Expmap(r), t)."""
    x6 = np.asarray(x6, float).reshape(6)
    T = np.eye(4)
    T[:3, :3] = so3_exp(x6[3:])
    T[:3, 3] = x6[:3]
    return T


# ----------------------------------------------------------------------------- pre-processing
def crop_pointcloud(points: np.ndarray, min_range: float, max_range: float, scan_max_range: float = 0.0):
    """OdometryPipeline::crop_pointcloud (OdometryPipeline.cpp:692-704): keep min_range² < |p|² < max_range².
    Also returns the updated ``scan_max_range_`` — which the reference sets to the largest SQUARED norm seen
    (:699) and later uses as a length (:578); mirrored as is."""
    p = np.asarray(points, float)[:, :3]
    f = p.astype(np.float32)
    # float32 arithmetic, left to right, as pt.x*pt.x + pt.y*pt.y + pt.z*pt.z on pcl::PointXYZ (:698); the comparisons
    # promote the float to double (max_range_ is a double)
    n2 = ((f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2]).astype(np.float64)
    keep = (n2 < max_range * max_range) & (n2 > min_range * min_range)
    if n2.size and not np.all(np.isnan(n2)):
        scan_max_range = max(scan_max_range, float(np.nanmax(n2)))
    return p[keep], scan_max_range


def downsample_uniform(points: np.ndarray, radius: float) -> np.ndarray:
    """pcl::UniformSampling with ``setRadiusSearch(radius)`` (OdometryPipeline.cpp:684-690): a grid of leaf size
    ``radius`` anchored at floor(min/leaf); per occupied leaf the point closest to the leaf centre survives (first
    one wins ties).  PCL emits leaves in hash-map order; here: ascending leaf index."""
    p = np.asarray(points, float)
    if p.shape[0] == 0 or radius <= 0:
        return p.copy()
    inv = 1.0 / radius
    mn = np.floor(p.min(axis=0) * inv).astype(np.int64)
    mx = np.floor(p.max(axis=0) * inv).astype(np.int64)
    div = mx - mn + 1
    ijk = np.floor(p * inv).astype(np.int64) - mn
    leaf = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    centre = (ijk + mn + 0.5) * radius
    e = p - centre
    d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    order = np.lexsort((np.arange(p.shape[0]), d2, leaf))   # by leaf, then distance to the centre, then input order
    first = np.ones(order.size, bool)
    first[1:] = leaf[order][1:] != leaf[order][:-1]
    return p[order[first]]


# ----------------------------------------------------------------------------- deskew (motion compensation)
# OdometryPipeline::deskew_pointcloud (OdometryPipeline.cpp:357-447), run ahead of the crop when deskew_cloud_ is set and the
# pose buffer holds two poses (:551-554).  Restated with the float32 / float64 steps of the reference; the same expressions, in
# the same order, are in registration_pipeline.hpp (deskew_pointcloud) and csrc/scan_prep.hip (k_deskew_*).  Parity unpinned:
# GTSAM and Eigen are absent, so Pose3::Expmap / transformFrom and AngleAxis are written out (se3_exp's formulas).
KITTI_VERTICAL_ANGLE_OFFSET = (0.205 * math.pi) / 180.0     # :386
STAMP_DTYPES = (np.float64, np.float32, np.uint32)          # PointField FLOAT64 / FLOAT32 / UINT32 (:403-413)


def kitti_correct_and_stamp(points: np.ndarray):
    """The KITTI branch of deskew_pointcloud (:385-401) -> (corrected float32 [n,3], stamps float64 [n]).
    Per point: p in double; axis = (p × ẑ).normalized() = (y, −x, 0)/|·| (Eigen's normalized() leaves a zero vector as it is);
    AngleAxisd(0.205°, axis) * p stored back into the float32 point; stamp 0.5·(yaw/π + 1) with yaw = −atan2(y, x) of the
    float32 corrected coordinates, a float (std::atan2's float overload; formed here as the float64 atan2 rounded once to
    float32 — the correctly rounded value — identically in all three layers).  AngleAxis::toRotationMatrix() is Eigen 3's
    (sin·axis, (1−c)·axis, diagonal last); the matrix-vector product is summed left to right — unpinned (Eigen absent)."""
    f = np.asarray(points, np.float32)[:, :3]
    x, y, z = (f[:, d].astype(np.float64) for d in range(3))
    ax, ay = y.copy(), -x                                       # p × (0, 0, 1) = (y·1 − z·0, z·0 − x·1, x·0 − y·0)
    n2 = (ax * ax + ay * ay) + 0.0 * 0.0
    nz = n2 > 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        nrm = np.sqrt(n2)
        ax = np.where(nz, ax / nrm, ax)
        ay = np.where(nz, ay / nrm, ay)
    az = np.zeros_like(ax)
    a = KITTI_VERTICAL_ANGLE_OFFSET
    sn, c = math.sin(a), math.cos(a)
    sx, sy, sz = sn * ax, sn * ay, sn * az                      # sin_axis
    cx, cy, cz = (1.0 - c) * ax, (1.0 - c) * ay, (1.0 - c) * az   # cos1_axis
    R = [[cx * ax + c, cx * ay - sz, cx * az + sy],
         [cx * ay + sz, cy * ay + c, cy * az - sx],
         [cx * az - sy, cy * az + sx, cz * az + c]]
    out = np.empty((f.shape[0], 3), np.float32)
    for d in range(3):
        out[:, d] = ((R[d][0] * x + R[d][1] * y) + R[d][2] * z).astype(np.float32)
    with np.errstate(invalid="ignore"):
        yaw = (-np.arctan2(out[:, 1].astype(np.float64), out[:, 0].astype(np.float64))).astype(np.float32)
    stamps = 0.5 * (yaw.astype(np.float64) / math.pi + 1.0)
    return out, stamps


def _se3_exp_rows(xi: np.ndarray):
    """se3_exp for many twists at once ([n,6] -> R [n,9] row-major, t [n,3]), in the operation order of the C++ se3_exp
    (registration_pipeline.hpp: hat, mul3 summed left to right, lin3 = b·K + c·K², then the diagonal) and of the device."""
    w0, w1, w2 = xi[:, 0], xi[:, 1], xi[:, 2]
    z = np.zeros_like(w0)
    K = [z, -w2, w1, w2, z, -w0, -w1, w0, z]
    K2 = [(K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j] for i in range(3) for j in range(3)]
    th = np.sqrt((w0 * w0 + w1 * w1) + w2 * w2)
    small = th < 1e-10
    with np.errstate(invalid="ignore", divide="ignore"):
        sn, cs = np.sin(th), np.cos(th)
        ra = np.where(small, 1.0, sn / th)
        rb = np.where(small, 0.5, (1.0 - cs) / (th * th))
        vb = np.where(small, 0.5, (1.0 - cs) / (th * th))
        vc = np.where(small, 0.0, (th - sn) / (th * th * th))
    R = [ra * K[i] + rb * K2[i] for i in range(9)]
    V = [vb * K[i] + vc * K2[i] for i in range(9)]
    for i in (0, 4, 8):
        R[i] = R[i] + 1.0
        V[i] = V[i] + 1.0
    v0, v1, v2 = xi[:, 3], xi[:, 4], xi[:, 5]
    t = [(V[3 * i] * v0 + V[3 * i + 1] * v1) + V[3 * i + 2] * v2 for i in range(3)]
    return R, t


def deskew_pointcloud(points: np.ndarray, stamps, delta6, kitti: bool = False) -> np.ndarray:
    """OdometryPipeline::deskew_pointcloud (:357-447) -> float32 [n,3].
    stamps: the per-point field ``t`` / ``timestamp`` / ``time`` (:364-367) as float64, float32 or uint32, widened to double
    (:372-381); None = no such field: the vector stays zero, min == max and the raw frame comes back (:418).  kitti: the
    ``/kitti/velo/pointcloud`` branch (:385-401) replaces the stamps by kitti_correct_and_stamp.  min / max over the stamps
    (:414-417); min == max returns the UNMODIFIED frame (:418, in KITTI mode without the vertical correction); otherwise
    s = (t − min)/(max − min) (:419-423) and every point becomes Pose3::Expmap((s − 0.5)·δ).transformFrom(p) (:436-445), p the
    float32 point widened to double, the result rounded once to float32; δ = Pose3::Logmap(start⁻¹·finish) of the last two
    buffered poses (:427-432), [ω, v].  Deliberate deviation: non-finite stamps take no part in min / max (the reference's
    std::minmax_element answer depends on where a NaN sits) and their points come out as NaN, which the crop drops."""
    f = np.asarray(points, np.float32)[:, :3]
    delta6 = np.asarray(delta6, np.float64).reshape(6)
    if kitti:
        src, t = kitti_correct_and_stamp(f)
    else:
        if stamps is None:
            return f.copy()
        st = np.asarray(stamps)
        if st.dtype.type not in STAMP_DTYPES:
            raise ValueError(f"deskew_pointcloud: stamp type {st.dtype} (float64, float32 or uint32)")
        if st.shape != (f.shape[0],):
            raise ValueError("deskew_pointcloud: one stamp per point")
        src, t = f, st.astype(np.float64)
    fin = np.isfinite(t)
    if not fin.any():
        return f.copy()
    tmin, tmax = float(t[fin].min()), float(t[fin].max())
    if tmin == tmax:
        return f.copy()                                        # :418, *frame: the raw points
    with np.errstate(invalid="ignore"):
        s = (t - tmin) / (tmax - tmin)
    sp = np.where(fin, s - 0.5, 0.0)                           # (the non-finite ones are set to NaN below)
    R, tr = _se3_exp_rows(sp[:, None] * delta6[None, :])
    x, y, z = (src[:, d].astype(np.float64) for d in range(3))
    out = np.empty_like(src)
    for d in range(3):
        out[:, d] = (((R[3 * d] * x + R[3 * d + 1] * y) + R[3 * d + 2] * z) + tr[d]).astype(np.float32)
    out[~fin] = np.nan
    return out


# ----------------------------------------------------------------------------- range-image segmentation
# LeGO-LOAM's ImageProjection::cloudHandler (include/segmentation/ImageProjection.h), which OdometryPipeline::lidar_msg_cb runs
# on every raw scan when USE_Segmentation is set (OdometryPipeline.cpp:328-355); the pipeline consumes GetSegmentedCloudPure(),
# which returns segmentedCloud_ (:533-534).  The same steps, in the same float32 / float64 order, are in
# registration_pipeline.hpp (segment_scan) and csrc/range_segment.hip (svnicp_prep_segment).  Deliberate deviation: every
# atan2f / sinf / cosf of the reference is the float64 function of the float32 operands rounded once to float32 (the host
# libm's float functions are not correctly rounded and differ between libraries), so the three forms agree bit for bit.
SEG_EMPTY_RANGE = np.float32(-100000.0)      # rangeMat_ of an empty pixel (resetParameters)
SEG_INVALID_LABEL = 999999                   # labelMat_ of a component that failed the validity test (:523-529)
_F32 = np.float32


@dataclass
class SegParams:
    """ImageProjection's sensor and segmentation constants (:63-68, :112-118); float fields hold float32 values."""
    n_scan: int = 64
    horizon_scan: int = 2250
    ground_scan_ind: int = 7
    ang_res_x: float = float(_F32(360.0 / 2250.0))
    ang_res_y: float = float(_F32(26.8 / 63.0))
    ang_bottom: float = float(_F32(24.8))
    min_range: float = 1.0                   # sensorMinimumRange
    mount_angle: float = 0.0                 # sensorMountAngle
    segment_theta: float = float(_F32(60.0 / 180.0 * math.pi))
    valid_point_num: int = 5                 # segmentValidPointNum
    valid_line_num: int = 3                  # segmentValidLineNum

    def alphas(self):
        """(sin αx, cos αx, sin αy, cos αy) as float32, α = float(double(ang_res) / 180 · π) (:119-120)."""
        out = []
        for res in (self.ang_res_x, self.ang_res_y):
            a = float(_F32(float(_F32(res)) / 180.0 * math.pi))
            out += [_F32(math.sin(a)), _F32(math.cos(a))]
        return tuple(out)


def seg_params_struct(prm: SegParams):
    """SegParams -> struct svnicp_seg_params (ctypes)."""
    from .binding import SegParamsStruct
    import ctypes as C
    return SegParamsStruct(C.sizeof(SegParamsStruct), int(prm.n_scan), int(prm.horizon_scan), int(prm.ground_scan_ind),
                           float(prm.ang_res_x), float(prm.ang_res_y), float(prm.ang_bottom), float(prm.min_range),
                           float(prm.mount_angle), float(prm.segment_theta), int(prm.valid_point_num), int(prm.valid_line_num))


def _seg_preset(n, h, rx, ry, bottom, g):
    return SegParams(n_scan=n, horizon_scan=h, ground_scan_ind=g, ang_res_x=float(_F32(rx)), ang_res_y=float(_F32(ry)),
                     ang_bottom=float(_F32(bottom)))


# the sensor blocks of ImageProjection.h:46-110, each value as the header's expression evaluates it (double expression stored
# to float; "int / float(...)" is a float division)
SEG_PRESETS = {
    "VLP-16": _seg_preset(16, 1800, 0.2, 2.0, 15.0 + 0.1, 7),
    "HDL-32E": _seg_preset(32, 1800, 360.0 / float(_F32(1800)), 41.33 / float(_F32(31)), 30.67, 20),
    "HDL-64E": _seg_preset(64, 2250, 360.0 / float(_F32(2250)), 26.8 / float(_F32(63)), 24.8, 7),
    "VLS-128": _seg_preset(128, 1800, 0.2, 0.3, 25.0, 10),
    "RS-LIDAR-32": _seg_preset(32, 2000, 0.18, _F32(40) / _F32(31), 25.0, 2),
    "OS1-16": _seg_preset(16, 1024, 360.0 / float(_F32(1024)), 33.2 / float(_F32(15)), 16.6 + 0.1, 7),
    "OS1-64": _seg_preset(64, 1024, 360.0 / float(_F32(1024)), 33.2 / float(_F32(63)), 16.6 + 0.1, 15),
    "OS0-128": _seg_preset(128, 1024, 360.0 / float(_F32(1024)), _F32(90) / _F32(127), 45 + 0.1, 11),
}
SEG_PRESET_IDS = {name: k for k, name in enumerate(SEG_PRESETS)}   # SVNICP_SEG_* of include/svnicp_hip.h, same order


def _atan2_f32(y, x):
    """The project's atan2f: float64 atan2 of the float32 operands, rounded once (header: deliberate deviation)."""
    return np.arctan2(np.asarray(y, np.float32).astype(np.float64), np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def _deg_f32(a):
    """float(double(a * 180.0f) / M_PI) for float32 radians a."""
    return ((a * _F32(180.0)).astype(np.float64) / math.pi).astype(np.float32)


def _c_round(v):
    """C round(): half away from zero, exact for every double."""
    t = np.trunc(v)
    return t + np.where(np.abs(v - t) >= 0.5, np.sign(v), 0.0)


def _range_project(points, prm: SegParams):
    """projectPointCloud's per-point part (:240, :281-325) for float32 [n,3] points -> (takes part bool [n], row int64 [n],
    column int64 [n], range float32 [n]); row / column are 0 where the point takes no part.  The one statement of the
    projection on the host: segment_images and VoxelHashMap.clear_seen_through both go through it."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    N, H = int(prm.n_scan), int(prm.horizon_scan)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        finite = np.isfinite(p).all(axis=1)                                           # removeNaNFromPointCloud (:240)
        va = _deg_f32(_atan2_f32(z, np.sqrt(x * x + y * y)))
        q = (va + _F32(prm.ang_bottom)) / _F32(prm.ang_res_y)                         # float32; converted to size_t (x86-64)
        row_ok = (q > _F32(-1.0)) & (q < _F32(N))
        row = np.where(row_ok, np.trunc(np.where(row_ok, q, 0)), 0).astype(np.int64)
        h = _deg_f32(_atan2_f32(x, y))
        col = -_c_round((h.astype(np.float64) - 90.0) / float(_F32(prm.ang_res_x))) + float(H // 2)
        col = np.where(col >= H, col - H, col)
        col_ok = (col >= 0) & (col < H)
        rng = np.sqrt((x * x + y * y) + z * z)
        keep = finite & row_ok & col_ok & ~(rng < _F32(prm.min_range))
    return keep, np.where(keep, row, 0), np.where(keep, col, 0).astype(np.int64), rng


def _seg_project(points, prm: SegParams):
    """copyPointCloud + projectPointCloud (:240, :281-325) -> owner image (int64 [N·H], -1 = empty) and the float32 ranges
    of all points."""
    N, H = int(prm.n_scan), int(prm.horizon_scan)
    keep, row, col, rng = _range_project(points, prm)
    owner = np.full(N * H, -1, np.int64)
    idx = np.flatnonzero(keep)
    pix = row[idx] * H + col[idx]
    np.maximum.at(owner, pix, idx)                                                    # the last point in input order wins
    return owner, rng


def segment_images(points, params: SegParams | None = None):
    """ImageProjection's images for one scan -> (owner int32 [N,H] (winning input index, -1 empty), range float32 [N,H]
    (-100000 empty), ground int8 [N,H] (groundMat_), label int32 [N,H] (labelMat_ after cloudSegmentation))."""
    prm = params or SegParams()
    N, H, G = int(prm.n_scan), int(prm.horizon_scan), int(prm.ground_scan_ind)
    p = np.asarray(points, np.float32).reshape(-1, 3)
    owner, rng = _seg_project(p, prm)
    filled = owner >= 0
    o = np.where(filled, owner, 0)
    rimg = np.where(filled, rng[o] if p.shape[0] else SEG_EMPTY_RANGE, SEG_EMPTY_RANGE).astype(np.float32).reshape(N, H)
    xyz = (p[o] if p.shape[0] else np.zeros((N * H, 3), np.float32)).reshape(N, H, 3)
    filled = filled.reshape(N, H)
    # groundRemoval (:329-374), closed form of the loop's overwrites
    ground = np.zeros((N, H), np.int8)
    if G > 0:
        valid = filled[:G] & filled[1:G + 1]                                          # pair (r, r+1), r = 0..G-1
        d = xyz[1:G + 1] - xyz[:G]
        with np.errstate(invalid="ignore"):
            ang = _deg_f32(_atan2_f32(d[..., 2], np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])))
            flat = valid & (np.abs(ang - _F32(prm.mount_angle)) <= _F32(10))
        up = np.zeros((G + 1, H), bool); up[:G] = flat                               # pair (r, r+1) flat
        dn = np.zeros((G + 1, H), bool); dn[1:] = flat                               # pair (r-1, r) flat
        inval = np.zeros((G + 1, H), bool); inval[:G] = ~valid
        ground[:G + 1] = np.where(inval, -1, np.where(up | dn, 1, 0))
    label = np.where((ground == 1) | ~filled, -1, 0).astype(np.int32)
    # link predicates (symmetric): right (wrapping) and down neighbour
    sx, cx, sy, cy = prm.alphas()
    theta = _F32(prm.segment_theta)

    def link(ra, rb, s, c):
        d1, d2 = np.maximum(ra, rb), np.minimum(ra, rb)
        return _atan2_f32(d2 * s, d1 - d2 * c) > theta

    right = link(rimg, np.roll(rimg, -1, axis=1), sx, cx)
    down = np.zeros((N, H), bool)
    down[:-1] = link(rimg[:-1], rimg[1:], sy, cy)
    _label_components(label, right, down, prm)
    return owner.astype(np.int32).reshape(N, H), rimg, ground, label


def _label_components(label, right, down, prm: SegParams):
    """cloudSegmentation's seed loop and labelComponents (:379-383, :435-531), literally: row-major seeds, a FIFO queue,
    lineCountFlag set on push only."""
    N, H = label.shape
    lab = label.reshape(-1)   # view
    rl, dl = right.reshape(-1), down.reshape(-1)
    count = 1
    for seed in np.flatnonzero(lab == 0).tolist():
        if lab[seed] != 0:
            continue
        queue = [seed]
        pushed = [seed]
        lines = set()
        lab[seed] = count
        head = 0
        while head < len(queue):
            a = queue[head]; head += 1
            r, c = divmod(a, H)
            nbrs = []
            if r > 0:
                nbrs.append((a - H, dl[a - H]))
            b = r * H + (c + 1) % H
            nbrs.append((b, rl[a]))
            b = r * H + (c - 1) % H
            nbrs.append((b, rl[b]))
            if r < N - 1:
                nbrs.append((a + H, dl[a]))
            for b, ok in nbrs:
                if lab[b] != 0 or not ok:
                    continue
                lab[b] = count
                queue.append(b)
                pushed.append(b)
                lines.add(b // H)
        n = len(pushed)
        if n >= 30 or (n >= prm.valid_point_num and len(lines) >= prm.valid_line_num):
            count += 1
        else:
            lab[pushed] = SEG_INVALID_LABEL


def segment_scan(points, params: SegParams | None = None):
    """ImageProjection::cloudHandler -> segmentedCloud_ (what GetSegmentedCloudPure returns, :384-414): float32 [n,3] and the
    input index of every point (int64 [n]).  Pixels row-major; a pixel is kept when it belongs to a valid component or is
    ground, ground pixels only at j % 5 == 0 or within 5 columns of the image edges."""
    prm = params or SegParams()
    p = np.asarray(points, np.float32).reshape(-1, 3)
    owner, _, ground, label = segment_images(p, prm)
    H = int(prm.horizon_scan)
    j = np.arange(H)[None, :]
    g = ground == 1
    keep = ((label > 0) | g) & (label != SEG_INVALID_LABEL) & ~(g & (j % 5 != 0) & (j > 5) & (j < H - 5))
    src = owner[keep].astype(np.int64)
    return (p[src] if src.size else np.zeros((0, 3), np.float32)), src


# ----------------------------------------------------------------------------- local map
def transform_f32(cloud, T) -> np.ndarray:
    """pcl::transformPointCloud of float32 points with gtsam's DOUBLE Matrix4 (VoxelHashMap.cpp:23-25): every coordinate
    q = ((R0·x + R1·y) + R2·z) + t is formed in float64 from the widened float32 point and rounded once to float32 — the
    same expression as registration_pipeline.hpp and map_table.hip, so all three maps hold identical points.  (Parity with
    PCL itself is unpinned: PCL is not in this image.)"""
    c = np.asarray(cloud, np.float32).astype(np.float64)
    R = np.asarray(T, float)[:3, :3]
    t = np.asarray(T, float)[:3, 3]
    out = np.empty((c.shape[0], 3), np.float32)
    for d in range(3):
        out[:, d] = (((R[d, 0] * c[:, 0] + R[d, 1] * c[:, 1]) + R[d, 2] * c[:, 2]) + t[d]).astype(np.float32)
    return out


VISIBILITY_STATS = ("pixels_filled", "points_tested", "points_removed", "voxels_emptied")   # struct svnicp_visibility_stats


def check_visibility_options(sensor: SegParams, window, margin, max_range):
    """The refusals of svnicp_map_clear_seen_through -> (window_rows, window_cols, margin_abs, margin_rel, max_range), the three
    floats as float32."""
    N, H = int(sensor.n_scan), int(sensor.horizon_scan)
    if not (1 <= N <= 128 and H >= 1 and N * H <= 1 << 19):
        raise ValueError("clear_seen_through: need 1 <= n_scan <= 128, horizon_scan >= 1 and n_scan * horizon_scan <= 2^19")
    if not (np.isfinite(sensor.ang_res_x) and sensor.ang_res_x > 0 and np.isfinite(sensor.ang_res_y) and sensor.ang_res_y > 0
            and np.isfinite(sensor.ang_bottom) and np.isfinite(sensor.min_range)):
        raise ValueError("clear_seen_through: ang_res_x / ang_res_y must be finite and positive, ang_bottom / min_range finite")
    if len(tuple(window)) != 2 or len(tuple(margin)) != 2:
        raise ValueError("clear_seen_through: window is (rows, cols), margin is (abs, rel)")
    wr, wc = int(window[0]), int(window[1])
    if wr != window[0] or wc != window[1] or not (0 <= wr <= 4 and 0 <= wc <= 8):
        raise ValueError("clear_seen_through: window rows must be 0..4 and window cols 0..8")
    with np.errstate(over="ignore"):
        ma, mr, rmax = _F32(margin[0]), _F32(margin[1]), _F32(max_range)
    if not (np.isfinite(ma) and ma >= 0 and np.isfinite(mr) and mr >= 0):
        raise ValueError("clear_seen_through: margins must be finite and >= 0")
    if not (np.isfinite(rmax) and rmax > 0):
        raise ValueError("clear_seen_through: max_range must be finite and > 0")
    return wr, wc, ma, mr, rmax


def visibility_image(scan, sensor: SegParams) -> np.ndarray:
    """The minimum-range image of a scan: float32 [n_scan, horizon_scan], +inf = empty; a pixel keeps the smallest range of the
    points projectPointCloud puts into it (the conservative choice for a rule that deletes; order-independent)."""
    N, H = int(sensor.n_scan), int(sensor.horizon_scan)
    keep, row, col, rng = _range_project(scan, sensor)
    img = np.full(N * H, np.inf, np.float32)
    np.minimum.at(img, (row * H + col)[keep], rng[keep])
    return img.reshape(N, H)


def visibility_test(map_points, pose, img, sensor: SegParams, wr: int, wc: int, margin_abs, margin_rel, max_range):
    """The per-point rule of clear_seen_through for float32 map points [m,3] -> (reached the comparison bool [m], removed bool
    [m])."""
    N, H = img.shape
    T = np.asarray(pose, float)
    R, t = T[:3, :3], T[:3, 3]
    d = np.asarray(map_points, np.float32).astype(np.float64) - t[None, :]
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.stack([((R[0, c] * d[:, 0] + R[1, c] * d[:, 1]) + R[2, c] * d[:, 2]).astype(np.float32) for c in range(3)], 1)   # Rᵀd
        ok, row, col, rm = _range_project(s, sensor)
        tested = ok & ~(rm > _F32(max_range)) & (img[row, col] < np.inf)
        r_min = np.full(rm.shape[0], np.inf, np.float32)
        for dr in range(-wr, wr + 1):
            rr = row + dr
            inside = (rr >= 0) & (rr < N)                                             # rows do not wrap
            rr = np.clip(rr, 0, N - 1)
            for dc in range(-wc, wc + 1):
                v = np.where(inside, img[rr, (col + dc) % H], _F32(np.inf))           # columns wrap
                r_min = np.minimum(r_min, v)
        r_min = np.where(tested, r_min, _F32(0))
        remove = tested & (rm < r_min - np.maximum(_F32(margin_abs), _F32(margin_rel) * r_min))
    return tested, remove


# ----------------------------------------------------------------------------- candidate poses scored against the map
SCORE_FIELDS = ("located", "inliers", "sum_d2", "cost")   # SVNICP_MAP_SCORE_FIELDS of include/svnicp_hip.h
SCORE_MAX_POSES = 1 << 20
_VOX_OFF = 1 << 20                                        # voxel indices in [-2^20, 2^20)
_GRID_SLACK = 1e-9                                        # correction_grid: extent / step may miss an integer by a rounding


def pose_rows(poses) -> np.ndarray:
    """Poses as svnicp_map_score_poses takes them: [C, 12] float64, R row-major then t.  Accepts [C, 12] or [C, 4, 4]."""
    p = np.asarray(poses, np.float64)
    if p.ndim == 3 and p.shape[1:] == (4, 4):
        p = np.concatenate([p[:, :3, :3].reshape(-1, 9), p[:, :3, 3]], axis=1)
    p = np.ascontiguousarray(p.reshape(-1, 12))
    if not 1 <= p.shape[0] <= SCORE_MAX_POSES:
        raise ValueError("score_poses: need 1 <= C <= 2^20 poses")
    return p


def check_score_gate(gate, voxel_size) -> float:
    """The gate refusal of svnicp_map_score_poses -> thr2."""
    gate = float(gate)
    if not (np.isfinite(gate) and 0.0 < gate <= float(voxel_size)):
        raise ValueError("score_poses: the gate must be finite, > 0 and <= voxel_size (the 3x3x3 block holds the nearest point only "
                         "up to that gate)")
    return gate * gate


def correction_grid(extent6, step6):
    """The nodes of a search grid as corrections in the solver's parametrisation [x, y, z, rx, ry, rz] -> ([C, 6], index of the
    zero correction).  Per axis the offsets are k·step, k = -m..m, m = floor(extent / step) (a quotient within 1e-9 below an
    integer counts as that integer: 10° / 2.5° is 4); extent 0 fixes the axis.  Lexicographic order, x slowest."""
    ext, stp = np.asarray(extent6, np.float64).reshape(-1), np.asarray(step6, np.float64).reshape(-1)
    if ext.shape != (6,) or stp.shape != (6,):
        raise ValueError("correction_grid: extent and step hold six entries [x, y, z, rx, ry, rz]")
    if not (np.isfinite(ext).all() and (ext >= 0).all()):
        raise ValueError("correction_grid: extents must be finite and >= 0")
    m = []
    for e, s in zip(ext.tolist(), stp.tolist()):
        if e == 0.0:
            m.append(0)
            continue
        if not (np.isfinite(s) and s > 0):
            raise ValueError("correction_grid: an axis with a non-zero extent needs a finite step > 0")
        m.append(int(math.floor(e / s + _GRID_SLACK)))
    count = 1
    for k in m:
        count *= 2 * k + 1
    if count > SCORE_MAX_POSES:
        raise ValueError(f"correction_grid: {count} nodes, more than 2^20")
    axes = [np.arange(-k, k + 1, dtype=np.float64) * (s if k else 0.0) for k, s in zip(m, stp.tolist())]
    nodes = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 6)
    zero = 0
    for k in m:
        zero = zero * (2 * k + 1) + k
    return nodes, zero


def correction_poses(guess, corrections) -> np.ndarray:
    """guess @ correction_to_pose(x) for every correction x -> [C, 12] (pose_rows' layout): how a particle's total pose is
    composed, so a scored node can be handed to the solver as a particle unchanged."""
    G = np.asarray(guess, float)
    X = np.asarray(corrections, float).reshape(-1, 6)
    out = np.empty((X.shape[0], 12))
    for i, x in enumerate(X):
        T = G @ correction_to_pose(x)
        out[i, :9] = T[:3, :3].reshape(9)
        out[i, 9:] = T[:3, 3]
    return out


def seed_from_scores(scores, corrections, P: int):
    """-> (best correction [6], the P best corrections [P, 6], their node indices [P]), ordered by (cost, index): ties in cost go
    to the lower index."""
    sc = np.asarray(scores, np.float64).reshape(-1, len(SCORE_FIELDS))
    X = np.asarray(corrections, np.float64).reshape(-1, 6)
    if sc.shape[0] != X.shape[0]:
        raise ValueError("seed_from_scores: one score record per correction")
    if not 1 <= int(P) <= X.shape[0]:
        raise ValueError("seed_from_scores: need 1 <= P <= number of corrections")
    order = np.lexsort((np.arange(sc.shape[0]), sc[:, 3]))[:int(P)]
    return X[order[0]].copy(), X[order].copy(), order


# ----------------------------------------------------------------------------- the coarse-to-fine search
SEARCH_MAX_LEVELS = 8          # SVNICP_MAP_SEARCH_MAX_LEVELS
SEARCH_MAX_KEEP = 1024         # SVNICP_MAP_SEARCH_MAX_KEEP
_LAT_OFF = 1 << 20             # lattice entries lie in (-2^20, 2^20)


def search_lattice(extent6, step6, levels: int):
    """The lattice of svnicp_map_search_poses (include/svnicp_hip.h) -> (level-0 lattice int32 [C0, 6], fine step [6], m [6],
    active axes).  Nodes are integer vectors on the finest lattice: fine = step / 3^(levels-1) (0 on an axis without a usable
    step), m as correction_grid's, level 0 is j·3^(levels-1), j = -m..m, lexicographic with x slowest; an axis is active iff
    m >= 1.  Refuses what the C call refuses."""
    levels = int(levels)
    if not 1 <= levels <= SEARCH_MAX_LEVELS:
        raise ValueError("search_lattice: need 1 <= levels <= 8")
    ext, stp = np.asarray(extent6, np.float64).reshape(-1), np.asarray(step6, np.float64).reshape(-1)
    if ext.shape != (6,) or stp.shape != (6,):
        raise ValueError("search_lattice: extent and step hold six entries [x, y, z, rx, ry, rz]")
    if not (np.isfinite(ext).all() and (ext >= 0).all()):
        raise ValueError("search_lattice: extents must be finite and >= 0")
    top = 3 ** (levels - 1)
    m, fine, count = [], [], 1
    for e, s in zip(ext.tolist(), stp.tolist()):
        k = 0
        if e != 0.0:
            if not (np.isfinite(s) and s > 0):
                raise ValueError("search_lattice: an axis with a non-zero extent needs a finite step > 0")
            q = e / s + _GRID_SLACK
            k = int(math.floor(q)) if q < _LAT_OFF else _LAT_OFF
        if k * top + (top - 1) // 2 >= _LAT_OFF:
            raise ValueError("search_lattice: lattice overflow, m * 3^(levels-1) + (3^(levels-1) - 1) / 2 must stay below 2^20")
        m.append(k)
        fine.append(s / float(top) if (np.isfinite(s) and s > 0) else 0.0)
        count *= 2 * k + 1
        if count > SCORE_MAX_POSES:
            raise ValueError("search_lattice: a level holds more than 2^20 nodes")
    axes = [np.arange(-k, k + 1, dtype=np.int64) * top for k in m]
    lat = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 6).astype(np.int32)
    return lat, np.array(fine), m, [a for a in range(6) if m[a] >= 1]


def search_level_counts(m, levels: int, keep: int):
    """-> ([count per level], [kept per level]): count_0 = prod(2m+1), count_{l+1} = kept_l · 3^A, kept_l = min(keep, count_l).
    Refuses a keep outside 1..1024 and a level over 2^20 nodes."""
    if not 1 <= int(keep) <= SEARCH_MAX_KEEP:
        raise ValueError("search: need 1 <= keep <= 1024")
    children = 3 ** sum(1 for k in m if k >= 1)
    counts, kept = [], []
    for l in range(int(levels)):
        c = int(np.prod([2 * k + 1 for k in m], dtype=object)) if l == 0 else kept[-1] * children
        if c > SCORE_MAX_POSES:
            raise ValueError("search: a level holds more than 2^20 nodes")
        counts.append(c)
        kept.append(min(int(keep), c))
    return counts, kept


def search_children(kept_lattice, level: int, levels: int, active):
    """The nodes of level `level`+1 from the kept nodes of level `level` in rank order -> int32 [kept · 3^A, 6]: per parent the
    offsets {-1, 0, 1}·3^(levels-2-level) over the active axes, lexicographic with x slowest; child index = rank·3^A + offset."""
    K = np.asarray(kept_lattice, np.int64).reshape(-1, 6)
    scale = 3 ** (int(levels) - 2 - int(level))
    off = np.zeros((3 ** len(active), 6), np.int64)
    if active:
        grid = np.stack(np.meshgrid(*([np.array([-1, 0, 1])] * len(active)), indexing="ij"), -1).reshape(-1, len(active))
        off[:, list(active)] = grid * scale
    return (K[:, None, :] + off[None, :, :]).reshape(-1, 6).astype(np.int32)


def search_rank(records, lattice, keep: int) -> np.ndarray:
    """Indices of the min(keep, count) best nodes in rank order: ascending (cost, lattice vector lexicographic, x first)."""
    sc = np.asarray(records, np.float64).reshape(-1, len(SCORE_FIELDS))
    L = np.asarray(lattice, np.int64).reshape(-1, 6)
    if sc.shape[0] != L.shape[0]:
        raise ValueError("search_rank: one record per lattice vector")
    return np.lexsort((L[:, 5], L[:, 4], L[:, 3], L[:, 2], L[:, 1], L[:, 0], sc[:, 3]))[:min(int(keep), L.shape[0])]


def search_corrections(lattice, fine) -> np.ndarray:
    """x = (double)k · fine: the corrections of lattice vectors, one multiplication each."""
    return np.asarray(lattice, np.int32).reshape(-1, 6).astype(np.float64) * np.asarray(fine, np.float64).reshape(1, 6)


def search_zero_index(m) -> int:
    zero = 0
    for k in m:
        zero = zero * (2 * k + 1) + k
    return zero


def _check_search_guess(guess) -> np.ndarray:
    G = np.asarray(guess, np.float64)
    if G.shape != (4, 4) or not np.isfinite(G[:3]).all():
        raise ValueError("search_poses: the guess must be a finite 4x4 pose")
    return G


class DeviceVoxelHashMap:
    """The same map resident in HBM (svnicp_map_* of the C ABI, csrc/voxel_map.hip): ``add_pointcloud`` uploads only the new
    points, ``get_map`` leaves the selected points in device memory as float64 rows and returns (device pointer, count) for
    ``SVNICP.add_cloud_device_target``.  Voxels come out in ascending (x, y, z) index, points of a voxel in insertion order."""

    def __init__(self, voxel_size: float, max_range: float, max_points: int, device: int = 0, capacity_voxels: int = 0):
        import ctypes as C
        from . import binding
        self._C = C
        self._L = binding.load_library()
        self._h = C.c_void_p()
        rc = self._L.svnicp_map_create(int(device), float(voxel_size), float(max_range), int(max_points), int(capacity_voxels),
                                       C.byref(self._h))
        if rc != 0:
            raise binding.SvnIcpError(f"svnicp_map_create failed ({rc}): {self._L.svnicp_map_last_error(None).decode()}")
        self.bytes_uploaded = 0
        self._max_range = float(max_range)

    def _chk(self, rc, what):
        if rc != 0:
            from . import binding
            raise binding.SvnIcpError(f"{what} failed ({rc}): {self._L.svnicp_map_last_error(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.svnicp_map_destroy(self._h)
            self._h = self._C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        n = self._C.c_int64(0)
        self._chk(self._L.svnicp_map_size(self._h, self._C.byref(n)), "svnicp_map_size")
        return int(n.value)

    def empty(self) -> bool:
        return len(self) == 0

    def skipped_points(self) -> int:
        """Points add_pointcloud has not stored (outside +-2^20 voxels, or NaN) since creation."""
        n = self._C.c_int64(0)
        self._chk(self._L.svnicp_map_skipped_points(self._h, self._C.byref(n)), "svnicp_map_skipped_points")
        return int(n.value)

    def table_info(self):
        """-> (capacity in slots, tombstones after the last modifying call, table rebuilds since creation) (test tap)."""
        C = self._C
        cap, tomb, reb = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self._L.svnicp_map_table_info(self._h, C.byref(cap), C.byref(tomb), C.byref(reb)), "svnicp_map_table_info")
        return int(cap.value), int(tomb.value), int(reb.value)

    def add_pointcloud(self, cloud: np.ndarray, pose: np.ndarray):
        C = self._C
        pts = np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :3])
        T = np.asarray(pose, float)
        R = np.ascontiguousarray(T[:3, :3]).reshape(9)
        t = np.ascontiguousarray(T[:3, 3])
        dp = C.POINTER(C.c_double)
        self._chk(self._L.svnicp_map_add_cloud(self._h, pts.ctypes.data_as(C.c_void_p), pts.shape[0], 0, R.ctypes.data_as(dp),
                                               t.ctypes.data_as(dp)), "svnicp_map_add_cloud")
        self.bytes_uploaded += pts.nbytes

    def add_pointcloud_device(self, devptr: int, n: int, pose: np.ndarray):
        """add_pointcloud for float32 rows that already live in HBM (DevicePreprocessor)."""
        C = self._C
        T = np.asarray(pose, float)
        R = np.ascontiguousarray(T[:3, :3]).reshape(9)
        t = np.ascontiguousarray(T[:3, 3])
        dp = C.POINTER(C.c_double)
        self._chk(self._L.svnicp_map_add_cloud(self._h, C.c_void_p(int(devptr)), int(n), 1, R.ctypes.data_as(dp), t.ctypes.data_as(dp)),
                  "svnicp_map_add_cloud")

    def clear_seen_through(self, scan, pose, sensor: SegParams, window=(1, 1), margin=(0.3, 0.02), max_range: float | None = None) -> dict:
        """Drop the stored points the scan (sensor frame, at ``pose``) sees through (svnicp_map_clear_seen_through; the rule is
        VoxelHashMap.clear_seen_through's) -> the call's statistics.  ``max_range`` None = the map's own."""
        pts = np.ascontiguousarray(np.asarray(scan, np.float32)[:, :3])
        self.bytes_uploaded += pts.nbytes
        return self._clear_seen_through(pts.ctypes.data_as(self._C.c_void_p), pts.shape[0], 0, pose, sensor, window, margin, max_range)

    def clear_seen_through_device(self, devptr: int, n: int, pose, sensor: SegParams, window=(1, 1), margin=(0.3, 0.02),
                                  max_range: float | None = None) -> dict:
        """clear_seen_through for float32 rows that already live in HBM (DevicePreprocessor.cropped_ptr)."""
        return self._clear_seen_through(self._C.c_void_p(int(devptr)), int(n), 1, pose, sensor, window, margin, max_range)

    def _clear_seen_through(self, ptr, n, mem, pose, sensor, window, margin, max_range):
        from . import binding
        C = self._C
        T = np.asarray(pose, float)
        R = np.ascontiguousarray(T[:3, :3]).reshape(9)
        t = np.ascontiguousarray(T[:3, 3])
        dp = C.POINTER(C.c_double)
        prm = seg_params_struct(sensor)
        mr = self._max_range if max_range is None else max_range
        opt = binding.VisibilityOptStruct(C.sizeof(binding.VisibilityOptStruct), int(window[0]), int(window[1]), float(margin[0]),
                                          float(margin[1]), float(mr))
        st = binding.VisibilityStatsStruct()
        self._chk(self._L.svnicp_map_clear_seen_through(self._h, ptr, n, mem, R.ctypes.data_as(dp), t.ctypes.data_as(dp), C.byref(prm),
                                                        C.byref(opt), C.byref(st)), "svnicp_map_clear_seen_through")
        return {k: int(getattr(st, k)) for k in VISIBILITY_STATS}

    def get_map(self, pose=None, max_range: float | None = None):
        """-> (device pointer of float64 [M][3], M)"""
        C = self._C
        n = C.c_int64(0)
        if pose is None:
            self._chk(self._L.svnicp_map_query(self._h, None, -1.0, C.byref(n)), "svnicp_map_query")
        else:
            c = np.ascontiguousarray(np.asarray(pose, float)[:3, 3])
            self._chk(self._L.svnicp_map_query(self._h, c.ctypes.data_as(C.POINTER(C.c_double)), float(max_range), C.byref(n)),
                      "svnicp_map_query")
        return int(self._L.svnicp_map_points_devptr(self._h) or 0), int(n.value)

    def get_map_normals(self, normal_k: int = 16):
        """Normals of the rows of the last get_map, from the 27-voxel neighbourhoods of the map (svnicp_map_query_normals)
        -> (device pointer of float64 [M][3], rows with a normal).  A zero row means no normal."""
        C = self._C
        n = C.c_int64(0)
        self._chk(self._L.svnicp_map_query_normals(self._h, int(normal_k), C.byref(n)), "svnicp_map_query_normals")
        return int(self._L.svnicp_map_normals_devptr(self._h) or 0), int(n.value)

    def score_poses(self, cloud, poses, gate: float) -> np.ndarray:
        """How well the scan ``cloud`` (float32 [n,3], sensor frame) fits the map at each of ``poses`` ([C,12], [C,4,4] or a CUDA
        float64 tensor [C,12]; map <- sensor) -> [C, 4] {located, inliers, sum_d2, cost} (svnicp_map_score_poses; the host
        restatement is VoxelHashMap.score_poses).  ``gate`` is the inlier distance, at most the voxel size."""
        pts = np.ascontiguousarray(np.asarray(cloud, np.float32).reshape(-1, 3))
        self.bytes_uploaded += pts.nbytes
        return self._score_poses(pts.ctypes.data_as(self._C.c_void_p) if pts.shape[0] else None, pts.shape[0], 0, poses, gate)

    def score_poses_device(self, devptr: int, n: int, poses, gate: float) -> np.ndarray:
        """score_poses for float32 rows that already live in HBM (DevicePreprocessor.source_f32_ptr)."""
        return self._score_poses(self._C.c_void_p(int(devptr)), int(n), 1, poses, gate)

    def _score_poses(self, ptr, n, mem, poses, gate):
        C = self._C
        if _is_cuda_tensor(poses):
            import torch
            t = poses.detach().to(torch.float64).reshape(-1, 12).contiguous()
            torch.cuda.current_stream(t.device).synchronize()
            pptr, nposes, pmem = C.c_void_p(t.data_ptr()), int(t.shape[0]), 1
        else:
            t = pose_rows(poses)
            pptr, nposes, pmem = t.ctypes.data_as(C.c_void_p), t.shape[0], 0
        out = np.zeros((max(nposes, 0), len(SCORE_FIELDS)))
        self._chk(self._L.svnicp_map_score_poses(self._h, ptr, n, mem, pptr, nposes, pmem, float(gate),
                                                 out.ctypes.data_as(C.POINTER(C.c_double))), "svnicp_map_score_poses")
        return out

    def search_poses(self, cloud, guess, extent6, step6, levels: int, keep: int, gate: float) -> dict:
        """Coarse-to-fine search around ``guess`` (svnicp_map_search_poses; the host restatement is VoxelHashMap.search_poses):
        ``levels`` levels of scored nodes, each three times finer, the ``keep`` best of a level expanded.  -> the fields of
        struct svnicp_map_search as a dict; ``search_top`` and ``search_level`` read the rest."""
        pts = np.ascontiguousarray(np.asarray(cloud, np.float32).reshape(-1, 3))
        self.bytes_uploaded += pts.nbytes
        return self._search_poses(pts.ctypes.data_as(self._C.c_void_p) if pts.shape[0] else None, pts.shape[0], 0, guess, extent6, step6,
                                  levels, keep, gate)

    def search_poses_device(self, devptr: int, n: int, guess, extent6, step6, levels: int, keep: int, gate: float) -> dict:
        """search_poses for float32 rows that already live in HBM (DevicePreprocessor.source_f32_ptr)."""
        return self._search_poses(self._C.c_void_p(int(devptr)), int(n), 1, guess, extent6, step6, levels, keep, gate)

    def _search_poses(self, ptr, n, mem, guess, extent6, step6, levels, keep, gate):
        from . import binding
        C = self._C
        G = np.ascontiguousarray(np.asarray(guess, np.float64).reshape(4, 4))
        R, t = np.ascontiguousarray(G[:3, :3]), np.ascontiguousarray(G[:3, 3])
        opt = binding.MapSearchOptStruct()
        opt.extent[:] = [float(v) for v in np.asarray(extent6, np.float64).reshape(6)]
        opt.step[:] = [float(v) for v in np.asarray(step6, np.float64).reshape(6)]
        opt.levels, opt.keep, opt.max_corr_dist = int(levels), int(keep), float(gate)
        out = binding.MapSearchStruct()
        dp = C.POINTER(C.c_double)
        self._chk(self._L.svnicp_map_search_poses(self._h, ptr, n, mem, R.ctypes.data_as(dp), t.ctypes.data_as(dp), C.byref(opt),
                                                  C.byref(out)), "svnicp_map_search_poses")
        L = out.levels
        return {"levels": L, "active_axes": out.active_axes, "nodes_scored": int(out.nodes_scored),
                "level_count": [int(v) for v in out.level_count[:L]], "level_kept": [int(v) for v in out.level_kept[:L]],
                "fine_step": np.array(out.fine_step[:]), "best_lattice": np.array(out.best_lattice[:], np.int32),
                "best_correction": np.array(out.best_correction[:]), "best_pose": np.array(out.best_pose[:]),
                "best_record": np.array(out.best_record[:]), "zero_record": np.array(out.zero_record[:])}

    def search_top(self, cap: int = SEARCH_MAX_KEEP) -> dict:
        """The kept nodes of the last search's last level in rank order, at most ``cap`` -> {"lattice" int32 [N,6], "corrections"
        [N,6], "poses" [N,12], "records" [N,4]}."""
        C = self._C
        n = C.c_int(0)
        self._chk(self._L.svnicp_map_search_top(self._h, 0, None, None, None, None, C.byref(n)), "svnicp_map_search_top")
        N = min(int(cap), n.value)
        lat, x, P, rec = np.zeros((N, 6), np.int32), np.zeros((N, 6)), np.zeros((N, 12)), np.zeros((N, 4))
        dp = C.POINTER(C.c_double)
        self._chk(self._L.svnicp_map_search_top(self._h, N, lat.ctypes.data_as(C.POINTER(C.c_int32)), x.ctypes.data_as(dp),
                                                P.ctypes.data_as(dp), rec.ctypes.data_as(dp), C.byref(n)), "svnicp_map_search_top")
        return {"lattice": lat, "corrections": x, "poses": P, "records": rec}

    def search_level(self, level: int) -> dict:
        """Level ``level`` of the last search (test tap) -> {"lattice" int32 [C,6], "poses" [C,12], "records" [C,4], "kept": the
        indices of the kept nodes in rank order}."""
        C = self._C
        cnt, kept = C.c_int64(0), C.c_int(0)
        self._chk(self._L.svnicp_map_search_level(self._h, int(level), 0, None, None, None, None, C.byref(cnt), C.byref(kept)),
                  "svnicp_map_search_level")
        N = int(cnt.value)
        lat, P, rec, idx = np.zeros((N, 6), np.int32), np.zeros((N, 12)), np.zeros((N, 4)), np.zeros(kept.value, np.int32)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        self._chk(self._L.svnicp_map_search_level(self._h, int(level), N, lat.ctypes.data_as(ip), P.ctypes.data_as(dp), rec.ctypes.data_as(dp),
                                                  idx.ctypes.data_as(ip), C.byref(cnt), C.byref(kept)), "svnicp_map_search_level")
        return {"lattice": lat, "poses": P, "records": rec, "kept": idx}

    @property
    def scores_ptr(self) -> int:
        """Device pointer of the last scoring's float64 [C][4] records (0 before one)."""
        return int(self._L.svnicp_map_scores_devptr(self._h) or 0)

    def download_normals(self) -> np.ndarray:
        """The rows of the last get_map_normals as a host array (test tap)."""
        C = self._C
        n = C.c_int64(0)
        self._chk(self._L.svnicp_map_download_normals(self._h, None, 0, C.byref(n)), "svnicp_map_download_normals")
        out = np.zeros((int(n.value), 3))
        if out.size:
            self._chk(self._L.svnicp_map_download_normals(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), out.shape[0],
                                                          C.byref(n)), "svnicp_map_download_normals")
        return out

    def download(self) -> np.ndarray:
        """The rows of the last get_map as a host array (test tap)."""
        C = self._C
        n = C.c_int64(0)
        self._chk(self._L.svnicp_map_download(self._h, None, 0, C.byref(n)), "svnicp_map_download")
        out = np.zeros((int(n.value), 3))
        if out.size:
            self._chk(self._L.svnicp_map_download(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), out.shape[0], C.byref(n)),
                      "svnicp_map_download")
        return out


# stamp types and flags of svnicp_prep_scan_deskew (include/svnicp_hip.h)
SVNICP_STAMP_F64, SVNICP_STAMP_F32, SVNICP_STAMP_U32 = 0, 1, 2
SVNICP_DESKEW_KITTI = 1


def _is_cuda_tensor(x) -> bool:
    return type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False)


class DevicePreprocessor:
    """crop_pointcloud + the two uniform samplings of a scan on the device (svnicp_prep_* of the C ABI, csrc/scan_prep.hip):
    the raw float32 scan is uploaded once, the cropped cloud, the map cloud (float32) and the source cloud (float64 rows)
    stay in HBM.  Same points in the same order as crop_pointcloud / downsample_uniform above."""

    def __init__(self, device: int = 0):
        import ctypes as C
        from . import binding
        self._C = C
        self._L = binding.load_library()
        self._h = C.c_void_p()
        rc = self._L.svnicp_prep_create(int(device), C.byref(self._h))
        if rc:
            raise binding.SvnIcpError(f"svnicp_prep_create failed ({rc}): {self._L.svnicp_prep_last_error(None).decode()}")
        self.n_cropped = self.n_map = self.n_source = 0
        self.n_segmented = 0
        self.seg_shape = (0, 0)

    def close(self):
        if getattr(self, "_h", None):
            self._L.svnicp_prep_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def scan(self, points, min_range: float, max_range: float, voxel_size: float, scan_max_range: float, *, stamps=None,
             delta=None, kitti: bool = False) -> float:
        """-> updated scan_max_range; counts in n_cropped / n_map / n_source, clouds behind the *_ptr properties.
        With ``delta`` (Pose3::Logmap of start⁻¹·finish, [ω, v]) the scan is deskewed on the device first
        (svnicp_prep_scan_deskew, deskew_pointcloud's semantics): ``stamps`` float64 / float32 / uint32 per point, or None;
        ``kitti`` the KITTI branch.  ``points`` / ``stamps`` may be CUDA torch tensors (SVNICP_MEM_DEVICE: nothing uploaded)."""
        from . import binding
        C = self._C
        keep = []                                          # host arrays / tensors that must outlive the call
        pts_ptr, n, mem, up = self._cloud_arg(points, keep)
        smr = C.c_double(float(scan_max_range))
        nc, nm, ns = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        if delta is None:
            if stamps is not None or kitti:
                raise ValueError("DevicePreprocessor.scan: stamps / kitti need delta")
            rc = self._L.svnicp_prep_scan(self._h, pts_ptr, n, mem, float(min_range), float(max_range),
                                          float(voxel_size), C.byref(smr), C.byref(nc), C.byref(nm), C.byref(ns))
            what = "svnicp_prep_scan"
        else:
            st_ptr, st_type, st_up = self._stamps_arg(stamps, n, mem, keep)
            up += st_up
            d = np.ascontiguousarray(np.asarray(delta, np.float64).reshape(6))
            rc = self._L.svnicp_prep_scan_deskew(self._h, pts_ptr, st_ptr, st_type, n, mem, d.ctypes.data_as(C.POINTER(C.c_double)),
                                                 SVNICP_DESKEW_KITTI if kitti else 0, float(min_range), float(max_range),
                                                 float(voxel_size), C.byref(smr), C.byref(nc), C.byref(nm), C.byref(ns))
            what = "svnicp_prep_scan_deskew"
        if rc:
            raise binding.SvnIcpError(f"{what} failed ({rc}): {self._L.svnicp_prep_last_error(self._h).decode()}")
        self.n_cropped, self.n_map, self.n_source = int(nc.value), int(nm.value), int(ns.value)
        self.bytes_uploaded = up
        return float(smr.value)

    def _cloud_arg(self, points, keep):
        """-> (pointer, n, mem_kind, bytes that cross PCIe)"""
        C = self._C
        if _is_cuda_tensor(points):
            import torch
            t = points.detach().to(torch.float32)[:, :3].contiguous()
            keep.append(t)
            return C.c_void_p(t.data_ptr()), int(t.shape[0]), 1, 0
        pts = np.ascontiguousarray(np.asarray(points, np.float32)[:, :3])
        keep.append(pts)
        return pts.ctypes.data_as(C.c_void_p), int(pts.shape[0]), 0, pts.nbytes

    def _stamps_arg(self, stamps, n, mem, keep):
        """-> (pointer or None, SVNICP_STAMP_*, bytes that cross PCIe); stamps live where the points live (one mem_kind)"""
        C = self._C
        if stamps is None:
            return None, SVNICP_STAMP_F64, 0
        if _is_cuda_tensor(stamps):
            import torch
            codes = {torch.float64: SVNICP_STAMP_F64, torch.float32: SVNICP_STAMP_F32, torch.uint32: SVNICP_STAMP_U32}
            if mem != 1 or stamps.dtype not in codes:
                raise ValueError("DevicePreprocessor.scan: CUDA stamps need CUDA points and dtype float64 / float32 / uint32")
            t = stamps.detach().reshape(-1).contiguous()
            if t.shape[0] != n:
                raise ValueError("DevicePreprocessor.scan: one stamp per point")
            keep.append(t)
            return C.c_void_p(t.data_ptr()), codes[t.dtype], 0
        if mem != 0:
            raise ValueError("DevicePreprocessor.scan: host stamps need host points")
        st = np.ascontiguousarray(np.asarray(stamps).reshape(-1))
        codes = {np.dtype(np.float64): SVNICP_STAMP_F64, np.dtype(np.float32): SVNICP_STAMP_F32, np.dtype(np.uint32): SVNICP_STAMP_U32}
        if st.dtype not in codes:
            raise ValueError(f"DevicePreprocessor.scan: stamp type {st.dtype} (float64, float32 or uint32)")
        if st.shape[0] != n:
            raise ValueError("DevicePreprocessor.scan: one stamp per point")
        keep.append(st)
        return st.ctypes.data_as(C.c_void_p), codes[st.dtype], st.nbytes

    def download_deskewed(self) -> np.ndarray:
        """Every point of the last svnicp_prep_scan_deskew after the deskew, before the crop — float32 rows (test tap)."""
        from . import binding
        C = self._C
        n = C.c_int64(0)
        rc = self._L.svnicp_prep_download_deskewed(self._h, None, 0, C.byref(n))
        out = np.zeros((int(n.value), 3), np.float32)
        if rc == 0 and out.size:
            rc = self._L.svnicp_prep_download_deskewed(self._h, out.ctypes.data_as(C.c_void_p), out.shape[0], C.byref(n))
        if rc:
            raise binding.SvnIcpError(f"svnicp_prep_download_deskewed failed ({rc}): {self._L.svnicp_prep_last_error(self._h).decode()}")
        return out

    def segment(self, points, params: SegParams | None = None) -> int:
        """Range-image segmentation on the device (svnicp_prep_segment, segment_scan's semantics) -> n_segmented.  The
        segmented cloud (float32 rows) and the input index of each of its points stay in HBM behind ``segmented_ptr`` /
        ``segmented_index_ptr``; ``scan_device(segmented_ptr, n, …)`` pre-processes the cloud without a second upload.
        ``points`` may be a CUDA torch tensor (nothing uploaded); ``bytes_uploaded`` counts the upload."""
        from . import binding
        C = self._C
        keep = []
        pts_ptr, n, mem, up = self._cloud_arg(points, keep)
        prm = seg_params_struct(params or SegParams())
        out = C.c_int64(0)
        rc = self._L.svnicp_prep_segment(self._h, pts_ptr, n, mem, C.byref(prm), C.byref(out))
        if rc:
            raise binding.SvnIcpError(f"svnicp_prep_segment failed ({rc}): {self._L.svnicp_prep_last_error(self._h).decode()}")
        self.n_segmented = int(out.value)
        self.seg_shape = (int(prm.n_scan), int(prm.horizon_scan))
        self.bytes_uploaded = up
        return self.n_segmented

    def scan_device(self, ptr: int, n: int, min_range: float, max_range: float, voxel_size: float, scan_max_range: float, *,
                    delta=None, kitti: bool = False) -> float:
        """``scan`` of a float32 [n][3] cloud already in HBM (SVNICP_MEM_DEVICE), e.g. ``segmented_ptr``: nothing uploaded.
        With ``delta`` the cloud goes through svnicp_prep_scan_deskew without stamps (KITTI with ``kitti``)."""
        from . import binding
        C = self._C
        smr = C.c_double(float(scan_max_range))
        nc, nm, ns = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        if delta is None:
            rc = self._L.svnicp_prep_scan(self._h, C.c_void_p(int(ptr)), int(n), 1, float(min_range), float(max_range), float(voxel_size),
                                          C.byref(smr), C.byref(nc), C.byref(nm), C.byref(ns))
            what = "svnicp_prep_scan"
        else:
            d = np.ascontiguousarray(np.asarray(delta, np.float64).reshape(6))
            rc = self._L.svnicp_prep_scan_deskew(self._h, C.c_void_p(int(ptr)), None, SVNICP_STAMP_F64, int(n), 1,
                                                 d.ctypes.data_as(C.POINTER(C.c_double)), SVNICP_DESKEW_KITTI if kitti else 0,
                                                 float(min_range), float(max_range), float(voxel_size), C.byref(smr), C.byref(nc),
                                                 C.byref(nm), C.byref(ns))
            what = "svnicp_prep_scan_deskew"
        if rc:
            raise binding.SvnIcpError(f"{what} failed ({rc}): {self._L.svnicp_prep_last_error(self._h).decode()}")
        self.n_cropped, self.n_map, self.n_source = int(nc.value), int(nm.value), int(ns.value)
        self.bytes_uploaded = 0
        return float(smr.value)

    def download_segmented(self):
        """The last svnicp_prep_segment's cloud -> (float32 [n,3], input index int64 [n]) (test tap)."""
        from . import binding
        C = self._C
        n = C.c_int64(0)
        rc = self._L.svnicp_prep_download_segmented(self._h, None, None, 0, C.byref(n))
        xyz = np.zeros((int(n.value), 3), np.float32)
        idx = np.zeros(int(n.value), np.int32)
        if rc == 0 and xyz.size:
            rc = self._L.svnicp_prep_download_segmented(self._h, xyz.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p),
                                                        xyz.shape[0], C.byref(n))
        if rc:
            raise binding.SvnIcpError(f"svnicp_prep_download_segmented failed ({rc}): {self._L.svnicp_prep_last_error(self._h).decode()}")
        return xyz, idx.astype(np.int64)

    def download_seg_images(self):
        """The last svnicp_prep_segment's images -> (owner int32, range float32, ground int8, label int32), each [N,H], as
        segment_images returns them (test tap)."""
        from . import binding
        C = self._C
        N, H = self.seg_shape
        owner = np.zeros((N, H), np.int32); rng = np.zeros((N, H), np.float32)
        ground = np.zeros((N, H), np.int8); label = np.zeros((N, H), np.int32)
        rc = self._L.svnicp_prep_download_seg_images(self._h, owner.ctypes.data_as(C.c_void_p), rng.ctypes.data_as(C.c_void_p),
                                                     ground.ctypes.data_as(C.c_void_p), label.ctypes.data_as(C.c_void_p), N * H)
        if rc:
            raise binding.SvnIcpError(f"svnicp_prep_download_seg_images failed ({rc}): {self._L.svnicp_prep_last_error(self._h).decode()}")
        return owner, rng, ground, label

    @property
    def segmented_ptr(self) -> int:
        return int(self._L.svnicp_prep_segmented_devptr(self._h) or 0)

    @property
    def segmented_index_ptr(self) -> int:
        return int(self._L.svnicp_prep_segmented_index_devptr(self._h) or 0)

    @property
    def deskewed_ptr(self) -> int:
        return int(self._L.svnicp_prep_deskewed_devptr(self._h) or 0)

    @property
    def cropped_ptr(self) -> int:
        return int(self._L.svnicp_prep_cropped_devptr(self._h) or 0)

    @property
    def map_cloud_ptr(self) -> int:
        return int(self._L.svnicp_prep_map_cloud_devptr(self._h) or 0)

    @property
    def source_f32_ptr(self) -> int:
        return int(self._L.svnicp_prep_source_f32_devptr(self._h) or 0)

    @property
    def source_ptr(self) -> int:
        return int(self._L.svnicp_prep_source_devptr(self._h) or 0)

    def download(self, which: int) -> np.ndarray:
        """0 cropped, 1 map cloud, 2 source — float32 rows (test tap)."""
        C = self._C
        n = C.c_int64(0)
        self._L.svnicp_prep_download(self._h, int(which), None, 0, C.byref(n))
        out = np.zeros((int(n.value), 3), np.float32)
        if out.size:
            self._L.svnicp_prep_download(self._h, int(which), out.ctypes.data_as(C.c_void_p), out.shape[0], C.byref(n))
        return out


class VoxelHashMap:
    """svnicp::VoxelHashMap (src/core/VoxelHashMap.cpp:22-101): voxel -> at most ``max_points`` points, in insertion
    order; voxel index = coordinates / voxel_size truncated TOWARD ZERO (Eigen ``cast<int>``, :29); a voxel is dropped
    when its FIRST point is farther than ``max_range`` from the current position (:89-97), and is selected by
    ``get_map(pose, r)`` when its first point is closer than ``r`` (:48-58).  Points are float32 like pcl::PointXYZ."""

    def __init__(self, voxel_size: float, max_range: float, max_points: int):
        self.voxel_size = float(voxel_size)
        self.max_range = float(max_range)
        self.max_points = int(max_points)
        self._vox: dict[tuple, list] = {}

    def __len__(self):
        return len(self._vox)

    def empty(self) -> bool:
        return not self._vox

    def add_pointcloud(self, cloud: np.ndarray, pose: np.ndarray):
        T = np.asarray(pose, float)
        pts = transform_f32(cloud, T)
        idx = np.trunc(pts / np.float32(self.voxel_size)).astype(np.int64)
        # group by voxel, keeping the input order inside a voxel
        order = np.lexsort((np.arange(idx.shape[0]), idx[:, 2], idx[:, 1], idx[:, 0]))
        si = idx[order]
        brk = np.ones(order.size, bool)
        brk[1:] = np.any(si[1:] != si[:-1], axis=1)
        starts = np.flatnonzero(brk)
        ends = np.append(starts[1:], order.size)
        for s, e in zip(starts, ends):
            key = (int(si[s, 0]), int(si[s, 1]), int(si[s, 2]))
            lst = self._vox.get(key)
            if lst is None:
                lst = []
                self._vox[key] = lst
            room = self.max_points - len(lst)
            if room > 0:
                lst.extend(pts[order[s:min(e, s + room)]])
        self.remove_far(T[:3, 3])

    def remove_far(self, position):
        pos = np.asarray(position, float)
        r2 = self.max_range * self.max_range
        far = [k for k, v in self._vox.items() if float(np.sum((v[0].astype(float) - pos) ** 2)) > r2]
        for k in far:
            del self._vox[k]

    def clear_seen_through(self, scan, pose, sensor: SegParams, window=(1, 1), margin=(0.3, 0.02), max_range: float | None = None) -> dict:
        """Visibility-based clearing (include/svnicp_hip.h: svnicp_map_clear_seen_through): a stored point is
        deleted when the scan's beam in its direction returned from clearly behind it.  ``scan`` float32 [n,3] in the sensor
        frame, ``pose`` 4x4 map <- sensor, ``sensor`` the range-image geometry, ``window`` (rows, cols) the pixel window the
        minimum is taken over, ``margin`` (abs m, rel), ``max_range`` None = the map's own.  Stored point p: d = double(p) − t,
        s = float(Rᵀd) summed left to right, projected like a scan point; kept when it does not project, r_m > max_range or its
        own pixel is empty; else removed iff r_m < r_min − max(margin_abs, margin_rel·r_min) in float32.  Survivors keep their
        order, so the next survivor becomes the voxel's first point; an emptied voxel disappears.  -> statistics."""
        opt = check_visibility_options(sensor, window, margin, self.max_range if max_range is None else max_range)
        stats = dict.fromkeys(VISIBILITY_STATS, 0)
        pts = np.asarray(scan, np.float32).reshape(-1, 3)
        if pts.shape[0] == 0 or not self._vox:
            return stats
        img = visibility_image(pts, sensor)
        stats["pixels_filled"] = int(np.count_nonzero(img < np.inf))
        keys = list(self._vox)
        sizes = np.array([len(self._vox[k]) for k in keys])
        P = np.concatenate([np.asarray(self._vox[k], np.float32).reshape(-1, 3) for k in keys], 0)
        tested, remove = visibility_test(P, pose, img, sensor, *opt)
        stats["points_tested"] = int(np.count_nonzero(tested))
        stats["points_removed"] = int(np.count_nonzero(remove))
        ends = np.cumsum(sizes)
        hit = np.add.reduceat(remove.astype(np.int64), ends - sizes)
        for v in np.flatnonzero(hit).tolist():
            a, b = int(ends[v] - sizes[v]), int(ends[v])
            left = [q for q, r in zip(self._vox[keys[v]], remove[a:b]) if not r]
            if left:
                self._vox[keys[v]] = left
            else:
                del self._vox[keys[v]]
                stats["voxels_emptied"] += 1
        return stats

    def _score_table(self):
        """The map as score_poses searches it: (ascending packed keys of the voxels inside the index range, first point of each
        in ``pts``, points per voxel clamped to max_points, the points float64 [sum, 3])."""
        keys = sorted(k for k in self._vox if all(-_VOX_OFF <= v < _VOX_OFF for v in k))
        if not keys:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3))
        K = np.array(keys, np.int64).reshape(-1, 3) + _VOX_OFF
        packed = (K[:, 0] << 42) | (K[:, 1] << 21) | K[:, 2]           # ascending, as the tuples are
        cnt = np.array([min(len(self._vox[k]), self.max_points) for k in keys], np.int64)
        pts = np.concatenate([np.asarray(self._vox[k][:self.max_points], np.float32).reshape(-1, 3) for k in keys], 0).astype(np.float64)
        return packed, np.cumsum(cnt) - cnt, cnt, pts

    def score_poses(self, cloud, poses, gate: float) -> np.ndarray:
        """The numpy restatement of svnicp_map_score_poses (include/svnicp_hip.h) -> [C, 4] {located, inliers,
        sum_d2, cost}.  Row p at pose (R, t): c = float32(((R0·x + R1·y) + R2·z) + t) in float64 of the widened float32 row;
        voxel = trunc(c / float32(voxel_size)), valid in [-2^20, 2^20); candidates = the points of the 3x3x3 block of voxels;
        d2 = ((dx·dx) + dy·dy) + dz·dz in float64; located iff the block holds a point, inlier iff located and min d2 < gate²
        (strict); sum_d2 over the inliers, added in row order; cost = (sum_d2 + (n − inliers)·gate²) / n; n == 0: the cost is
        gate².  Searched through sorted keys (searchsorted), one pass per pose and neighbour offset."""
        thr2 = check_score_gate(gate, self.voxel_size)
        P = pose_rows(poses)
        f = np.asarray(cloud, np.float32).reshape(-1, 3)
        n = f.shape[0]
        out = np.zeros((P.shape[0], len(SCORE_FIELDS)))
        out[:, 3] = thr2
        if n == 0:
            return out
        packed, start, cnt, pts = self._score_table()
        x, y, z = (f[:, d].astype(np.float64) for d in range(3))
        vs = np.float32(self.voxel_size)
        offs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
        batch = max(1, 65536 // n)                                       # poses handled at once: rows of the batch are flattened
        for c0 in range(0, P.shape[0], batch):
            Pb = P[c0:c0 + batch]
            g = Pb.shape[0]
            with np.errstate(all="ignore"):
                c = np.stack([(((Pb[:, 3 * d, None] * x + Pb[:, 3 * d + 1, None] * y) + Pb[:, 3 * d + 2, None] * z)
                               + Pb[:, 9 + d, None]).astype(np.float32) for d in range(3)], 2).reshape(g * n, 3)
                q = np.trunc(c / vs)
                ok = np.all((q >= np.float32(-_VOX_OFF)) & (q < np.float32(_VOX_OFF)), axis=1)      # False for NaN and inf
            if packed.size == 0 or not ok.any():
                continue
            rows_ok = np.flatnonzero(ok)                                 # flat index = pose in the batch * n + row
            v = q[rows_ok].astype(np.int64) + _VOX_OFF
            key0 = (v[:, 0] << 42) | (v[:, 1] << 21) | v[:, 2]
            by_key = np.argsort(key0)                                    # neighbouring queries: the bisections share their path
            rows_ok, v, key0 = rows_ok[by_key], v[by_key], key0[by_key]
            inside = [{-1: v[:, d] > 0, 0: True, 1: v[:, d] < 2 * _VOX_OFF - 1} for d in range(3)]   # outside: no such voxel
            rr, vv = [], []
            for o in offs:
                key = key0 + ((o[0] << 42) + (o[1] << 21) + o[2])
                pos = np.minimum(np.searchsorted(packed, key), packed.size - 1)
                hit = (packed[pos] == key) & inside[0][o[0]] & inside[1][o[1]] & inside[2][o[2]]
                rr.append(rows_ok[hit]); vv.append(pos[hit])
            rr, vv = np.concatenate(rr), np.concatenate(vv)
            if rr.size == 0:
                continue
            order = np.argsort(rr, kind="stable")
            rr, vv = rr[order], vv[order]
            cn = cnt[vv]
            seg = np.cumsum(cn) - cn
            idx = np.repeat(start[vv] - seg, cn) + np.arange(int(cn.sum()))
            rep = np.repeat(rr, cn)
            d = pts[idx] - c[rep].astype(np.float64)
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            first = np.flatnonzero(np.r_[True, rep[1:] != rep[:-1]])
            dmin = np.minimum.reduceat(d2, first)                                                    # per located row, flat rows ascending
            cut = np.searchsorted(rep[first], np.arange(g + 1) * n)                                  # the located rows of each pose
            for k in range(g):
                dk = dmin[cut[k]:cut[k + 1]]
                inl = dk[dk < thr2]
                sm = float(np.add.accumulate(inl)[-1]) if inl.size else 0.0                          # sequential, in row order
                out[c0 + k] = (dk.size, inl.size, sm, (sm + (n - inl.size) * thr2) / n)
        return out

    def search_poses(self, cloud, guess, extent6, step6, levels: int, keep: int, gate: float) -> dict:
        """The numpy restatement of svnicp_map_search_poses (include/svnicp_hip.h), built on score_poses and the
        lattice helpers -> the fields DeviceVoxelHashMap.search_poses returns, plus "top" (search_top's dict) and "level": per
        level {"lattice", "corrections", "poses", "records", "kept"} (search_level's dict)."""
        check_score_gate(gate, self.voxel_size)
        G = _check_search_guess(guess)
        lat, fine, m, active = search_lattice(extent6, step6, levels)
        counts, kepts = search_level_counts(m, levels, keep)
        rows = np.asarray(cloud, np.float32).reshape(-1, 3)
        level = []
        for l in range(int(levels)):
            if l > 0:
                prev = level[-1]
                lat = search_children(prev["lattice"][prev["kept"]], l - 1, levels, active)
            x = search_corrections(lat, fine)
            poses = correction_poses(G, x)
            rec = self.score_poses(rows, poses, gate)
            level.append({"lattice": lat, "corrections": x, "poses": poses, "records": rec,
                          "kept": search_rank(rec, lat, keep).astype(np.int32)})
            assert lat.shape[0] == counts[l] and level[-1]["kept"].shape[0] == kepts[l]
        last = level[-1]
        order = last["kept"]
        top = {"lattice": last["lattice"][order], "corrections": last["corrections"][order], "poses": last["poses"][order],
               "records": last["records"][order]}
        return {"levels": int(levels), "active_axes": len(active), "nodes_scored": int(sum(counts)), "level_count": counts,
                "level_kept": kepts, "fine_step": fine, "best_lattice": top["lattice"][0].copy(),
                "best_correction": top["corrections"][0].copy(), "best_pose": top["poses"][0].copy(),
                "best_record": top["records"][0].copy(), "zero_record": level[0]["records"][search_zero_index(m)].copy(),
                "top": top, "level": level}

    def get_map(self, pose=None, max_range: float | None = None) -> np.ndarray:
        if not self._vox:
            return np.zeros((0, 3))
        if pose is None:
            chunks = [np.asarray(v) for v in self._vox.values()]
        else:
            pos = np.asarray(pose, float)[:3, 3]
            r2 = max_range * max_range
            chunks = [np.asarray(v) for v in self._vox.values() if float(np.sum((v[0].astype(float) - pos) ** 2)) < r2]
        if not chunks:
            return np.zeros((0, 3))
        return np.concatenate(chunks, 0).astype(np.float64)


# ----------------------------------------------------------------------------- pose prediction
def pose_prediction(poses: list, times: list, new_time: float) -> np.ndarray:
    """OdometryPipeline::pose_prediction (OdometryPipeline.cpp:706-737): constant twist between the last two poses,
    scaled by the time ratio; identity / last pose while fewer than two poses exist."""
    if len(poses) == 0:
        return np.eye(4)
    if len(poses) < 2:
        return np.array(poses[-1], float)
    T0, T1 = np.asarray(poses[-2], float), np.asarray(poses[-1], float)
    dt = times[-1] - times[-2]
    delta = np.linalg.inv(T0) @ T1
    ratio = (new_time - times[-1]) / dt
    return T1 @ se3_exp(ratio * se3_log(delta))


# ----------------------------------------------------------------------------- the sequence
@dataclass
class PipelineConfig:
    """Field names follow the node's parameters (OdometryPipeline.cpp parameter block; config/*.yaml)."""
    min_range: float = 1.0
    max_range: float = 100.0
    voxel_size: float = 1.0
    map_voxel_size: float = 1.0
    map_voxel_max_points: int = 20
    map_range: float = 100.0
    particle_count: int = 128
    gpu_map: bool = False          # keep the local map in HBM (DeviceVoxelHashMap): the target never crosses PCIe
    gpu_prep: bool = False         # with gpu_map: crop and both uniform samplings on the device (DevicePreprocessor): the raw scan is uploaded, no host pass over the points
    deskew: bool = False           # deskew_cloud (config/ICP_parameters.yaml:18): motion compensation from the last two poses ahead of the crop (:551-554)
    kitti: bool = False            # with deskew: the KITTI branch (cloud_topic "/kitti/velo/pointcloud", :385-401) instead of per-point stamps
    segmentation: bool = False     # USE_Segmentation (OdometryPipeline.cpp:180, :328-355): range-image segmentation of the raw scan first
    seg_params: SegParams = field(default_factory=SegParams)   # the sensor of ImageProjection.h (SEG_PRESETS); HDL-64E by default
    solver: SteinICPParam = field(default_factory=lambda: SteinICPParam(iterations=20, lr=1.0, max_dist=1.0, KNN_count=100))
    seed: int = 0
    eval_dist: float = 0.0         # > 0: every registered scan is evaluated at its result pose with this inlier gate (svnicp_evaluate) before the map update; 0 = off, no call is made
    information: str = "off"       # "point" | "plane": after that evaluate, the Gauss-Newton information matrix of its pairs (svnicp_eval_information) in ScanResult.information; needs eval_dist > 0.  "gicp": the same in the generalized-ICP objective (svnicp_eval_information_gicp, with solver.gicp_epsilon); only with solver.residual == "gicp".  "off": no call is made
    info_huber: float = float("inf")   # with information: its Huber delta (+inf = unweighted)
    weight_dist: float = 0.0       # > 0: every registration ends with one scoring of the particles at this gate and soft-min weights (svnicp_set_particle_weighting): correction, variance, cov and weights are the weighted figures; 0 = off, the reference's equal weights
    weight_temperature: float = 0.0   # with weight_dist: the soft-min temperature in m^2, > 0
    weight_cost: str = "point"     # with weight_dist: "point" = the mean truncated squared point distance (no call changes); "solved" = the residual the registration runs with, plane or generalized-ICP, with the solver's huber_delta and epsilon (svnicp_set_particle_weighting_objective)
    map_normals: bool = False      # with gpu_map and solver.residual == "plane" or "gicp" (whose source normals stay the solver's own pass): the target's normals come from the map's own voxels (svnicp_map_query_normals) instead of the solver's pass over the target
    mode_link: tuple | None = None  # (link_trans m, link_rot rad): after every registration the particles are grouped into modes (svnicp_particle_modes) in ScanResult.modes; None = off, no call is made
    mode_max: int = 8              # with mode_link: modes reported in full (1..32)
    mode_select: str = "mean"      # "heaviest": the correction is the first mode's mean instead of the global mean, and the pose, the evaluate, the information and the map update follow it; needs mode_link
    clear_seen_through: tuple | None = None   # (window_rows, window_cols, margin_abs m, margin_rel): after every successful registration the map points the cropped scan sees through at the result pose are dropped (clear_seen_through, sensor = seg_params) right before the map update, count in ScanResult.cleared; None = off, no call is made
    clear_max_range: float = 0.0   # with clear_seen_through: map points farther than this from the sensor are left alone; 0 = max_range
    seed_grid: tuple | None = None  # (extent6, step6) of correction_grid: before every registration the scan's rows are scored against the map at the grid's nodes around the prediction (score_poses), result in ScanResult.seed; None = off, no call is made
    seed_gate: float = 0.0         # with seed_grid: the inlier gate of that scoring, at most map_voxel_size; 0 = map_voxel_size
    seed_mode: str = "best"        # "best": the registration's initial mean becomes prediction · correction_to_pose(best node), the particles are drawn as ever; "top": the mean stays the prediction and the particles are the particle_count best nodes

    seed_levels: int = 1           # with seed_grid: > 1 = coarse-to-fine (search_poses): seed_grid is level 0, every further level is three times finer and expands the seed_keep best nodes of the one before; 1 = the flat grid
    seed_keep: int = 8             # with seed_levels > 1: nodes of a level that are expanded ("top": at least particle_count are kept)
    seed_skip_fitness: float = 0.0  # with seed_grid: > 0 = the prediction alone is scored first, and with inliers / rows at or above this no search is made and the registration starts as without seeding; 0 = every scan is searched
    prior_sigma: tuple | None = None   # (sx, sy, sz m, srx, sry, srz rad) > 0: every registration runs with a Gaussian prior on the correction (svnicp_set_pose_prior) centred on the registration's initial mean — the zero correction; with seed_mode "best" that is the SEEDED mean, not the prediction — with information prior_point_sigma^2 diag(1 / sigma^2), and ScanResult.prior_chi2 is filled; None = off, no call is made
    prior_point_sigma: float = 1.0     # with prior_sigma: the point noise in m that turns the metric sigmas into the cost's units (Lambda = sigma_pt^2 Sigma^-1)

    def prior_information(self) -> np.ndarray:
        """Lambda [6, 6] of prior_sigma and prior_point_sigma."""
        return np.diag(float(self.prior_point_sigma) ** 2 / np.asarray(self.prior_sigma, np.float64) ** 2)

    def seed_nodes(self):
        """-> (corrections [C, 6], index of the zero correction) of seed_grid."""
        return correction_grid(*self.seed_grid)

    def seed_search_keep(self) -> int:
        """The `keep` of the coarse-to-fine search: "top" needs particle_count nodes out of the last level."""
        return max(int(self.seed_keep), int(self.particle_count)) if self.seed_mode == "top" else int(self.seed_keep)

    def __post_init__(self):
        if self.seed_mode not in ("best", "top"):
            raise ValueError('PipelineConfig: seed_mode must be "best" or "top"')
        if not (isinstance(self.seed_levels, int) and 1 <= self.seed_levels <= SEARCH_MAX_LEVELS):
            raise ValueError("PipelineConfig: seed_levels must be an integer in 1..8")
        if not (isinstance(self.seed_keep, int) and 1 <= self.seed_keep <= SEARCH_MAX_KEEP):
            raise ValueError("PipelineConfig: seed_keep must be an integer in 1..1024")
        if not (np.isfinite(self.seed_skip_fitness) and 0 <= self.seed_skip_fitness <= 1):
            raise ValueError("PipelineConfig: seed_skip_fitness must lie in [0, 1] (0 = every scan is searched)")
        if self.seed_grid is None and (self.seed_levels > 1 or self.seed_skip_fitness > 0):
            raise ValueError("PipelineConfig: seed_levels > 1 and seed_skip_fitness > 0 need seed_grid (level 0 of the search)")
        if self.seed_grid is not None and self.seed_levels > 1:
            if len(tuple(self.seed_grid)) != 2:
                raise ValueError("PipelineConfig: seed_grid must be (extent6, step6)")
            if self.seed_mode == "top" and self.particle_count > SEARCH_MAX_KEEP:
                raise ValueError('PipelineConfig: seed_mode "top" with seed_levels > 1 hands over at most 1024 nodes (particle_count)')
            _, _, m, _ = search_lattice(*self.seed_grid, self.seed_levels)          # refuses what the search itself refuses
            counts, _ = search_level_counts(m, self.seed_levels, self.seed_search_keep())
            if self.seed_mode == "top" and counts[-1] < self.particle_count:
                raise ValueError('PipelineConfig: seed_mode "top" needs at least particle_count nodes in the last level of the search')
        if not (np.isfinite(self.seed_gate) and 0 <= self.seed_gate <= self.map_voxel_size):
            raise ValueError("PipelineConfig: seed_gate must be finite, >= 0 (0 = map_voxel_size) and at most map_voxel_size")
        if self.seed_grid is not None:
            if len(tuple(self.seed_grid)) != 2:
                raise ValueError("PipelineConfig: seed_grid must be (extent6, step6)")
            nodes, _ = self.seed_nodes()                       # refuses steps <= 0 with an extent and more than 2^20 nodes
            if self.seed_mode == "top" and self.seed_levels == 1 and nodes.shape[0] < self.particle_count:
                raise ValueError('PipelineConfig: seed_mode "top" needs at least particle_count nodes in seed_grid')
        if self.clear_seen_through is not None:
            if len(tuple(self.clear_seen_through)) != 4:
                raise ValueError("PipelineConfig: clear_seen_through must be (window_rows, window_cols, margin_abs, margin_rel)")
            if not (np.isfinite(self.clear_max_range) and self.clear_max_range >= 0):
                raise ValueError("PipelineConfig: clear_max_range must be finite and >= 0 (0 = max_range)")
            w0, w1, m0, m1 = self.clear_seen_through
            check_visibility_options(self.seg_params, (w0, w1), (m0, m1), self.clear_max_range or self.max_range)
        if self.mode_select not in ("mean", "heaviest"):
            raise ValueError('PipelineConfig: mode_select must be "mean" or "heaviest"')
        if self.mode_link is not None:
            if len(tuple(self.mode_link)) != 2 or not all(np.isfinite(v) and v >= 0 for v in self.mode_link):
                raise ValueError("PipelineConfig: mode_link must be (link_trans, link_rot), both finite and >= 0")
            if not 1 <= int(self.mode_max) <= 32:
                raise ValueError("PipelineConfig: mode_max must lie in 1..32")
        elif self.mode_select == "heaviest":
            raise ValueError('PipelineConfig: mode_select "heaviest" needs mode_link (the modes are what it selects from)')
        if not (np.isfinite(self.weight_dist) and self.weight_dist >= 0):
            raise ValueError("PipelineConfig: weight_dist must be finite and >= 0 (0 = equal weights)")
        if self.weight_dist > 0 and not (np.isfinite(self.weight_temperature) and self.weight_temperature > 0):
            raise ValueError("PipelineConfig: weight_dist > 0 needs a finite weight_temperature > 0 (m^2)")
        if self.weight_cost not in ("point", "solved"):
            raise ValueError('PipelineConfig: weight_cost must be "point" or "solved"')
        if self.weight_cost != "point" and not self.weight_dist > 0:
            raise ValueError('PipelineConfig: weight_cost "solved" needs weight_dist > 0 (it names the cost of that weighting)')
        if self.information not in ("off", "point", "plane", "gicp"):
            raise ValueError('PipelineConfig: information must be "off", "point" or "plane"')
        if self.information == "gicp" and self.solver.residual != "gicp":
            raise ValueError('PipelineConfig: information "gicp" needs solver.residual == "gicp" (only then does the context hold the normals of both clouds)')
        if self.information != "off" and not self.eval_dist > 0:
            raise ValueError("PipelineConfig: information needs eval_dist > 0 (its rows are the evaluate's)")
        if self.information != "off" and not self.info_huber > 0:
            raise ValueError("PipelineConfig: info_huber must be > 0 (+inf = unweighted)")
        if self.prior_sigma is not None:
            if len(tuple(self.prior_sigma)) != 6 or not all(np.isfinite(v) and v > 0 for v in self.prior_sigma):
                raise ValueError("PipelineConfig: prior_sigma must be six finite standard deviations > 0 (m, m, m, rad, rad, rad)")
            if not (np.isfinite(self.prior_point_sigma) and self.prior_point_sigma > 0):
                raise ValueError("PipelineConfig: prior_point_sigma must be finite and > 0 (m)")
        if self.map_normals and not self.gpu_map:
            raise ValueError("PipelineConfig: map_normals needs gpu_map=True (the normals are computed from the device map)")
        if self.map_normals and self.solver.residual not in ("plane", "gicp"):
            raise ValueError('PipelineConfig: map_normals needs solver.residual == "plane" or "gicp" (point mode uses no normals)')


@dataclass
class ScanResult:
    stamp: float
    pose: np.ndarray            # 4x4, map <- sensor
    initial_guess: np.ndarray   # 4x4
    correction: np.ndarray | None = None     # [6] solver mean (x,y,z,rx,ry,rz)
    variance: np.ndarray | None = None       # [6]
    cov: np.ndarray | None = None            # [36]
    particles: np.ndarray | None = None      # [6*P]
    weights: np.ndarray | None = None        # [P]
    preprocessing_s: float = 0.0
    align_s: float = 0.0
    state: int | None = None
    with_normal: int | None = None           # cfg.map_normals: target rows the map gave a normal
    fitness: float | None = None             # cfg.eval_dist > 0: inliers / source rows of the result pose against the whole target
    inlier_rmse: float | None = None         # … sqrt(mean d2) over the inliers
    plane_rmse: float | None = None          # … sqrt(mean r2) over the inliers whose target has a normal; None without normals
    plane_inliers: int | None = None
    information: object | None = None        # cfg.information != "off": solver.RegistrationInformation at the result pose (H, b, eigen-structure, rank, step, cov)
    modes: object | None = None              # cfg.mode_link: solver.ParticleModes of the final particle set, heaviest first
    cleared: int | None = None               # cfg.clear_seen_through: map points the scan saw through and the map dropped
    prior_chi2: float | None = None          # cfg.prior_sigma: e^T diag(1 / sigma^2) e of the returned correction (e = the correction itself: the prior's mean is the zero correction), the innovation statistic a gate would read
    seed: dict | None = None                 # cfg.seed_grid: {"index": best node, "cost": its cost, "cost_zero": the cost of the zero correction (the prediction), "correction": the correction applied to the initial mean ("top": zeros; with "best" initial_guess is prediction · correction_to_pose(correction)), "prediction": the constant-velocity prediction the grid is centred on, "nodes": the nodes handed over as particles ("top" only)}; cfg.seed_levels > 1: "index" gives way to "lattice" (the best node's integer vector on the finest lattice, "nodes" likewise [P, 6]) and "levels", "fine_step", "nodes_scored", "cost_level0" (level 0's best cost) and "fitness_zero" (inliers / rows of the prediction) are added; cfg.seed_skip_fitness > 0: "searched" and "fitness_zero" are added, and a scan that was not searched has only those two, "cost_zero" and "prediction"


class RegistrationPipeline:
    """One instance per sensor; ``process_scan`` is one pass of ICP_processing's loop body for one LiDAR frame."""

    def __init__(self, cfg: PipelineConfig | None = None, device: int = 0):
        self.cfg = cfg or PipelineConfig()
        self.device = device
        self.map = (DeviceVoxelHashMap(self.cfg.map_voxel_size, self.cfg.map_range, self.cfg.map_voxel_max_points, device)
                    if self.cfg.gpu_map else
                    VoxelHashMap(self.cfg.map_voxel_size, self.cfg.map_range, self.cfg.map_voxel_max_points))
        self.bytes_h2d = 0            # cloud bytes sent to the GPU so far (source scans + map traffic)
        self.poses: list[np.ndarray] = []
        self.times: list[float] = []
        self.scan_max_range = 0.0
        self._rng = np.random.default_rng(self.cfg.seed)
        self._solver: SVNICP | None = None
        self._prep: DevicePreprocessor | None = None
        self._seed_nodes = self.cfg.seed_nodes() if self.cfg.seed_grid is not None else None

    def _seed(self, guess, source, dev):
        """cfg.seed_grid: the scan's rows scored at the grid's nodes around the prediction -> (initial mean, particles or None,
        ScanResult.seed).  The only policy is cfg.seed_skip_fitness; otherwise every scan is searched, and the best node is taken
        as it comes.  seed_levels == 1 and seed_skip_fitness == 0 is the flat grid as ever."""
        c = self.cfg
        gate = c.seed_gate or c.map_voxel_size
        extra = {}
        if c.seed_skip_fitness > 0:   # the prediction alone first: one pose, the existing call
            one = pose_rows(np.asarray(guess, float)[None])
            if dev:
                rec, n = self.map.score_poses_device(self._prep.source_f32_ptr, self._prep.n_source, one, gate)[0], self._prep.n_source
            else:
                rec, n = self.map.score_poses(source, one, gate)[0], source.shape[0]
                if c.gpu_map:
                    self.bytes_h2d += source.shape[0] * 12
            fitness = float(rec[1]) / n if n else 0.0
            if fitness >= c.seed_skip_fitness:
                return guess, None, {"searched": False, "fitness_zero": fitness, "cost_zero": float(rec[3]),
                                     "prediction": np.array(guess, float)}
            extra = {"searched": True, "fitness_zero": fitness}
        if c.seed_levels > 1:
            return self._seed_search(guess, source, dev, gate, extra)
        nodes, zero = self._seed_nodes
        poses = correction_poses(guess, nodes)
        if dev:
            scores = self.map.score_poses_device(self._prep.source_f32_ptr, self._prep.n_source, poses, gate)   # not uploaded again
        else:
            scores = self.map.score_poses(source, poses, gate)
            if c.gpu_map:
                self.bytes_h2d += source.shape[0] * 12
        top = c.seed_mode == "top"
        best, first, order = seed_from_scores(scores, nodes, c.particle_count if top else 1)
        seed = {"index": int(order[0]), "cost": float(scores[order[0], 3]), "cost_zero": float(scores[zero, 3]),
                "correction": np.zeros(6) if top else best, "prediction": np.array(guess, float)}
        seed.update(extra)
        if top:
            seed["nodes"] = order.copy()
            return guess, np.ascontiguousarray(first.T), seed
        return guess @ correction_to_pose(best), None, seed

    def _seed_search(self, guess, source, dev, gate, extra):
        """cfg.seed_levels > 1: _seed through the coarse-to-fine search (search_poses), seed_grid being its level 0."""
        c = self.cfg
        ext, stp = c.seed_grid
        keep = c.seed_search_keep()
        if dev:
            n = self._prep.n_source
            res = self.map.search_poses_device(self._prep.source_f32_ptr, n, guess, ext, stp, c.seed_levels, keep, gate)   # not uploaded again
        else:
            n = source.shape[0]
            res = self.map.search_poses(source, guess, ext, stp, c.seed_levels, keep, gate)
            if c.gpu_map:
                self.bytes_h2d += n * 12
        level0 = res["level"][0] if "level" in res else self.map.search_level(0)
        top = c.seed_mode == "top"
        seed = {"lattice": np.array(res["best_lattice"], np.int32), "cost": float(res["best_record"][3]),
                "cost_zero": float(res["zero_record"][3]), "cost_level0": float(level0["records"][level0["kept"][0], 3]),
                "correction": np.zeros(6) if top else np.array(res["best_correction"], float), "prediction": np.array(guess, float),
                "levels": int(res["levels"]), "fine_step": np.array(res["fine_step"], float), "nodes_scored": int(res["nodes_scored"]),
                "fitness_zero": float(res["zero_record"][1]) / n if n else 0.0}
        seed.update(extra)
        if top:
            first = res["top"] if "top" in res else self.map.search_top(c.particle_count)
            seed["nodes"] = np.array(first["lattice"][:c.particle_count], np.int32)
            return guess, np.ascontiguousarray(np.array(first["corrections"][:c.particle_count], float).T), seed
        return guess @ correction_to_pose(seed["correction"]), None, seed

    def _particles(self) -> np.ndarray:
        return initialize_particles(self.cfg.particle_count, PRIOR_UB, PRIOR_LB, self._rng)   # set_initPose, :661-667

    def process_scan(self, points: np.ndarray, stamp: float, point_stamps=None) -> ScanResult:
        """point_stamps: the scan's per-point time field (float64 / float32 / uint32), used when cfg.deskew is set.

        With cfg.segmentation the raw scan is segmented first (segment_scan; on the device with gpu_prep, where the segmented
        cloud feeds the crop without a second upload).  As in the reference, the segmented message is a PointXYZI cloud with
        no time field (OdometryPipeline.cpp:363-381): point_stamps are dropped, so deskew degenerates to min == max (no change);
        the KITTI branch still runs, on the segmented cloud."""
        c = self.cfg
        t0 = time.perf_counter()
        dev = c.gpu_map and c.gpu_prep
        delta = None
        if c.deskew and len(self.poses) >= 2:                                                                   # :552
            delta = se3_log(np.linalg.inv(self.poses[-2]) @ self.poses[-1])                                     # :427-432
        if c.segmentation:
            point_stamps = None                                                                                 # segmentedCloud_ has no time field
        if dev:
            if self._prep is None:
                self._prep = DevicePreprocessor(self.device)
            if c.segmentation:                                                                                  # :331-343 on the device
                n = self._prep.segment(points, c.seg_params)
                self.bytes_h2d += self._prep.bytes_uploaded
                self.scan_max_range = self._prep.scan_device(self._prep.segmented_ptr, n, c.min_range, c.max_range, c.voxel_size,
                                                             self.scan_max_range, delta=delta, kitti=c.kitti)
            elif delta is None:
                self.scan_max_range = self._prep.scan(points, c.min_range, c.max_range, c.voxel_size, self.scan_max_range)  # :556-560
            else:                                                                                               # :551-560
                self.scan_max_range = self._prep.scan(points, c.min_range, c.max_range, c.voxel_size, self.scan_max_range,
                                                      stamps=point_stamps, delta=delta, kitti=c.kitti)
            self.bytes_h2d += self._prep.bytes_uploaded
        else:
            if c.segmentation:
                points, _ = segment_scan(points, c.seg_params)                                                 # :331-343
            if delta is not None:
                points = deskew_pointcloud(points, point_stamps, delta, c.kitti)                               # :553
            cropped, self.scan_max_range = crop_pointcloud(points, c.min_range, c.max_range, self.scan_max_range)   # :556
            to_map = downsample_uniform(cropped, 0.5 * c.voxel_size)                                                # :559
            source = downsample_uniform(to_map, 1.5 * c.voxel_size)                                                 # :560
        guess = pose_prediction(self.poses, self.times, stamp)                                                  # :563-564
        init = self._particles()                                                                                # :573
        if self.map.empty():                                                                                    # :585-593
            # the reference's downsample_uniform filters its input IN PLACE (:684-690): at :585 *cropped_cloud already holds
            # the 0.5-voxel sampling, and that is what seeds the map
            if dev:
                self.map.add_pointcloud_device(self._prep.map_cloud_ptr, self._prep.n_map, guess)
            else:
                self.map.add_pointcloud(to_map, guess)
            self.poses.append(guess); self.times.append(stamp)
            return ScanResult(stamp, guess, guess, preprocessing_s=time.perf_counter() - t0)
        if self._solver is None:
            self._solver = SVNICP(c.solver, init, ParticleWeightOpt(c.weight_dist > 0, c.weight_dist, c.weight_temperature, c.weight_cost), device=self.device)
        s = self._solver
        seed = None
        if c.seed_grid is not None:
            guess, seeded, seed = self._seed(guess, None if dev else source, dev)
            if seeded is not None:
                init = seeded
        with_normal = None
        if c.gpu_map:
            ptr, M = self.map.get_map(guess, self.scan_max_range + 10.0)                                        # :577-578
            if M == 0:
                ptr, M = self.map.get_map()                                                                     # :579-581
            if c.map_normals:
                nptr, with_normal = self.map.get_map_normals(c.solver.normal_k)
            if dev:
                s.add_cloud_device(self._prep.source_ptr, self._prep.n_source, ptr, M, init)                    # :583
            else:
                s.add_cloud_device_target(source, ptr, M, init)                                                 # :583
                self.bytes_h2d += source.shape[0] * 24
            if c.map_normals:
                s.set_target_normals_device(nptr, M)                  # right after the target they belong to: no normal pass
        else:
            target = self.map.get_map(guess, self.scan_max_range + 10.0)                                        # :577-578
            if target.shape[0] == 0:
                target = self.map.get_map()                                                                     # :579-581
            s.add_cloud(source, target, init)                                                                   # :583
            self.bytes_h2d += (source.shape[0] + target.shape[0]) * 24
        t1 = time.perf_counter()
        if c.prior_sigma is not None:   # centred on the initial mean set below: the zero correction
            s.set_pose_prior(np.zeros(6), c.prior_information())
        s.set_initial_mean(guess)                                                                               # :601
        state = s.stein_align()                                                                                 # :602
        if state != SteinICPState.ALIGN_SUCCESS:                                                                # :602-604
            return ScanResult(stamp, guess, guess, preprocessing_s=t1 - t0, align_s=time.perf_counter() - t1, state=int(state),
                              with_normal=with_normal, seed=seed)
        corr = s.get_transformation()                                                                           # :605
        pose = guess @ correction_to_pose(corr)                                                                 # updater_, :37-46
        modes = None
        if c.mode_link is not None:   # no policy here: "heaviest" is the caller's choice, made once in the configuration
            modes = s.particle_modes(c.mode_link[0], c.mode_link[1], c.mode_max)
            if c.mode_select == "heaviest" and modes.n_reported > 0 and np.isfinite(modes.mean[0]).all():
                corr = modes.mean[0].copy()
                pose = guess @ correction_to_pose(corr)
        res = ScanResult(stamp, pose, guess, corr, s.get_distribution(), s.get_cov_matrix(), s.get_particles().reshape(-1),
                         s.get_particle_weight(), t1 - t0, 0.0, int(state), with_normal)
        res.modes = modes
        res.seed = seed
        if c.prior_sigma is not None:   # no policy here: the number a gate would read
            res.prior_chi2 = float(np.sum((np.asarray(corr, np.float64) / np.asarray(c.prior_sigma, np.float64)) ** 2))
        if c.eval_dist > 0:   # the number a caller may gate the map update on (no policy here)
            ev = s.evaluate(c.eval_dist, pose)
            res.fitness, res.inlier_rmse = ev.fitness, ev.inlier_rmse
            if ev.has_normals:
                res.plane_rmse, res.plane_inliers = ev.plane_rmse, ev.plane_inliers
            if c.information != "off":   # what a filter or a gate may read; no policy here either
                res.information = s.information(c.information, c.info_huber)
        if c.clear_seen_through is not None:   # no policy here either: every registered scan clears, with the densest cloud the step has
            w0, w1, m0, m1 = c.clear_seen_through
            args = (pose, c.seg_params, (w0, w1), (m0, m1), c.clear_max_range or c.max_range)
            if dev:
                res.cleared = self.map.clear_seen_through_device(self._prep.cropped_ptr, self._prep.n_cropped, *args)["points_removed"]
            else:
                res.cleared = self.map.clear_seen_through(cropped, *args)["points_removed"]
                if c.gpu_map:
                    self.bytes_h2d += cropped.shape[0] * 12
        # … and at :630 *voxelized_cloud_toMap holds the 1.5-voxel sampling (the second in-place filter, :560): the map is
        # updated with the same points the solver registered
        if dev:
            self.map.add_pointcloud_device(self._prep.source_f32_ptr, self._prep.n_source, pose)                # :630
        else:
            self.map.add_pointcloud(source, pose)                                                               # :630
            if c.gpu_map:
                self.bytes_h2d += source.shape[0] * 12
        self.poses.append(pose); self.times.append(stamp)                                                       # :630
        res.align_s = time.perf_counter() - t1
        return res
