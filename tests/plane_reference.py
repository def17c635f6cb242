"""Float64 numpy restatement of the point-to-plane residual (include/svnicp_hip.h "point-to-plane residual", DESIGN.md
section 4.9) — test infrastructure.  The reference has no such mode, so nothing here is a golden: the expectations of
tests/test_plane_cpu.py and tests/test_plane_gpu.py are computed at test time from the formulas below.

    normals    orc.knn_topk(tgt, tgt, kn) + numpy.linalg.eigh of the neighbourhood covariance
    record     per particle [42] = H | b from  e = Ts - q,  r = n.e,  w = 1 (|r| <= delta) else delta / |r|,
               m = Rt^T n,  j = [m ; s x m],  H = sum w j j^T + 1e-6 I,  b = sum w r j   over the accepted pairs
    solver     the oracle's split-phase calls (orc_sp_begin / orc_sp_update / orc_sp_finish), as tests/oracle_backend.py
               drives them: the Stein step is the oracle's own, only the record comes from here
"""
import ctypes as C

import numpy as np

MIN_RATIO = 0.01      # a normal is valid iff lambda1 >= MIN_RATIO * lambda2 (kPlaneMinRatio, csrc/plane_normal_device.hpp)
DAMPING = 1e-6        # SVNICP.cpp:153, kept in plane mode


def neighbourhood_eig(orc, tgt, kn):
    """(eigenvalues [M,3] ascending, eigenvectors [M,3,3] columns, all-neighbours-finite [M]) of the covariance of every
    target point's kn nearest target points (itself included), offsets taken relative to the point itself."""
    tgt = np.ascontiguousarray(tgt, np.float64)
    idx, _ = orc.knn_topk(tgt, tgt, kn)
    d = tgt[idx] - tgt[:, None, :]                       # [M, kn, 3]
    finite = np.isfinite(d).all(axis=(1, 2))
    mean = np.zeros((tgt.shape[0], 3))
    for k in range(kn):                                  # neighbour order, like the device
        mean = mean + d[:, k, :]
    mean = mean / kn
    c = d - mean[:, None, :]
    cov = np.zeros((tgt.shape[0], 3, 3))
    for k in range(kn):
        cov = cov + c[:, k, :, None] * c[:, k, None, :]
    cov[~finite] = np.eye(3)
    lam, vec = np.linalg.eigh(cov)
    return lam, vec, finite


def normals(orc, tgt, kn):
    """(unit normals [M,3] with 0 rows where there is none, valid [M] bool, eigenvalues [M,3])."""
    lam, vec, finite = neighbourhood_eig(orc, tgt, kn)
    valid = finite & (lam[:, 2] > 0.0) & (lam[:, 1] >= MIN_RATIO * lam[:, 2])
    n = vec[:, :, 0].copy()
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[~valid] = 0.0
    return n, valid, lam


def normalise_supplied(nrm, tgt):
    """What svnicp_set_target_normals keeps: unit rows, 0 for a zero / non-finite row or a non-finite point."""
    nrm = np.asarray(nrm, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nn = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
        ok = (nn > 0.0) & np.isfinite(nn) & np.isfinite(np.asarray(tgt)).all(axis=1)
        out = np.where(ok[:, None], nrm / np.where(ok, nn, 1.0)[:, None], 0.0)
    return out


def transform(src, Rt, tt):
    """Ts with the kernels' unfused expression (s0*R0 + s1*R1 + s2*R2) + t per row."""
    s0, s1, s2 = src[:, 0], src[:, 1], src[:, 2]
    return np.stack([(s0 * Rt[i, 0] + s1 * Rt[i, 1] + s2 * Rt[i, 2]) + tt[i] for i in range(3)], axis=1)


def pairs(src, tgt, nrm, cand, Rt, tt, max_dist):
    """One particle: winner slot [B] (nearest of the K candidates, unfused d², ties to the lowest slot), accepted [B],
    e = Ts - q [B,3], the winner's normal [B,3]."""
    Ts = transform(src, Rt, tt)
    q = tgt[cand]                                        # [B, K, 3]
    dx, dy, dz = Ts[:, None, 0] - q[:, :, 0], Ts[:, None, 1] - q[:, :, 1], Ts[:, None, 2] - q[:, :, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    slot = np.argmin(d2, axis=1)
    rows = np.arange(src.shape[0])
    win = cand[rows, slot]
    e = Ts - tgt[win]
    n = nrm[win]
    with np.errstate(invalid="ignore"):
        ok = (d2[rows, slot] < max_dist) & (n != 0.0).any(axis=1)      # squared distance against max_dist: the project's gate
    return slot, ok, e, n


def huber_weight(r, delta):
    ar = np.abs(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ar <= delta, 1.0, delta / ar)


def record_one(src, tgt, nrm, cand, Rt, tt, max_dist, delta):
    """(record [42] = H | b, slot [B], stats [2] = {accepted pairs, sum w r²}, residuals of the accepted pairs)."""
    slot, ok, e, n = pairs(src, tgt, nrm, cand, Rt, tt, max_dist)
    s, e, n = src[ok], e[ok], n[ok]
    r = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
    w = huber_weight(r, delta)
    m = n @ Rt                                           # rows: Rt^T n
    j = np.concatenate([m, np.cross(s, m)], axis=1)      # [N, 6]
    H = (j * w[:, None]).T @ j
    H = np.triu(H) + np.triu(H, 1).T + DAMPING * np.eye(6)   # the upper triangle, mirrored: what the device stores
    b = (j * (w * r)[:, None]).sum(axis=0)
    return np.concatenate([H.reshape(36), b]), slot, np.array([float(ok.sum()), float((w * r * r).sum())]), r


def total_pose(orc, x6, R0, t0):
    """Rt = R0 R, tt = t0 + R0 t of a particle [t ; Log R]."""
    R = orc.so3_exp(x6[3:])[0]
    return R0 @ R, t0 + R0 @ x6[:3]


class PlaneRun:
    """Result of run(): trace arrays like svnicp_get_trace's, the final particles and statistics."""


def run(orc, src, tgt, nrm, init, K, iterations, max_dist, delta, lr=1.0, svn_full_grad=True, check_early_stop=False,
        convergence_threshold=1e-5, R0=None, t0=None):
    src = np.ascontiguousarray(src, np.float64)
    tgt = np.ascontiguousarray(tgt, np.float64)
    R0 = np.eye(3) if R0 is None else np.asarray(R0, np.float64).reshape(3, 3)
    t0 = np.zeros(3) if t0 is None else np.asarray(t0, np.float64).reshape(3)
    s = orc.Solver(init, iterations=iterations, lr=lr, max_dist=max_dist, check_early_stop=check_early_stop,
                   convergence_threshold=convergence_threshold, knn_count=K, svn_full_grad=svn_full_grad)
    s.add_cloud(src, tgt, init)
    s.set_initial_mean(R0, t0)
    tr = s.enable_trace()
    L, P, B = s.L, s.P, src.shape[0]
    L.orc_sp_begin(s.h)
    cand, _ = orc.knn_topk(orc.transform(src, R0, t0), tgt, K)   # stage A: candidates of R0 s + t0
    out = PlaneRun()
    out.corr = np.full((iterations, P, B), -1, np.int32)
    out.stats = np.zeros((P, 2))
    out.residuals = []
    rec = np.zeros((P, 42))
    for it in range(iterations):
        L.orc_sp_finish(s.h)                             # refresh_pose_svn: idempotent
        x = s.get_particles().reshape(6, P)
        res = []
        for p in range(P):
            Rt, tt = total_pose(orc, x[:, p], R0, t0)
            rec[p], out.corr[it, p], out.stats[p], r = record_one(src, tgt, nrm, cand, Rt, tt, max_dist, delta)
            res.append(r)
        out.residuals.append(res)
        if L.orc_sp_update(s.h, it, rec.ctypes.data_as(C.POINTER(C.c_double))):
            break
    L.orc_sp_finish(s.h)
    out.H, out.b, out.newton, out.phi, out.h = tr["H"], tr["b"], tr["newton"], tr["phi"], tr["h"]
    out.iterations_run = s.iterations_run()
    out.particles = s.get_particles()
    out.solver = s                                       # mean, variance and covariance: the oracle's getters on its particles
    return out


def pose_error(pose6, true6):
    """(translation error in metres, rotation error in radians) of [t ; Log R] against the true displacement."""
    import math
    def exp(w):
        a = np.linalg.norm(w)
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        return np.eye(3) if a == 0 else np.eye(3) + math.sin(a) / a * Kx + (1 - math.cos(a)) / a ** 2 * Kx @ Kx
    dR = exp(np.asarray(pose6[3:])).T @ exp(np.asarray(true6[3:]))
    ang = math.acos(max(-1.0, min(1.0, 0.5 * (np.trace(dR) - 1.0))))
    return float(np.linalg.norm(np.asarray(pose6[:3]) - np.asarray(true6[:3]))), float(ang)
