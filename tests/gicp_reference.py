"""Float64 numpy restatement of the generalized-ICP residual (include/svnicp_hip.h "generalized-ICP residual", DESIGN.md
section 4.19) — test infrastructure.  The reference has no such mode, so nothing here is a golden: the expectations of
tests/test_gicp_cpu.py and tests/test_gicp_gpu.py are computed at test time from the formulas below.

    normals    tests/plane_reference.normals, for the target AND (with the source as the cloud) for the source
    weight     C(n) = I - (1 - eps) n n^T,  m = Rt^T n_q,  S = C(m) + C(n_s),  W = 2 eps S^-1  (inverse by cofactors)
    record     per particle [42] = H | b from  u = Rt^T (Ts - q),  rho = sqrt(u^T W u),  w = 1 (rho <= delta) else delta / rho,
               G = [I | -[s]x],  H = sum w G^T W G + 1e-6 I,  b = sum w G^T W u   over the accepted pairs
    accepted   d2 < max_dist (the project's gate), the winner has a normal and the source row has one
    solver     the oracle's split-phase Stein step on the record, exactly as tests/plane_reference.run drives it
"""
import ctypes as C

import numpy as np

import plane_reference as pr

DAMPING = pr.DAMPING
EPS_DEFAULT, EPS_MIN = 1e-3, 1e-6

normals = pr.normals                          # (orc, cloud, kn): the source pass is the target pass on the source cloud
normalise_supplied = pr.normalise_supplied
pose_error = pr.pose_error
total_pose = pr.total_pose


def surface_sum(m, n, eps):
    """S = C(m) + C(n) for rows of unit (or zero) vectors m, n: [N, 3, 3]."""
    a = 1.0 - eps
    return 2.0 * np.eye(3)[None] - a * (m[:, :, None] * m[:, None, :] + n[:, :, None] * n[:, None, :])


def weight(m, n, eps):
    """W = 2 eps S^-1 [N, 3, 3], S inverted by cofactors in float64 (the expression of csrc/gicp_pair_device.hpp)."""
    S = surface_sum(m, n, eps)
    s00, s11, s22, s01, s02, s12 = S[:, 0, 0], S[:, 1, 1], S[:, 2, 2], S[:, 0, 1], S[:, 0, 2], S[:, 1, 2]
    c00, c01, c02 = s11 * s22 - s12 * s12, s02 * s12 - s01 * s22, s01 * s12 - s02 * s11
    c11, c12, c22 = s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01
    det = (s00 * c00 + s01 * c01) + s02 * c02
    k = (2.0 * eps) / det
    W = np.empty_like(S)
    W[:, 0, 0], W[:, 1, 1], W[:, 2, 2] = k * c00, k * c11, k * c22
    W[:, 0, 1] = W[:, 1, 0] = k * c01
    W[:, 0, 2] = W[:, 2, 0] = k * c02
    W[:, 1, 2] = W[:, 2, 1] = k * c12
    return W


def skew(s):
    """[s]x for rows s: [N, 3, 3]."""
    z = np.zeros(s.shape[0])
    return np.stack([np.stack([z, -s[:, 2], s[:, 1]], 1), np.stack([s[:, 2], z, -s[:, 0]], 1), np.stack([-s[:, 1], s[:, 0], z], 1)], 1)


def huber_weight(rho, delta):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(rho <= delta, 1.0, delta / rho)


def pairs(src, tgt, nrm_t, nrm_s, cand, Rt, tt, max_dist):
    """plane_reference.pairs with the source's side added: (slot [B], accepted [B], e [B,3], winner normal [B,3])."""
    slot, ok, e, n = pr.pairs(src, tgt, nrm_t, cand, Rt, tt, max_dist)
    return slot, ok & (nrm_s != 0.0).any(axis=1), e, n


def pair_terms(s, e, nq, ns, Rt, delta, eps):
    """Per accepted pair: (W [N,3,3], u [N,3], rho [N], w [N], G [N,3,6]); pair_rho2: rho^2 = max(u^T W u, 0) as it is summed."""
    m = nq @ Rt                                          # rows: Rt^T n_q
    u = e @ Rt                                           # rows: Rt^T e
    W = weight(m, ns, eps)
    rho = np.sqrt(pair_rho2(W, u))
    G = np.concatenate([np.broadcast_to(np.eye(3), (s.shape[0], 3, 3)), -skew(s)], axis=2)
    return W, u, rho, huber_weight(rho, delta), G


def pair_rho2(W, u):
    v = np.einsum("nij,nj->ni", W, u)
    return np.maximum((u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2], 0.0)


def record_one(src, tgt, nrm_t, nrm_s, cand, Rt, tt, max_dist, delta, eps):
    """(record [42] = H | b, slot [B], stats [2] = {accepted pairs, sum w rho^2}, rho of the accepted pairs)."""
    slot, ok, e, n = pairs(src, tgt, nrm_t, nrm_s, cand, Rt, tt, max_dist)
    W, u, rho, w, G = pair_terms(src[ok], e[ok], n[ok], nrm_s[ok], Rt, delta, eps)
    WG = np.einsum("nij,njk->nik", W, G)
    H = np.einsum("n,nji,njk->ik", w, G, WG)
    H = np.triu(H) + np.triu(H, 1).T + DAMPING * np.eye(6)   # the upper triangle, mirrored: what the device stores
    b = np.einsum("n,nji,nj->i", w, WG, u)
    return np.concatenate([H.reshape(36), b]), slot, np.array([float(ok.sum()), float((w * pair_rho2(W, u)).sum())]), rho


def run(orc, src, tgt, nrm_t, nrm_s, init, K, iterations, max_dist, delta, eps=EPS_DEFAULT, lr=1.0, svn_full_grad=True,
        check_early_stop=False, convergence_threshold=1e-5, R0=None, t0=None, prior=None):
    """plane_reference.run with this module's record; prior = (mean6, Lambda [36]): the pose prior of
    tests/pose_prior_reference.py added to every particle's record, as the library adds it in front of the Stein step."""
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
    if prior is not None:
        import pose_prior_reference as ppr
        import stein_step_reference as ss
        A, mean6, Lam = ss.F64(), prior[0], [float(v) for v in np.asarray(prior[1], np.float64).reshape(36)]
    out = pr.PlaneRun()
    out.corr = np.full((iterations, P, B), -1, np.int32)
    out.stats = np.zeros((P, 2))
    out.residuals = []
    rec = np.zeros((P, 42))
    for it in range(iterations):
        L.orc_sp_finish(s.h)                             # refresh_pose_svn: idempotent
        x = s.get_particles().reshape(6, P)
        res = []
        for p in range(P):
            Rp = orc.so3_exp(x[3:, p])[0]
            Rt, tt = R0 @ Rp, t0 + R0 @ x[:3, p]
            rec[p], out.corr[it, p], out.stats[p], rho = record_one(src, tgt, nrm_t, nrm_s, cand, Rt, tt, max_dist, delta, eps)
            res.append(rho)
            if prior is not None:
                with np.errstate(all="ignore"):
                    H, b = ppr.record(A, rec[p].copy(), R0.reshape(9), Rp.reshape(9), x[:3, p], mean6, Lam, plane=True)
                rec[p] = np.array([float(v) for v in H] + [float(v) for v in b])
        out.residuals.append(res)
        if L.orc_sp_update(s.h, it, rec.ctypes.data_as(C.POINTER(C.c_double))):
            break
    L.orc_sp_finish(s.h)
    out.H, out.b, out.newton, out.phi, out.h = tr["H"], tr["b"], tr["newton"], tr["phi"], tr["h"]
    out.iterations_run = s.iterations_run()
    out.particles = s.get_particles()
    out.solver = s
    return out
