"""The contract of include/svnicp_hip.h "score and weight the particles in the objective the solver minimised" (DESIGN.md
section 4.12.1) in plain numpy float64 — no device, no oracle.  It reuses particle_score_reference.pairs (poses, transformed
point, winner, classes) and states the two new tails: the Huber-weighted plane residual and the generalized-ICP residual, every
product and sum rounded on its own in the operand order the header and csrc/gicp_pair_device.hpp state; only the order in which
the rows of a particle are ADDED is numpy's, not the device's.
"""
from types import SimpleNamespace

import numpy as np

import particle_score_reference as ps

FIELDS = ("evaluated", "inliers", "accepted", "sum_d2", "sum_h", "cost")
AS_SOLVED, POINT, PLANE, GICP = -1, 0, 1, 2    # SVNICP_SCORE_*


def h(x, x2, delta):
    """h(x) = x*x if x <= delta else delta*(2*x - delta), handed x and x*x; the branch is a select (delta = +inf: x2 itself)."""
    with np.errstate(all="ignore"):
        inside = x <= delta
        d = np.where(inside, 0.0, delta)
        return np.where(inside, x2, d * (2.0 * x - d))


def cap(gate, delta):
    g = np.float64(gate)
    return float(h(g, g * g, np.float64(delta)))


def gicp_weight(m, n, eps):
    """W = 2 eps (C(m) + C(n))^-1 by cofactors: the six entries [W00 W01 W02 W11 W12 W22] in gicp_weight's operand order."""
    m0, m1, m2, n0, n1, n2 = m[..., 0], m[..., 1], m[..., 2], n[..., 0], n[..., 1], n[..., 2]
    a = 1.0 - eps
    s00, s11, s22 = 2.0 - a * (m0 * m0 + n0 * n0), 2.0 - a * (m1 * m1 + n1 * n1), 2.0 - a * (m2 * m2 + n2 * n2)
    s01, s02, s12 = -(a * (m0 * m1 + n0 * n1)), -(a * (m0 * m2 + n0 * n2)), -(a * (m1 * m2 + n1 * n2))
    c00, c01, c02 = s11 * s22 - s12 * s12, s02 * s12 - s01 * s22, s01 * s12 - s02 * s11
    c11, c12, c22 = s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01
    det = (s00 * c00 + s01 * c01) + s02 * c02
    k = (2.0 * eps) / det
    return k * c00, k * c01, k * c02, k * c11, k * c12, k * c22


def rotate_back(R, x):
    """R^T x per (particle, row): R [P, 9] row-major, x [P, B, 3]; u_i = R[i]*x0 + R[3+i]*x1 + R[6+i]*x2 (left to right)."""
    R = R[:, None, :]
    return np.stack([R[..., i] * x[..., 0] + R[..., 3 + i] * x[..., 1] + R[..., 6 + i] * x[..., 2] for i in range(3)], axis=2)


def gicp_rho2(u, m, ns, eps):
    """(rho2 = max(u^T W u, 0), v = W u) in gicp_pair_metric's operand order."""
    W0, W1, W2, W3, W4, W5 = gicp_weight(m, ns, eps)
    u0, u1, u2 = u[..., 0], u[..., 1], u[..., 2]
    v0 = (W0 * u0 + W1 * u1) + W2 * u2
    v1 = (W1 * u0 + W3 * u1) + W4 * u2
    v2 = (W2 * u0 + W4 * u1) + W5 * u2
    q = (u0 * v0 + u1 * v1) + u2 * v2
    return np.where(q > 0.0, q, 0.0), np.stack([v0, v1, v2], axis=-1)


def terms(form, pr, poses, gate, normals, src_normals=None, delta=np.inf, eps=1e-3):
    """Per (particle, row) of the plane or GICP form: evaluated, inlier, accepted [P, B] and the pair's x (|r| or rho), x2 (r*r or
    rho2) and h, zeros where not accepted."""
    thr2 = np.float64(gate) * np.float64(gate)
    with np.errstate(all="ignore"):
        evaluated = np.isfinite(pr.T).all(axis=2) & ~np.isnan(pr.d2)
        inlier = evaluated & (pr.d2 < thr2)
        n = np.asarray(normals, np.float64)[pr.idx]
        acc = inlier & (n != 0.0).any(axis=2)
        if form == GICP:
            ns = np.broadcast_to(np.asarray(src_normals, np.float64)[None], n.shape)
            acc = acc & (ns != 0.0).any(axis=2)
        nz, ez = np.where(acc[..., None], n, 0.0), np.where(acc[..., None], pr.e, 0.0)
        if form == PLANE:
            r = (nz[..., 0] * ez[..., 0] + nz[..., 1] * ez[..., 1]) + nz[..., 2] * ez[..., 2]
            x, x2 = np.abs(r), r * r
        else:
            R = np.asarray(poses, np.float64).reshape(-1, 12)[:, :9]
            u, m = rotate_back(R, ez), rotate_back(R, nz)
            x2, _ = gicp_rho2(u, m, np.where(acc[..., None], ns, 0.0), np.float64(eps))
            x = np.sqrt(x2)
        hh = h(x, x2, np.float64(delta))
    return SimpleNamespace(evaluated=evaluated, inlier=inlier, accepted=acc, x=x, x2=x2, h=hh)


def score(form, src, tgt, cand, poses, gate, normals=None, src_normals=None, delta=np.inf, eps=1e-3, pr=None):
    """float64 [P, 6] in the order of FIELDS; form POINT: particle_score_reference.score."""
    if form == POINT:
        return ps.score(src, tgt, cand, poses, gate, normals=normals, pr=pr)
    pr = ps.pairs(src, tgt, cand, poses) if pr is None else pr
    B = len(src)
    t = terms(form, pr, poses, gate, normals, src_normals, delta, eps)
    sum_d2 = np.where(t.inlier, pr.d2, 0.0).sum(axis=1)
    sum_h = t.h.sum(axis=1)
    n_acc = t.accepted.sum(axis=1)
    cost = (sum_h + (B - n_acc) * cap(gate, delta)) / B
    f = np.float64
    return np.stack([t.evaluated.sum(axis=1).astype(f), t.inlier.sum(axis=1).astype(f), n_acc.astype(f), sum_d2, sum_h, cost], axis=1)
