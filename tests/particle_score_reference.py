"""The contract of include/svnicp_hip.h "score and weight the particles"  in plain numpy float64 — no
device, no oracle: scoring every particle through a candidate table, the soft-min weights, the reference's weighted mean /
variance / covariance (SVNICP.cpp:286-308).  Every product and sum is rounded on its own, in the order the header states;
only the order in which the rows of a particle are ADDED is numpy's, not the device's.
"""
from types import SimpleNamespace

import numpy as np

FIELDS = ("evaluated", "inliers", "plane_inliers", "sum_d2", "sum_r2", "cost")


def transform(src, poses):
    """T_i = (s0*R[3i] + s1*R[3i+1] + s2*R[3i+2]) + t[i] per pose [12] = R row-major | t; poses [P, 12] -> [P, B, 3]."""
    s, p = np.asarray(src, np.float64), np.asarray(poses, np.float64).reshape(-1, 12)[:, None, :]
    with np.errstate(all="ignore"):
        return np.stack([((s[:, 0] * p[..., 3 * i] + s[:, 1] * p[..., 3 * i + 1]) + s[:, 2] * p[..., 3 * i + 2]) + p[..., 9 + i]
                         for i in range(3)], axis=2)


def pairs(src, tgt, cand, poses):
    """The winner of every (particle, source row): strict `<` from candidate 0 among cand [B, K] (clamped to [0, M)), a NaN
    first distance is never replaced.  T [P, B, 3], winner's target index [P, B], its d2, e = T - q, and the smallest d2
    among the OTHER candidates (+inf when there is none; for the precondition checks)."""
    tgt = np.asarray(tgt, np.float64)
    cand = np.clip(np.asarray(cand, np.int64), 0, tgt.shape[0] - 1)
    T = transform(src, poses)
    P, B, K = T.shape[0], cand.shape[0], cand.shape[1]
    kb = np.zeros((P, B), np.int64)
    best = None
    second = np.full((P, B), np.inf)
    with np.errstate(all="ignore"):
        for k in range(K):
            e = T - tgt[cand[:, k]][None]
            d2 = ((e[..., 0] * e[..., 0]) + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
            if k == 0:
                best = d2
                continue
            take = d2 < best
            loser = np.where(take, best, d2)
            second = np.where(loser < second, loser, second)
            kb = np.where(take, k, kb)
            best = np.where(take, d2, best)
        idx = cand[np.arange(B)[None, :], kb]
        return SimpleNamespace(T=T, idx=idx, d2=best, e=T - tgt[idx], second=second, kb=kb)


def score(src, tgt, cand, poses, gate, normals=None, pr=None):
    """float64 [P, 6] in the order of FIELDS (pr: the pairs(...) of the same arguments, to share them between gates)."""
    pr = pairs(src, tgt, cand, poses) if pr is None else pr
    B = len(src)
    thr2 = np.float64(gate) * np.float64(gate)
    with np.errstate(all="ignore"):
        evaluated = np.isfinite(pr.T).all(axis=2) & ~np.isnan(pr.d2)
        inlier = evaluated & (pr.d2 < thr2)
        sum_d2 = np.where(inlier, pr.d2, 0.0).sum(axis=1)
        plane = np.zeros_like(inlier)
        sum_r2 = np.zeros(len(pr.T))
        if normals is not None:
            n = np.asarray(normals, np.float64)[pr.idx]
            plane = inlier & (n != 0.0).any(axis=2)
            nz, ez = np.where(plane[..., None], n, 0.0), np.where(plane[..., None], pr.e, 0.0)
            r = (nz[..., 0] * ez[..., 0] + nz[..., 1] * ez[..., 1]) + nz[..., 2] * ez[..., 2]
            sum_r2 = (r * r).sum(axis=1)
    n_in = inlier.sum(axis=1)
    cost = (sum_d2 + (B - n_in) * thr2) / B
    return np.stack([evaluated.sum(axis=1).astype(np.float64), n_in.astype(np.float64), plane.sum(axis=1).astype(np.float64),
                     sum_d2, sum_r2, cost], axis=1)


def preconditions(pr, gate):
    """(particle, row) pairs within 1e-12 relative of the gate, and those whose two best candidates are within 1e-12
    relative, among the pairs with a finite winner distance."""
    thr2 = gate * gate
    with np.errstate(all="ignore"):
        ok = np.isfinite(pr.T).all(axis=2) & np.isfinite(pr.d2)
        near_gate = np.argwhere(ok & (np.abs(pr.d2 - thr2) <= 1e-12 * thr2))
        tie = np.argwhere(ok & np.isfinite(pr.second) & (np.abs(pr.second - pr.d2) <= 1e-12 * np.maximum(pr.second, pr.d2)))
    return near_gate, tie


def weights(cost, temperature):
    """w_p = exp(-(cost_p - cost_min) / temperature) / Z, Z added in particle order."""
    cost = np.asarray(cost, np.float64)
    w = np.exp(-(cost - cost.min()) / np.float64(temperature))
    z = np.float64(0.0)
    for v in w:
        z = z + v
    return w / z


def weighted_stats(particles_6p, w):
    """SVNICP.cpp:286-308 for arbitrary weights, every sum in particle order: mean [6], var [6], cov [6, 6]."""
    x = np.asarray(particles_6p, np.float64).reshape(6, -1)
    w = np.asarray(w, np.float64)
    P = x.shape[1]
    mean, var, cov = np.zeros(6), np.zeros(6), np.zeros((6, 6))
    for p in range(P):
        mean = mean + x[:, p] * w[p]
    d = x - mean[:, None]
    for p in range(P):
        var = var + d[:, p] * d[:, p] * w[p]
        cov = cov + w[p] * np.outer(d[:, p], d[:, p])
    return mean, var, cov
