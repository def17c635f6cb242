"""Float64 numpy restatement of svnicp_evaluate (include/svnicp_hip.h "evaluate a registration")
— test infrastructure, no device.

    q           orc.transform(src, R, t): (s0*R[i,0] + s1*R[i,1] + s2*R[i,2]) + t[i]
    neighbour   finite clouds: orc.knn_topk(q, tgt, 1); clouds with bad rows: nonfinite_reference.knn_contract(q, tgt, 1)
                (the oracle's heap is not the contract where a distance is NaN)
    classify    d2 recomputed from q and the returned row; evaluated iff q is finite and d2 is not NaN; inlier iff evaluated
                and d2 < thr2 = gate * gate; plane inlier iff inlier and the row's normal is non-zero, r = (n0 e0 + n1 e1) + n2 e2
"""
from dataclasses import dataclass

import numpy as np

import nonfinite_reference as nf


@dataclass
class Eval:
    index: np.ndarray          # int64 [B], -1 = not evaluated
    d2: np.ndarray             # float64 [B], NaN = not evaluated
    second_d2: np.ndarray      # float64 [B] the runner-up's d2 (precondition checks; NaN when M == 1 or not asked for)
    has_normals: bool
    rows: int
    evaluated: int
    inliers: int
    plane_inliers: int
    sum_d2: float
    sum_r2: float
    fitness: float
    inlier_rmse: float
    plane_rmse: float


def pose_matrix(R, t):
    T = np.eye(4)
    T[:3, :3] = np.asarray(R, np.float64).reshape(3, 3)
    T[:3, 3] = np.asarray(t, np.float64).reshape(3)
    return T


def nearest(orc, q, tgt, finite, k=1):
    """k nearest target rows of every q by (d2, index): int64 [B, k] and float64 [B, k]."""
    k = min(k, tgt.shape[0])
    if finite:
        return orc.knn_topk(q, tgt, k)
    return nf.knn_contract(q, tgt, k)


def evaluate(orc, src, tgt, pose, gate, normals=None, finite=True, with_second=False):
    """The figures and per-row arrays svnicp_evaluate must return for the 4x4 ``pose``.  ``finite=False``: the clouds may hold
    NaN, inf or huge rows (the contract's neighbours instead of the oracle's).  ``normals``: [M, 3] as the context holds them
    (unit rows, 0 = none) or None."""
    src, tgt = np.ascontiguousarray(src, np.float64), np.ascontiguousarray(tgt, np.float64)
    T = np.asarray(pose, np.float64).reshape(4, 4)
    with np.errstate(all="ignore"):
        q = orc.transform(src, T[:3, :3], T[:3, 3])
        idx, dk = nearest(orc, q, tgt, finite, 2 if with_second else 1)
        j = idx[:, 0]
        p = tgt[j]
        e0, e1, e2 = q[:, 0] - p[:, 0], q[:, 1] - p[:, 1], q[:, 2] - p[:, 2]
        d2 = ((e0 * e0) + e1 * e1) + e2 * e2
        thr2 = float(gate) * float(gate)
        evaluated = np.isfinite(q).all(axis=1) & ~np.isnan(d2)
        inlier = evaluated & (d2 < thr2)
        sum_d2 = float(np.sum(d2[inlier]))
        n_in = int(inlier.sum())
        plane, sum_r2 = np.zeros_like(inlier), 0.0
        if normals is not None:
            n = np.asarray(normals, np.float64)[j]
            plane = inlier & (n != 0.0).any(axis=1)
            r = (n[:, 0] * e0 + n[:, 1] * e1) + n[:, 2] * e2
            sum_r2 = float(np.sum((r * r)[plane]))
    n_pl = int(plane.sum())
    second = dk[:, 1] if (with_second and dk.shape[1] > 1) else np.full(src.shape[0], np.nan)
    return Eval(np.where(evaluated, j, -1).astype(np.int64), np.where(evaluated, d2, np.nan), second, normals is not None,
                src.shape[0], int(evaluated.sum()), n_in, n_pl, sum_d2, sum_r2, n_in / src.shape[0],
                float(np.sqrt(sum_d2 / n_in)) if n_in else 0.0, float(np.sqrt(sum_r2 / n_pl)) if n_pl else 0.0)


def preconditions(ev, gate):
    """(rows whose d2 lies within 1e-9 relative of the gate, rows whose first and second nearest d2 lie within 1e-12
    relative): both must be empty for a case whose index array and counts are compared exactly."""
    thr2 = float(gate) * float(gate)
    ok = ev.index >= 0
    with np.errstate(invalid="ignore"):
        near_gate = np.flatnonzero(ok & (np.abs(ev.d2 - thr2) <= 1e-9 * thr2))
        tie = np.flatnonzero(ok & (np.abs(ev.second_d2 - ev.d2) <= 1e-12 * np.maximum(ev.second_d2, ev.d2)))
    return near_gate, tie
