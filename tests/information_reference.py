"""Float64 numpy restatement of svnicp_eval_information and svnicp_information_solve (include/svnicp_hip.h "information matrix
of a registration") — test infrastructure, no device.

    rows        evaluate_reference.evaluate(...): its index, d2 and classes; q = orc.transform(src, R, t), e = q - p
    tangent     right perturbation T Exp([v ; omega]), translation first
    point       rows = inliers; d = sqrt(d2), w = 1 if d <= delta else delta / d; c = R^T e;
                H += w [[I, -hat(s)], [hat(s), |s|^2 I - s s^T]];  b += w [c ; s x c];  sum_wr2 += w d2
    plane       rows = inliers whose target normal is non-zero; r = (n0 e0 + n1 e1) + n2 e2; w = 1 if |r| <= delta else delta / |r|;
                m = R^T n, j = [m ; s x m];  H += w j j^T;  b += w r j;  sum_wr2 += w r^2
    A           the sum of the ABSOLUTE terms of every entry of H and b: the scale a sum's rounding error is measured in
    solve       numpy.linalg.eigh on (H + H^T) / 2 and the two diagonal blocks; rank, H+, step, dof, sigma2, cov as the header says
"""
from dataclasses import dataclass

import numpy as np

import evaluate_reference as er

DEFAULT_FLOOR = 1e-12


@dataclass
class Sums:
    form: str
    pairs: int
    sum_w: float
    sum_wr2: float
    H: np.ndarray        # [6, 6]
    b: np.ndarray        # [6]
    A_H: np.ndarray      # [6, 6] sum of |terms|
    A_b: np.ndarray      # [6]
    rows: np.ndarray     # bool [B]: the contributing rows
    w: np.ndarray        # [B] the weights (0 where a row does not contribute)
    eval: object         # the evaluate_reference.Eval the rows came from


@dataclass
class Solved:
    rank: int
    dof: int
    sigma2: float
    eigval: np.ndarray   # [6] ascending
    eigvec: np.ndarray   # [6, 6] rows
    eig_t: np.ndarray
    vec_t: np.ndarray
    eig_r: np.ndarray
    vec_r: np.ndarray
    step: np.ndarray
    cov: np.ndarray
    pinv: np.ndarray


def hat(s):
    """[n, 3] -> [n, 3, 3]: hat(s) x = s x x."""
    z = np.zeros(len(s))
    return np.stack([np.stack([z, -s[:, 2], s[:, 1]], 1), np.stack([s[:, 2], z, -s[:, 0]], 1), np.stack([-s[:, 1], s[:, 0], z], 1)], 1)


def row_terms(orc, src, tgt, pose, ev, gate, form, delta, normals=None, rows=None):
    """(contributing rows bool [B], w [B], J [B, d, 6], residual [B, d]) with d = 3 (point) or 1 (plane); zero where a row does
    not contribute, and the rows' w r^2 terms.  ``ev``: the evaluate_reference.Eval of ``pose`` at ``gate``; ``rows``: restrict to
    this boolean mask (a row shard)."""
    src, tgt = np.ascontiguousarray(src, np.float64), np.ascontiguousarray(tgt, np.float64)
    T = np.asarray(pose, np.float64).reshape(4, 4)
    R = T[:3, :3]
    B = src.shape[0]
    with np.errstate(all="ignore"):
        q = orc.transform(src, R, T[:3, 3])
        j = np.where(ev.index >= 0, ev.index, 0)
        e = q - tgt[j]
        on = (ev.index >= 0) & (ev.d2 < float(gate) * float(gate))       # evaluate's inliers (NaN d2: not evaluated)
        if form == "plane":
            n = np.asarray(normals, np.float64)[j]
            on &= (n != 0.0).any(axis=1)
        if rows is not None:
            on &= rows
        s = np.where(on[:, None], src, 0.0)
        e = np.where(on[:, None], e, 0.0)
        if form == "point":
            d2 = np.where(on, ev.d2, 0.0)
            d = np.sqrt(d2)
            w = np.where(on, np.where(d <= delta, 1.0, delta / np.where(d > 0, d, 1.0)), 0.0)
            c = e @ R                                    # rows of R^T e
            J = np.concatenate([np.broadcast_to(np.eye(3), (B, 3, 3)), -hat(s)], axis=2) * on[:, None, None]
            res = c
            wr2 = w * d2
        else:
            n = np.where(on[:, None], n, 0.0)
            r = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
            ar = np.abs(r)
            w = np.where(on, np.where(ar <= delta, 1.0, delta / np.where(ar > 0, ar, 1.0)), 0.0)
            m = n @ R
            J = np.concatenate([m, np.cross(s, m)], axis=1)[:, None, :]
            res = r[:, None]
            wr2 = w * r * r
    return on, w, J, res, wr2


def sums(orc, src, tgt, pose, gate, form, delta, normals=None, finite=True, rows=None, ev=None):
    """Every sum svnicp_eval_information returns for the evaluate of ``pose`` at ``gate`` (``normals``: as the context holds
    them), and A.  ``ev``: that evaluate_reference.Eval when the caller already has it (it does not depend on form or delta)."""
    if ev is None:
        ev = er.evaluate(orc, src, tgt, pose, gate, normals=normals, finite=finite)
    on, w, J, res, wr2 = row_terms(orc, src, tgt, pose, ev, gate, form, float(delta), normals, rows)
    WJ = w[:, None, None] * J
    H = np.einsum("bdi,bdj->ij", WJ, J)
    b = np.einsum("bdi,bd->i", WJ, res)
    A_H = np.einsum("bdi,bdj->ij", np.abs(WJ), np.abs(J))
    A_b = np.einsum("bdi,bd->i", np.abs(WJ), np.abs(res))
    return Sums(form, int(on.sum()), float(w.sum()), float(wr2.sum()), H, b, A_H, A_b, on, w, ev)


def _signed(vals, vecs):
    """eigh's columns -> rows, largest-magnitude component positive (lowest index on a tie)."""
    V = vecs.T.copy()
    for v in V:
        k = int(np.argmax(np.abs(v)))
        if v[k] < 0:
            v *= -1.0
    return vals, V


def solve(form, pairs, sum_wr2, H, b, eig_floor_ratio=0.0):
    H = np.asarray(H, np.float64).reshape(6, 6)
    b = np.asarray(b, np.float64).reshape(6)
    S = 0.5 * H + 0.5 * H.T
    val, V = _signed(*np.linalg.eigh(S))
    vt, Vt = _signed(*np.linalg.eigh(S[:3, :3]))
    vr, Vr = _signed(*np.linalg.eigh(S[3:, 3:]))
    f = DEFAULT_FLOOR if eig_floor_ratio == 0.0 else eig_floor_ratio
    top = val[5]
    keep = (val > f * top) & (top > 0)
    rank = int(keep.sum())
    pinv = np.zeros((6, 6))
    for i in np.flatnonzero(keep):
        pinv += np.outer(V[i], V[i]) / val[i]
    dof = (3 if form == "point" else 1) * int(pairs) - rank
    sigma2 = sum_wr2 / dof if dof > 0 else 0.0
    return Solved(rank, dof, sigma2, val, V, vt, Vt, vr, Vr, -pinv @ b, sigma2 * pinv, pinv)
