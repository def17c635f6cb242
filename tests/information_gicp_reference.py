"""Float64 numpy restatement of svnicp_eval_information_gicp (include/svnicp_hip.h "information matrix of a registration", the
GICP form) — test infrastructure, no device.

    rows        evaluate_reference.evaluate(...): its index, d2 and classes; q = orc.transform(src, R, t), e = q - p.  A row
                contributes iff it is a plane inlier of that evaluate (inlier, target normal non-zero) and its source normal
                is non-zero (k_gicp_accumulate's rule, tests/gicp_reference.pairs)
    terms       u = R^T e, m = R^T n_q, W = 2 eps (C(m) + C(n_s))^-1 (gicp_reference.weight: the cofactor expression of
                csrc/gicp_pair_device.hpp), rho = sqrt(max(u^T W u, 0)), w = 1 if rho <= delta else delta / rho,
                G = [I | -hat(s)];  H += w G^T W G;  b += w G^T W u;  sum_w += w;  sum_wr2 += w rho^2
    A           the sums of the ABSOLUTE terms, with |W|'s entries: A_H = sum w |G|^T |W| |G|, A_b = sum w |G|^T |W| |u|
    solve       information_reference.solve with dim = 3 (rho is a three-dimensional whitened residual)
"""
import numpy as np

import evaluate_reference as er
import gicp_reference as gr
import information_reference as ir


def row_sums(R, s, e, nq, ns, delta, eps):
    """The sums over rows that all contribute.  R [3, 3]; s, e, nq, ns [N, 3].
    -> (H, b, sum_w, sum_wr2, A_H, A_b, w [N], rho [N])."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    W, u, rho, w, G = gr.pair_terms(s, e, nq, ns, R, float(delta), float(eps))
    WG = np.einsum("nij,njk->nik", W, G)
    H = np.einsum("n,nji,njk->ik", w, G, WG)
    b = np.einsum("n,nji,nj->i", w, WG, u)
    aG, aW = np.abs(G), np.abs(W)
    A_H = np.einsum("n,nji,njk->ik", w, aG, np.einsum("nij,njk->nik", aW, aG))
    A_b = np.einsum("n,nji,nj->i", w, aG, np.einsum("nij,nj->ni", aW, np.abs(u)))
    return H, b, float(w.sum()), float((w * rho * rho).sum()), A_H, A_b, w, rho


def sums(orc, src, tgt, pose, gate, delta, eps, normals, src_normals, finite=True, rows=None, ev=None):
    """information_reference.Sums (form "gicp") of the evaluate of ``pose`` at ``gate``.  ``normals`` [M, 3] and
    ``src_normals`` [B, 3]: as the context holds them (unit rows, 0 = none).  ``ev``: that evaluate_reference.Eval when the
    caller already has it; ``rows``: restrict to this boolean mask (a row shard)."""
    src, tgt = np.ascontiguousarray(src, np.float64), np.ascontiguousarray(tgt, np.float64)
    nt, ns = np.asarray(normals, np.float64), np.asarray(src_normals, np.float64)
    if ev is None:
        ev = er.evaluate(orc, src, tgt, pose, gate, normals=nt, finite=finite)
    T = np.asarray(pose, np.float64).reshape(4, 4)
    with np.errstate(all="ignore"):
        q = orc.transform(src, T[:3, :3], T[:3, 3])
        j = np.where(ev.index >= 0, ev.index, 0)
        on = (ev.index >= 0) & (ev.d2 < float(gate) * float(gate)) & (nt[j] != 0.0).any(axis=1) & (ns != 0.0).any(axis=1)
        if rows is not None:
            on &= rows
        e = (q - tgt[j])[on]
    H, b, sum_w, sum_wr2, A_H, A_b, w_on, _ = row_sums(T[:3, :3], src[on], e, nt[j][on], ns[on], delta, eps)
    w = np.zeros(src.shape[0])
    w[on] = w_on
    return ir.Sums("gicp", int(on.sum()), sum_w, sum_wr2, H, b, A_H, A_b, on, w, ev)


def solve(form, pairs, sum_wr2, H, b, eig_floor_ratio=0.0):
    """information_reference.solve extended by the GICP form: dim = 3, dof = 3 pairs - rank."""
    return ir.solve("point" if form == "gicp" else form, pairs, sum_wr2, H, b, eig_floor_ratio)
