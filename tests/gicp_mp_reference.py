"""The 29 sums of k_gicp_accumulate + k_plane_finalize for the cases of tests/gicp_cases.py, in float64 (the restatement of
tests/gicp_reference.py) and in mpmath at 60 digits (test infrastructure; tests/test_gicp_alone_gpu.py).

The yardstick of a sum is  mag = sum over the accepted pairs of cond(S_pair) |term|,  |term| taken factor by factor
(|G^T| |W| |G| and so on).  Why cond(S): every term holds W = 2 eps S^-1, and a closed-form inverse of a 3 x 3 in float64 returns
S^-1 (1 + theta) with |theta| of a few cond(S) u — the entries of adj(S) and det(S) are differences of products of entries of
S, each a few u |S|^2 resp. u |S|^3 off, and |S^-1| is up to cond(S) / |S|.  A pair's term is therefore known to cond(S) u |term|
and no better; the products around W and the additions cost a few u |term| more, which cond(S) >= 1 covers.  The count of
accepted pairs (entry 27) is exact and compared exactly.
"""
import numpy as np

import gicp_reference as gr
import plane_mp_reference as pm

DPS = 60
NS = 29
GROUPS = pm.GROUPS
TINY = 1e-300


def discrete(case):
    """plane_mp_reference.discrete (winner slot, row, Ts, gate, the winner has a normal) and the source row has one."""
    D = pm.discrete(case.src, case.tgt, case.nt, case.cand, case.poses, case.max_dist)
    D["ok"] = D["ok"] & (case.ns != 0.0).any(axis=1)[None, :]
    return D


def sums_f64(case):
    """(values [P][29], mag [P][29]) in float64: values from gicp_reference.record_one, mag as the module docstring states."""
    D = case.discrete()
    out, mag = np.zeros((case.P, NS)), np.zeros((case.P, NS))
    with np.errstate(all="ignore"):
        for p in range(case.P):
            Rt, tt = case.poses[p, :9].reshape(3, 3), case.poses[p, 9:]
            rec, slot, st, _ = gr.record_one(case.src, case.tgt, case.nt, case.ns, case.cand, Rt, tt, case.max_dist, case.delta, case.eps)
            assert np.array_equal(slot, D["win"][p]) and st[0] == D["ok"][p].sum(), "record_one's discrete part differs"
            out[p] = pm.vec29(rec[None], st[None])[0]
            ok = D["ok"][p]
            mag[p, list(pm.DIAG)] = gr.DAMPING
            mag[p, 27] = float(ok.sum())
            if not ok.any():
                continue
            s, nq = case.src[ok], case.nt[D["widx"][p][ok]]
            e = D["Ts"][p][ok] - case.tgt[D["widx"][p][ok]]
            W, u, rho, w, G = gr.pair_terms(s, e, nq, case.ns[ok], Rt, case.delta, case.eps)
            cond = np.linalg.cond(gr.surface_sum(nq @ Rt, case.ns[ok], case.eps))
            aG, aW, au = np.abs(G), np.abs(W), np.abs(e) @ np.abs(Rt)
            cw = cond * w
            Ha = np.einsum("n,nji,njk,nkl->il", cw, aG, aW, aG)
            mag[p, :21] += Ha[np.triu_indices(6)]
            mag[p, 21:27] = np.einsum("n,nji,njk,nk->i", cw, aG, aW, au)
            mag[p, 28] = np.einsum("n,nj,njk,nk->", cw, au, aW, au)
    return out, mag


def sums_mp(case, particles):
    """(values, mag) [n][29] lists of mpf for `particles`, unrounded at DPS digits: S inverted exactly (cofactors in mpmath), the
    Huber branch decided in mpmath, the same accepted pairs and Ts as the float64 discrete part (asserted far from every edge
    by the cases that use this)."""
    import mpmath
    mpmath.mp.dps = DPS
    mpf = mpmath.mpf
    D = case.discrete()
    eps = mpf(case.eps)
    a = 1 - eps
    dl = mpf(case.delta) if np.isfinite(case.delta) else None
    out, mag = [], []
    for p in particles:
        R = [[mpf(float(case.poses[p, 3 * i + k])) for k in range(3)] for i in range(3)]
        acc, ab = [mpf(0)] * NS, [mpf(0)] * NS
        for b in range(case.B):
            if not D["ok"][p, b]:
                continue
            t = int(D["widx"][p, b])
            nq = [mpf(float(v)) for v in case.nt[t]]
            n = [mpf(float(v)) for v in case.ns[b]]
            s = [mpf(float(v)) for v in case.src[b]]
            e = [mpf(float(D["Ts"][p, b, i])) - mpf(float(case.tgt[t, i])) for i in range(3)]
            m = [R[0][i] * nq[0] + R[1][i] * nq[1] + R[2][i] * nq[2] for i in range(3)]
            u = [R[0][i] * e[0] + R[1][i] * e[1] + R[2][i] * e[2] for i in range(3)]
            ua = [abs(R[0][i] * e[0]) + abs(R[1][i] * e[1]) + abs(R[2][i] * e[2]) for i in range(3)]
            S = mpmath.matrix(3, 3)
            for i in range(3):
                for k in range(3):
                    S[i, k] = (2 if i == k else 0) - a * (m[i] * m[k] + n[i] * n[k])
            W = 2 * eps * S ** -1
            ev = mpmath.eigsy(S, eigvals_only=True)
            cond = max(abs(x) for x in ev) / min(abs(x) for x in ev)
            v = [sum(W[i, k] * u[k] for k in range(3)) for i in range(3)]
            rho2 = sum(u[i] * v[i] for i in range(3))
            rho = mpmath.sqrt(rho2)
            w = mpf(1) if (dl is None or rho <= dl) else dl / rho
            sx = [[0, -s[2], s[1]], [s[2], 0, -s[0]], [-s[1], s[0], 0]]
            G = [[mpf(1 if i == k else 0) for k in range(3)] + [-sx[i][k] for k in range(3)] for i in range(3)]
            Wa = [[abs(W[i, k]) for k in range(3)] for i in range(3)]
            Ga = [[abs(x) for x in row] for row in G]
            WG = [[sum(W[i, j] * G[j][k] for j in range(3)) for k in range(6)] for i in range(3)]
            WGa = [[sum(Wa[i][j] * Ga[j][k] for j in range(3)) for k in range(6)] for i in range(3)]
            for idx, (i, k) in enumerate(pm.TRI):
                acc[idx] += w * sum(G[j][i] * WG[j][k] for j in range(3))
                ab[idx] += cond * w * sum(Ga[j][i] * WGa[j][k] for j in range(3))
            for i in range(6):
                acc[21 + i] += w * sum(G[j][i] * v[j] for j in range(3))
                ab[21 + i] += cond * w * sum(Ga[j][i] * sum(Wa[j][k] * ua[k] for k in range(3)) for j in range(3))
            acc[27] += 1; ab[27] += 1
            acc[28] += w * rho2
            ab[28] += cond * w * sum(ua[j] * Wa[j][k] * ua[k] for j in range(3) for k in range(3))
        for i in pm.DIAG:
            acc[i] += mpf(gr.DAMPING); ab[i] += mpf(gr.DAMPING)
        out.append(acc); mag.append(ab)
    return out, mag


def errors(v, mp_sums, mp_mag):
    """E [n][29] = |v - v_mp| / max(mag_mp, 1e-300), formed in mpmath."""
    import mpmath
    tiny = mpmath.mpf(TINY)
    return np.array([[float(abs(m - mpmath.mpf(float(x))) / max(a, tiny)) for m, x, a in zip(rm, rv, ra)]
                     for rm, rv, ra in zip(mp_sums, v, mp_mag)], np.float64)
