"""The plane residual's kernels one by one, restated for exact and 60-digit arithmetic (test infrastructure; the float64
restatement stays tests/plane_reference.py).

NORMALS.  A neighbourhood's scatter matrix C = sum (x - mean)(x - mean)^T is a rational function of its float64
coordinates: `exact_scatter` forms it in exact rationals (fractions.Fraction), whatever the magnitudes (1e-170 and 1e20
included), and `mp_eigenvalues` takes its eigenvalues in mpmath at DPS digits.  `criterion` judges a float64 vector n as the
eigenvector of the smallest eigenvalue l0 <= l1 <= l2, again in exact rationals, so that judging adds no rounding:

    norm      | |n| - 1 |
    residual  | C n - rho n | / (|n| l2),   rho = n^T C n / n^T n
    rayleigh  (rho - l0) / l2                (>= 0 for the exact C)

Where (l1 - l0) / l2 >= 1e-3 the angle to the true eigenvector follows from the residual (sin theta <= residual / gap,
Davis-Kahan); where the gap closes the eigenvector is not determined and the two figures are all there is to ask.

ACCUMULATE.  The discrete part (Ts, winner, d2, gate) is tests/stage_b_reference.discrete, defined in float64; a pair is
accepted iff d2 < max_dist and the winner has a normal.  The real-valued part takes Ts, winners and gates as given and forms
the 29 values of a particle's record — H's upper triangle WITH the 1e-6 of the diagonal (21), b (6), the accepted count,
sum w r^2 — and the sum of |term| of each: `sums_mp` in mpmath, `sums_f64` with tests/plane_reference.record_one (the
yardstick) and a numpy sum of |term|.  |term| takes the Jacobian term-wise absolute (|m_i| as sum |R_ki n_k|, |s x m| as
|s_1| |m_2| + |s_2| |m_1| ..., |r| as sum |n_i e_i|), so that cancellation inside j or r does not hide in the yardstick.
E(v) = |v - v_mp| / max(sum|term|_mp, 1e-300).

VARIANTS are deliberately wrong float64 programs the CPU test must see refused.
"""
from fractions import Fraction

import numpy as np

import plane_reference as pr
import stage_b_reference as sb

DPS = 60
NS = 29
TRI = tuple((i, k) for i in range(6) for k in range(i, 6))
DIAG = tuple(e for e, (i, k) in enumerate(TRI) if i == k)
GROUPS = (("Htt", tuple(e for e, (i, k) in enumerate(TRI) if k < 3)), ("Htr", tuple(e for e, (i, k) in enumerate(TRI) if i < 3 <= k)),
          ("Hrr", tuple(e for e, (i, k) in enumerate(TRI) if i >= 3)), ("b", tuple(range(21, 27))), ("wr2", (28,)))
VARIANTS = ("gate_le", "no_damping", "huber_unweighted", "huber_squared", "normal_untransposed", "zero_normal_accepted")
TINY = 1e-300


# ------------------------------------------------------------------------------------------------ normals
def exact_scatter(pts):
    """3x3 list of Fractions: sum (x - mean)(x - mean)^T of the rows of pts [n][3], exactly."""
    X = [[Fraction(float(v)) for v in row] for row in np.asarray(pts, np.float64)]
    n = len(X)
    mean = [sum(r[i] for r in X) / n for i in range(3)]
    D = [[r[i] - mean[i] for i in range(3)] for r in X]
    return [[sum(d[i] * d[k] for d in D) for k in range(3)] for i in range(3)]


def _mpf(q):
    import mpmath
    return mpmath.mpf(q.numerator) / mpmath.mpf(q.denominator)


def mp_eigenvalues(C, dps=DPS, clamp=True):
    """Ascending eigenvalues (mpf) of a symmetric 3x3 of Fractions; clamp: negative rounding residue of a scatter matrix
    becomes 0 (a matrix that is merely symmetric keeps its negative eigenvalues)."""
    import mpmath
    mpmath.mp.dps = dps
    tr = C[0][0] + C[1][1] + C[2][2]
    if tr == 0:
        return [mpmath.mpf(0)] * 3
    A = mpmath.matrix([[_mpf(C[i][k] / tr) for k in range(3)] for i in range(3)])     # scaled: eigsy's stopping rule is absolute
    lam = sorted(mpmath.eigsy(A, eigvals_only=True))
    t = _mpf(tr)
    return [(max(v, mpmath.mpf(0)) if clamp else v) * t for v in lam]


def as_fraction(v, digits=45):
    """An mpf as a Fraction good to `digits` significant digits (the criterion divides by eigenvalues in rationals)."""
    import mpmath
    if v == 0:
        return Fraction(0)
    man, exp = mpmath.frexp(v)
    return Fraction(int(mpmath.floor(man * mpmath.mpf(2) ** 160))) * Fraction(2) ** (int(exp) - 160)


def split_double(q):
    """(hi, lo) float64 with hi + lo = q to 2^-106 relative: how the fixture keeps an eigenvalue."""
    hi = float(q)
    return hi, float(q - Fraction(hi))


def criterion(C, l0, l2, n):
    """(norm, residual, rayleigh) of the float64 vector n against the exact C and its eigenvalues l0, l2 (Fractions)."""
    from math import sqrt
    v = [Fraction(float(x)) for x in n]
    nn = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    Cn = [C[i][0] * v[0] + C[i][1] * v[1] + C[i][2] * v[2] for i in range(3)]
    rho = (v[0] * Cn[0] + v[1] * Cn[1] + v[2] * Cn[2]) / nn
    res2 = sum((Cn[i] - rho * v[i]) ** 2 for i in range(3)) / (nn * l2 * l2)
    # |n| - 1 = (nn - 1) / (|n| + 1): formed from the exact nn - 1, |n| + 1 is 2 to a part in 1e15
    return abs(float(nn - 1)) / (sqrt(float(nn)) + 1.0), sqrt(float(res2)), float((rho - l0) / l2)


OFFSET_MAX = 2.0 ** 64    # kOffsetMax of k_target_normals: a neighbour offset at or beyond it means "no normal"


def scatter_f64(tgt, idx):
    """k_target_normals' float64 scatter matrices [M][6] = d0 d1 d2 a01 a02 a12 and its `finite` [M] from neighbour lists
    idx [M][kn]: offsets relative to the row's own point, mean by sum / kn, second pass in neighbour order."""
    tgt = np.asarray(tgt, np.float64)
    kn = idx.shape[1]
    with np.errstate(all="ignore"):
        d = tgt[idx] - tgt[:, None, :]
        finite = (np.abs(d) < OFFSET_MAX).all(axis=(1, 2))
        m = np.zeros((tgt.shape[0], 3))
        for k in range(kn):
            m = m + d[:, k]
        m = m / kn
        c = d - m[:, None, :]
        out = np.zeros((tgt.shape[0], 6))
        for k in range(kn):
            x, y, z = c[:, k, 0], c[:, k, 1], c[:, k, 2]
            out = out + np.stack([x * x, y * y, z * z, x * y, x * z, y * z], 1)
    return out, finite


def judge_clusters(case, lam, valid, n):
    """A normal case's rows n [M][3] (0 = no normal) against the exact scatter matrices of its clusters.  Returns
    (wrong: [(kind, placement, row)] whose validity differs from valid [cluster], figures: {kind: (norm, residual, rayleigh)},
    the largest of each over the rows of the kind's valid clusters, axes: [(kind, placement, row)] of exact kinds whose normal
    is not the signed unit axis vector bit for bit).  No row of a judged cluster is left out."""
    wrong, axes, fig = [], [], {}
    has = (np.asarray(n) != 0.0).any(axis=1)
    for c, l, v in zip(case.clusters, lam, valid):
        for r in c.rows:
            if has[r] != bool(v):
                wrong.append((c.kind, c.placement, int(r)))
        if not v:
            continue
        C = exact_scatter(c.pts)
        for r in c.rows:
            if not has[r]:
                continue
            f = criterion(C, l[0], l[2], n[r])
            fig[c.kind] = tuple(max(a, b) for a, b in zip(fig.get(c.kind, (0.0, 0.0, 0.0)), f))
            if c.axis is not None:
                a = np.abs(n[r])
                unit = sorted(a.tolist()) == [0.0, 0.0, 1.0]
                if not unit or (c.axis >= 0 and a[c.axis] != 1.0):
                    axes.append((c.kind, c.placement, int(r)))
    return wrong, fig, axes


# ------------------------------------------------------------------------------------------------ accumulate
def discrete(src, tgt, nrm, cand, poses, max_dist, variant=()):
    """stage_b_reference.discrete plus widx [P][B] (the winner's target row) and ok [P][B] (accepted: the gate, and the
    winner has a normal)."""
    V = frozenset(variant)
    D = sb.discrete(src, tgt, cand, poses, max_dist, ("mask_le",) if "gate_le" in V else ())
    D["widx"] = cand[np.arange(src.shape[0])[None, :], D["win"]]
    has = (nrm != 0.0).any(axis=1)
    D["ok"] = D["mask"] & (True if "zero_normal_accepted" in V else has[D["widx"]])
    return D


def vec29(Hb, stats):
    """[P][29] from records [P][42] and statistics [P][2]: H's upper triangle row-major, b, accepted pairs, sum w r^2."""
    H = np.asarray(Hb)[:, :36].reshape(-1, 6, 6)
    return np.concatenate([np.stack([H[:, i, k] for i, k in TRI], 1), np.asarray(Hb)[:, 36:], np.asarray(stats)], 1)


def _terms(w, r, rabs, j, jabs):
    t = [w * j[i] * j[k] for i, k in TRI] + [w * r * j[i] for i in range(6)] + [None, w * r * r]
    a = [w * jabs[i] * jabs[k] for i, k in TRI] + [w * rabs * jabs[i] for i in range(6)] + [None, w * rabs * rabs]
    return t, a


def sums_f64(src, tgt, nrm, cand, poses, max_dist, delta, D, variant=()):
    """(values [P][29], sum|term| [P][29]) in float64.  Values: plane_reference.record_one per particle (the yardstick's own
    program) — or, for a variant, this module's deliberately wrong one."""
    V = frozenset(variant)
    P = poses.shape[0]
    out, mag = np.zeros((P, NS)), np.zeros((P, NS))
    with np.errstate(all="ignore"):
        for p in range(P):
            Rt, tt = poses[p, :9].reshape(3, 3), poses[p, 9:]
            ok = D["ok"][p]
            s, n = src[ok], nrm[D["widx"][p][ok]]
            e = D["Ts"][p][ok] - tgt[D["widx"][p][ok]]
            r = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
            rabs = np.abs(n * e).sum(1)
            w = pr.huber_weight(r, delta)
            if "huber_unweighted" in V:
                w = np.ones_like(r)
            if "huber_squared" in V:
                w = w * w
            m = n @ (Rt.T if "normal_untransposed" in V else Rt)
            mabs = np.abs(n) @ np.abs(Rt)
            j = np.concatenate([m, np.cross(s, m)], 1)
            sa = np.abs(s)
            jabs = np.concatenate([mabs, np.stack([sa[:, 1] * mabs[:, 2] + sa[:, 2] * mabs[:, 1], sa[:, 2] * mabs[:, 0] + sa[:, 0] * mabs[:, 2],
                                                   sa[:, 0] * mabs[:, 1] + sa[:, 1] * mabs[:, 0]], 1)], 1)
            _, a = _terms(w, r, rabs, j.T, jabs.T)
            mag[p] = [0.0 if x is None else float(np.sum(x)) for x in a]
            mag[p, 27] = float(ok.sum())
            damp = 0.0 if "no_damping" in V else pr.DAMPING
            mag[p, list(DIAG)] += damp
            if V:
                t, _ = _terms(w, r, rabs, j.T, jabs.T)
                out[p] = [0.0 if x is None else float(np.sum(x)) for x in t]
                out[p, 27] = float(ok.sum())
                out[p, list(DIAG)] += damp
            else:     # the yardstick: record_one itself, fed the same inputs (its own discrete part is asserted equal)
                rec, slot, st, _ = pr.record_one(src, tgt, nrm, cand, Rt, tt, max_dist, delta)
                assert np.array_equal(slot, D["win"][p]) and st[0] == ok.sum(), "record_one's discrete part differs"
                out[p] = vec29(rec[None], st[None])[0]
    return out, mag


def sums_mp(src, tgt, nrm, cand, poses, delta, D, particles):
    """(values, sum|term|) [n][29] lists of mpf for the particles of `particles`, unrounded at DPS digits."""
    import mpmath
    mpmath.mp.dps = DPS
    mpf = mpmath.mpf
    B = src.shape[0]
    S = [[mpf(float(v)) for v in row] for row in src]
    dl = mpf(float(delta)) if np.isfinite(delta) else None
    damp = mpf(float(pr.DAMPING))
    out, mag = [], []
    for p in particles:
        R = [[mpf(float(poses[p, 3 * i + k])) for k in range(3)] for i in range(3)]
        acc, ab = [mpf(0)] * NS, [mpf(0)] * NS
        for b in range(B):
            if not D["ok"][p, b]:
                continue
            t = int(D["widx"][p, b])
            n = [mpf(float(v)) for v in nrm[t]]
            e = [mpf(float(D["Ts"][p, b, i])) - mpf(float(tgt[t, i])) for i in range(3)]
            ne = [n[i] * e[i] for i in range(3)]
            r, rabs = ne[0] + ne[1] + ne[2], abs(ne[0]) + abs(ne[1]) + abs(ne[2])
            w = mpf(1) if (dl is None or abs(r) <= dl) else dl / abs(r)
            m = [R[0][i] * n[0] + R[1][i] * n[1] + R[2][i] * n[2] for i in range(3)]
            ma = [abs(R[0][i] * n[0]) + abs(R[1][i] * n[1]) + abs(R[2][i] * n[2]) for i in range(3)]
            s = S[b]
            j = m + [s[1] * m[2] - s[2] * m[1], s[2] * m[0] - s[0] * m[2], s[0] * m[1] - s[1] * m[0]]
            ja = ma + [abs(s[1]) * ma[2] + abs(s[2]) * ma[1], abs(s[2]) * ma[0] + abs(s[0]) * ma[2], abs(s[0]) * ma[1] + abs(s[1]) * ma[0]]
            tv, ta = _terms(w, r, rabs, j, ja)
            tv[27] = ta[27] = mpf(1)
            for i in range(NS):
                acc[i] += tv[i]; ab[i] += ta[i]
        for i in DIAG:
            acc[i] += damp; ab[i] += damp
        out.append(acc); mag.append(ab)
    return out, mag


def signed_error_f64(v64, mp_sums, mp_mag):
    """eps [n][29] float32 = (v_mp - v_f64) / max(sum|term|_mp, 1e-300), formed in mpmath: |eps| is the restatement's E."""
    import mpmath
    tiny = mpmath.mpf(TINY)
    return np.array([[float((m - mpmath.mpf(float(v))) / max(a, tiny)) for m, v, a in zip(rm, rv, ra)]
                     for rm, rv, ra in zip(mp_sums, v64, mp_mag)], np.float32)


def error_against_mp(v, v64, mag, eps):
    """E [n][29] of values v against mpmath, held as v_mp = v_f64 + eps mag (v - v_f64 is formed first: exact for neighbours)."""
    with np.errstate(all="ignore"):
        return np.abs((np.asarray(v, np.float64) - v64) / mag - eps.astype(np.float64))


def group_max(e):
    return {g: float(e[:, list(ix)].max()) for g, ix in GROUPS}
