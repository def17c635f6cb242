"""Stage B of one iteration, restated from the reference's source for two arithmetics (test infrastructure).

Stage B turns (source point, particle) pairs into the 22 Gauss-Newton sums per particle.  Written from the reference, not
from the kernels and not from oracle/svnicp_oracle.c:

    total pose, transform          SVNICP.cpp:58-64
    nearest of the K candidates    SVGDICP.cpp:300-329   (KNearestNeighborIdx with K = 1: strict '<' from the first candidate)
    point_filter                   SVGDICP.cpp:331-333   (the SQUARED distance against max_dist; rows multiplied by the mask)
    error, weight, J, H and b      SVNICP.cpp:116-157    (as the 22 raw sums of stein_iter.hip:16-21)
    SVGD-ICP's row count           SVGDICP.cpp:404       (count_nonzero of the masked transformed rows summed over xyz)

Two parts.  The DISCRETE part is defined in float64 and is exact: Ts = ((s0 R[i][0] + s1 R[i][1]) + s2 R[i][2]) + t_i unfused,
d2 = (dx dx + dy dy) + dz dz, argmin over the slots with strict '<' from slot 0, mask = d2 < max_dist, count =
mask and ((T0 + T1) + T2) != 0 — vectorised numpy with explicit elementwise expressions (no matmul, no einsum: their order
is not the reference's).  The REAL-VALUED part takes the discrete part's Ts, winners and masks as given and forms the 22
sums and the sum of |term| of each: `sums_mp` in mpmath at 60 digits, `sums_f64` in IEEE double, one rounding per operation,
rows added left to right.  E(v) = |v - v_mp| / max(sum|term|_mp, 1e-300); the float64 restatement's E is the yardstick.

VARIANTS are deliberately wrong float64 programs the CPU test must see refused.
"""
from fractions import Fraction

import numpy as np

DPS = 60
NS = 22
GROUPS = (("w", (0,)), ("ws", (1, 2, 3)), ("wss", (4, 5, 6, 7, 8, 9)), ("we", (10, 11, 12)), ("wes", tuple(range(13, 22))))
VARIANTS = ("argmin_le", "mask_le", "mask_squared", "reject_dropped", "weight_unsquared", "weight_on_rejected", "count_on_mask",
            "transform_fused", "anchor_nearest", "sum_f32")


def _fma(a, b, c):
    """Correctly rounded a b + c, elementwise (exact rationals: the CPU test's small arrays only)."""
    a, b, c = np.broadcast_arrays(a, b, c)
    out = np.empty(a.shape, np.float64)
    for i in np.ndindex(a.shape):
        out[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out


def transform(src, poses, variant=()):
    """Ts [P][B][3] of SVNICP.cpp:62-64 in float64: poses [P][12] = R row-major, then t."""
    s0, s1, s2 = (src[None, :, i] for i in range(3))
    out = np.empty((poses.shape[0], src.shape[0], 3), np.float64)
    for i in range(3):
        r0, r1, r2, t = (poses[:, c, None] for c in (3 * i, 3 * i + 1, 3 * i + 2, 9 + i))
        if "transform_fused" in variant:
            out[:, :, i] = _fma(s2, r2, _fma(s1, r1, _fma(s0, r0, t)))
        else:
            out[:, :, i] = ((s0 * r0 + s1 * r1) + s2 * r2) + t
    return out


def discrete(src, tgt, cand, poses, max_dist, variant=()):
    """The discrete part: dict(Ts [P][B][3], win [P][B] slot, d2 [P][B] of the winner, q [P][B][3] its coordinates,
    mask [P][B], cnt [P][B] SVGD-ICP's counted rows, tie [P][B] the least d2 is reached by more than one slot)."""
    V = frozenset(variant)
    Ts = transform(src, poses, V)
    P, B, K = poses.shape[0], src.shape[0], cand.shape[1]
    best = np.full((P, B), np.inf)
    win = np.zeros((P, B), np.int64)
    nmin = np.zeros((P, B), np.int64)
    for k in range(K):
        q = tgt[cand[:, k]][None]
        dx, dy, dz = (Ts[:, :, i] - q[:, :, i] for i in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        better = (d2 <= best) if "argmin_le" in V else (d2 < best)
        if k == 0:
            better = np.ones_like(better)
        if "anchor_nearest" in V and k > 0:
            better = np.zeros_like(better)
        nmin = np.where(d2 < best, 1, nmin + (d2 == best))
        win = np.where(better, k, win)
        best = np.where(better, d2, best)
    q = tgt[cand[np.arange(B)[None, :], win]]
    lim = max_dist * max_dist if "mask_squared" in V else max_dist
    mask = (best <= lim) if "mask_le" in V else (best < lim)
    nz = ((Ts[:, :, 0] + Ts[:, :, 1]) + Ts[:, :, 2]) != 0.0
    cnt = mask.copy() if "count_on_mask" in V else (mask & nz)
    return dict(Ts=Ts, win=win, d2=best, q=q, mask=mask, cnt=cnt, tie=nmin > 1)


def _terms(w, we, s):
    """The 22 terms of one row from w, we [3] and the (masked) source row s [3], in the record's order."""
    ws = [w * s[0], w * s[1], w * s[2]]
    return ([w] + ws + [ws[0] * s[0], ws[0] * s[1], ws[0] * s[2], ws[1] * s[1], ws[1] * s[2], ws[2] * s[2]] + list(we) +
            [we[i] * s[j] for i in range(3) for j in range(3)])


def sums_f64(src, D, max_dist, svgd=False, variant=()):
    """(sums [P][22], sum|term| [P][22]) in float64, every particle at once, rows added left to right."""
    V = frozenset(variant)
    dt = np.float32 if "sum_f32" in V else np.float64
    P, B = D["mask"].shape
    acc, mag = np.zeros((P, 1, NS), dt), np.zeros((P, 1, NS), dt)
    d = np.float64(max_dist)
    CH = 512      # rows per chunk; np.cumsum adds sequentially, so the chunks' carry keeps the order left to right
    with np.errstate(all="ignore"):
        for b0 in range(0, B, CH):
            r = slice(b0, min(B, b0 + CH))
            m = D["mask"][:, r].astype(np.float64)
            s = [m * src[None, r, i] for i in range(3)]                      # point_filter: the rows times the mask
            e = [m * D["Ts"][:, r, i] - m * D["q"][:, r, i] for i in range(3)]
            n = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])            # torch::norm(error, 2, 2)
            if "weight_on_rejected" in V:
                n = np.sqrt(D["d2"][:, r])
            w = d / (d + 3.0 * n)
            if "weight_unsquared" not in V:
                w = w * w
            if "reject_dropped" in V:
                w = w * m
            t = _terms(w, [w * e[i] for i in range(3)], s)
            if svgd:
                t[4] = D["cnt"][:, r].astype(np.float64)
            t = np.stack(t, -1).astype(dt)                                    # [P][rows][22]
            acc = np.cumsum(np.concatenate([acc, t], 1), axis=1, dtype=dt)[:, -1:]
            mag = np.cumsum(np.concatenate([mag, np.abs(t)], 1), axis=1, dtype=dt)[:, -1:]
    return acc[:, 0].astype(np.float64), mag[:, 0].astype(np.float64)


def sums_mp(src, D, max_dist, particles, svgd=False):
    """The same for the particles of `particles` in mpmath at DPS digits, unrounded: (sums, sum|term|), [n][22] lists of mpf."""
    import mpmath
    mpmath.mp.dps = DPS
    mpf = mpmath.mpf
    d = mpf(float(max_dist))
    one = mpf(1)
    out, mag = [], []
    B = D["mask"].shape[1]
    S = [[mpf(float(v)) for v in src[b]] for b in range(B)]
    for p in particles:
        acc, ab = [mpf(0)] * NS, [mpf(0)] * NS
        for b in range(B):
            if not D["mask"][p, b]:      # a rejected row is all zeros: e = 0, w = (d / d)^2 = 1, and it adds 1 to the first sum
                acc[0] += one; ab[0] += one
                continue
            e = [mpf(float(D["Ts"][p, b, i])) - mpf(float(D["q"][p, b, i])) for i in range(3)]
            n = mpmath.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
            w = (d / (d + 3 * n)) ** 2
            t = _terms(w, [w * e[i] for i in range(3)], S[b])
            if svgd:
                t[4] = one if D["cnt"][p, b] else mpf(0)
            for i in range(NS):
                acc[i] += t[i]; ab[i] += abs(t[i])
        out.append(acc); mag.append(ab)
    return out, mag


def signed_error_f64(v64, mp_sums, mp_mag):
    """(eps, rho) of the float64 sums v64 [n][22] against the mpmath sums: eps = (v_mp - v_f64) / max(sum|term|_mp, 1e-300),
    formed in mpmath and rounded to float32 — |eps| is the float64 restatement's E; rho = sum|term|_mp / sum|term|_f64 is not
    formed here (see make_stage_b.py)."""
    import mpmath
    tiny = mpmath.mpf("1e-300")
    return np.array([[float((m - mpmath.mpf(float(v))) / max(a, tiny)) for m, v, a in zip(rm, rv, ra)]
                     for rm, rv, ra in zip(mp_sums, v64, mp_mag)], np.float32)


def error_against_mp(v, v64, mag, eps):
    """E [n][22] of sums v against the mpmath sums, which the fixture holds as v_mp = v_f64 + eps mag: |v - v_mp| / mag with
    v - v_f64 formed first (exact for neighbours).  mag is sum|term|_mp floored at 1e-300."""
    with np.errstate(all="ignore"):
        return np.abs((np.asarray(v, np.float64) - v64) / mag - eps.astype(np.float64))


def group_max(e):
    """{sum group: largest E} of an [n][22] array of E."""
    return {g: float(e[:, list(ix)].max()) for g, ix in GROUPS}


def mp_particles(P, shard=None):
    """The particles that get mpmath: 0 and P - 1, both sides of every multiple of 16 (and so of 64) below P, the first and
    the last particle of a shard."""
    s = {0, P - 1}
    for m in range(16, P, 16):
        s.update((m - 1, m))
    if shard is not None:
        s.update((shard[0], shard[1] - 1))
    lo, hi = shard if shard is not None else (0, P)
    return np.array(sorted(p for p in s if lo <= p < hi), np.int64)
