"""The two sum_h sums of tests/particle_score_objective_reference.py in mpmath at 60 digits, in the style of
tests/gicp_mp_reference.py (test infrastructure; tests/test_particle_score_objective_cpu.py).

The discrete part (winner, classes, accepted) is the float64 restatement's: the cases that use this assert it far from every
edge.  The yardstick of a particle's sum is  mag = sum over the accepted pairs of cond * |term|,  |term| taken factor by factor:
|n|.|e| squared for the plane form (cond = 1), |u| |W| |u| for the GICP form with cond = cond(S) of the pair — a closed-form
inverse of a 3 x 3 returns S^-1 (1 + theta) with |theta| of a few cond(S) u, as gicp_mp_reference.py argues.  Beyond delta the
term delta (2 x - delta) is at most 2 delta / x times x^2 <= 2 x^2, which the same yardstick covers with a factor 2.
"""
import numpy as np

import particle_score_objective_reference as po

DPS = 60


def sum_h_mp(form, pr, poses, gate, normals, src_normals=None, delta=np.inf, eps=1e-3, particles=None):
    """(values [n], mag [n]) lists of mpf: sum h over the accepted pairs of each particle, unrounded at DPS digits, from the
    float64 transformed points pr.T (the contract's T is a float64 quantity) and the float64 clouds and normals."""
    import mpmath
    mpmath.mp.dps = DPS
    mpf = mpmath.mpf
    t = po.terms(form, pr, poses, gate, normals, src_normals, delta, eps)
    P = pr.T.shape[0]
    particles = range(P) if particles is None else particles
    poses = np.asarray(poses, np.float64).reshape(-1, 12)
    dl = mpf(delta) if np.isfinite(delta) else None
    ep = mpf(eps)
    a = 1 - ep
    nrm = np.asarray(normals, np.float64)
    out, mag = [], []
    for p in particles:
        R = [[mpf(float(poses[p, 3 * i + k])) for k in range(3)] for i in range(3)]
        acc, ab = mpf(0), mpf(0)
        for b in np.flatnonzero(t.accepted[p]):
            e = [mpf(float(v)) for v in pr.e[p, b]]
            n = [mpf(float(v)) for v in nrm[pr.idx[p, b]]]
            if form == po.PLANE:
                r = sum(n[i] * e[i] for i in range(3))
                x, x2 = abs(r), r * r
                m2 = sum(abs(n[i] * e[i]) for i in range(3)) ** 2
            else:
                ns = [mpf(float(v)) for v in src_normals[b]]
                u = [R[0][i] * e[0] + R[1][i] * e[1] + R[2][i] * e[2] for i in range(3)]
                m = [R[0][i] * n[0] + R[1][i] * n[1] + R[2][i] * n[2] for i in range(3)]
                ua = [abs(R[0][i] * e[0]) + abs(R[1][i] * e[1]) + abs(R[2][i] * e[2]) for i in range(3)]
                S = mpmath.matrix(3, 3)
                for i in range(3):
                    for k in range(3):
                        S[i, k] = (2 if i == k else 0) - a * (m[i] * m[k] + ns[i] * ns[k])
                W = 2 * ep * S ** -1
                ev = mpmath.eigsy(S, eigvals_only=True)
                cond = max(abs(v) for v in ev) / min(abs(v) for v in ev)
                x2 = sum(u[i] * W[i, k] * u[k] for i in range(3) for k in range(3))
                x = mpmath.sqrt(x2)
                m2 = cond * sum(ua[i] * abs(W[i, k]) * ua[k] for i in range(3) for k in range(3))
            inside = dl is None or x <= dl
            acc += x2 if inside else dl * (2 * x - dl)
            ab += m2 if inside else 2 * m2
        out.append(acc); mag.append(ab)
    return out, mag
