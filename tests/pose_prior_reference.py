"""The Gaussian pose prior on the correction (include/svnicp_hip.h "pose prior"), restated from its
contract for two arithmetics (test infrastructure).

    e = [t_p - mu_t ; Log(R_mu^T R_p)]      J = blkdiag(R_p, Jr^-1(e_r)),  Jr^-1(w) = I + 1/2 [w]x + c(theta) [w]x^2
    b <- b + J^T (Lambda e)                 H <- H + J^T Lambda J   (i <= j, mirrored)

`F64` (tests/stein_step_reference.py) runs it in IEEE double with the summation order DESIGN states (every sum over ascending
index, left to right, R_mu from the host's Rodrigues formula); `MP` runs the same text in mpmath at 60 digits with the exact
closed form of c and the exact Exp: the reference.  The base record is finalize_Hb of stein_step_reference (point mode) or a
given [42] record (plane mode).  Inputs are float64 values: the particle's R_p and t_p AS THE DEVICE HOLDS THEM, mean6, Lambda.
"""
import numpy as np

import stein_step_reference as ss

SERIES_THETA = 1e-2      # csrc/pose_prior.hip: kSeriesTheta
FACTOR, EPS = 16.0, 2.0 ** -52


def exp_host(A, r, guard=1e-12):
    """R_mu as svnicp_set_pose_prior stores it (csrc/pose_prior.hpp: exp_so3: the identity below 1e-12 rad); in mpmath the
    exact Rodrigues formula.  r: values of A."""
    r = [A.c(v) if isinstance(v, (float, np.floating)) else v for v in r]
    a = A.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    eye = [A.c(v) for v in (1, 0, 0, 0, 1, 0, 0, 0, 1)]
    if a < guard or a == 0:
        return eye
    z = A.c(0.0)
    K = [z, -r[2], r[1], r[2], z, -r[0], -r[1], r[0], z]
    s = A.sin(a) / a
    h = A.sin(A.c(0.5) * a) / a
    c = A.c(2.0) * h * h
    KK = ss.mat3_mul(K, K)
    return [(eye[i] + s * K[i]) + c * KK[i] for i in range(9)]


def jr_inv_c(A, th2):
    th = A.sqrt(th2)
    if A.name == "f64":
        if th < SERIES_THETA:
            return (A.c(1.0) / A.c(12.0) + th2 / A.c(720.0)) + (th2 * th2) / A.c(30240.0)
        return A.c(1.0) / th2 - (A.c(1.0) + A.cos(th)) / ((A.c(2.0) * th) * A.sin(th))
    if th == 0:
        return A.c(1.0) / 12
    return 1 / th2 - (1 + A.cos(th)) / (2 * th * A.sin(th))


def error_and_jacobian(A, Rp, tp, Rmu, mu_t):
    """e [6], Jr^-1 [9] at the pose (R_p, t_p); J = blkdiag(R_p, Jr^-1)."""
    e = [tp[i] - mu_t[i] for i in range(3)]
    E = [Rmu[i] * Rp[j] + Rmu[3 + i] * Rp[3 + j] + Rmu[6 + i] * Rp[6 + j] for i in range(3) for j in range(3)]
    w = ss.so3_log(A, E)
    e = e + w
    c = jr_inv_c(A, (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    z = A.c(0.0)
    W = [z, -w[2], w[1], w[2], z, -w[0], -w[1], w[0], z]
    W2 = ss.mat3_mul(W, W)
    Jr = [(A.c(1.0 if i % 4 == 0 else 0.0) + A.c(0.5) * W[i]) + c * W2[i] for i in range(9)]
    return e, Jr


def prior_terms(A, Rp, tp, Rmu, mu_t, L):
    """(g [6] = J^T Lambda e, G [36] = J^T Lambda J with G[i][j] computed for i <= j and mirrored)."""
    e, Jr = error_and_jacobian(A, Rp, tp, Rmu, mu_t)
    v = []
    for k in range(6):
        s = L[6 * k] * e[0]
        for m in range(1, 6):
            s = s + L[6 * k + m] * e[m]
        v.append(s)
    g = [None] * 6
    for j in range(3):
        g[j] = (Rp[j] * v[0] + Rp[3 + j] * v[1]) + Rp[6 + j] * v[2]
        g[3 + j] = (Jr[j] * v[3] + Jr[3 + j] * v[4]) + Jr[6 + j] * v[5]
    Am = [None] * 36
    for k in range(6):
        for j in range(3):
            Am[6 * k + j] = (L[6 * k] * Rp[j] + L[6 * k + 1] * Rp[3 + j]) + L[6 * k + 2] * Rp[6 + j]
            Am[6 * k + 3 + j] = (L[6 * k + 3] * Jr[j] + L[6 * k + 4] * Jr[3 + j]) + L[6 * k + 5] * Jr[6 + j]
    G = [None] * 36
    for i in range(6):
        Jb, ci, k0 = (Rp, i, 0) if i < 3 else (Jr, i - 3, 3)
        for j in range(i, 6):
            G[6 * i + j] = (Jb[ci] * Am[6 * k0 + j] + Jb[3 + ci] * Am[6 * (k0 + 1) + j]) + Jb[6 + ci] * Am[6 * (k0 + 2) + j]
            G[6 * j + i] = G[6 * i + j]
    return g, G


def record(A, base, R0, Rp, tp, mean6, L, plane=False):
    """The [42] record H | b of one particle: base = its 22 sums (point mode) or a finished [42] record (plane=True); R0 [9],
    Rp [9], tp [3], mean6 [6], L [36] float64.  L None: no prior (the base record alone).  A non-finite pose: all NaN."""
    if L is not None and not (np.all(np.isfinite(np.asarray(Rp, float))) and np.all(np.isfinite(np.asarray(tp, float)))):
        return [A.nan] * 36, [A.nan] * 6
    c = A.c
    Rpc, tpc = [c(v) for v in Rp], [c(v) for v in tp]
    if plane:
        H, b = [c(v) for v in base[:36]], [c(v) for v in base[36:42]]
    else:
        H, b = ss.finalize_Hb(A, [c(v) for v in base], ss.mat3_mul([c(v) for v in R0], Rpc))
    if L is None:
        return H, b
    g, G = prior_terms(A, Rpc, tpc, exp_host(A, mean6[3:6]), [c(v) for v in mean6[:3]], [c(v) for v in L])
    return [H[i] + G[i] for i in range(36)], [b[i] + g[i] for i in range(6)]


def records(A, bases, R0, R, t, mean6, L, plane=False):
    """[P][36], [P][6] float64 arrays of `record` over the particles."""
    Hs, bs = [], []
    with np.errstate(all="ignore"):
        for p in range(len(R)):
            H, b = record(A, bases[p], R0, R[p], t[p], mean6, L, plane)
            Hs.append([float(v) for v in H]); bs.append([float(v) for v in b])
    return np.array(Hs, np.float64), np.array(bs, np.float64)


def rel_err(v, ref):
    """max |v - ref| / max(max |ref|, 1e-300) over one particle's quantity; None when the non-finite patterns differ."""
    v, ref = np.asarray(v, np.float64), np.asarray(ref, np.float64)
    if not np.array_equal(np.isfinite(v), np.isfinite(ref)):
        return None
    m = np.isfinite(ref)
    if not m.any():
        return 0.0
    return float(np.abs(v[m] - ref[m]).max() / max(np.abs(ref[m]).max(), 1e-300))


def cost(A, Rp, tp, mean6, L):
    """1/2 e^T Lambda e at the pose (R_p, t_p), in arithmetic A (exact Exp of the mean in mpmath)."""
    e, _ = error_and_jacobian(A, Rp, tp, exp_host(A, mean6[3:6]), [A.c(v) for v in mean6[:3]])
    s = A.c(0.0)
    for i in range(6):
        for j in range(6):
            s = s + e[i] * A.c(L[6 * i + j]) * e[j]
    return s / 2


def perturbed(A, Rp, tp, d):
    """The right perturbation of the contract: R_p Exp(d_r), t_p + R_p d_t."""
    dR = exp_host(A, d[3:6], guard=0)
    Rn = ss.mat3_mul(Rp, dR)
    Rd = ss.mat3_vec(Rp, d[:3])
    return Rn, [tp[i] + Rd[i] for i in range(3)]


def run_scene(orc, src, tgt, nrm, init, K, iterations, max_dist, delta, mean6=None, L=None, R0=None, t0=None, svn_full_grad=False):
    """The plane-mode registration of tests/plane_reference.run with the prior added to every particle's record in float64
    (L None: no prior): the oracle's own split-phase Stein step (orc_sp_update) on the [P][42] record.  Returns plane_reference's
    PlaneRun (trace H, b include the prior, like the library's)."""
    import ctypes as C

    import plane_reference as plref
    A = ss.F64()
    src = np.ascontiguousarray(src, np.float64)
    tgt = np.ascontiguousarray(tgt, np.float64)
    R0 = np.eye(3) if R0 is None else np.asarray(R0, np.float64).reshape(3, 3)
    t0 = np.zeros(3) if t0 is None else np.asarray(t0, np.float64).reshape(3)
    s = orc.Solver(init, iterations=iterations, lr=1.0, max_dist=max_dist, check_early_stop=False, knn_count=K,
                   svn_full_grad=svn_full_grad)
    s.add_cloud(src, tgt, init)
    s.set_initial_mean(R0, t0)
    tr = s.enable_trace()
    lib, P, B = s.L, s.P, src.shape[0]
    lib.orc_sp_begin(s.h)
    cand, _ = orc.knn_topk(orc.transform(src, R0, t0), tgt, K)
    out = plref.PlaneRun()
    out.corr = np.full((iterations, P, B), -1, np.int32)
    rec = np.zeros((P, 42))
    Lf = None if L is None else [float(v) for v in np.asarray(L, np.float64).reshape(36)]
    for it in range(iterations):
        lib.orc_sp_finish(s.h)
        x = s.get_particles().reshape(6, P)
        for p in range(P):
            Rp = orc.so3_exp(x[3:, p])[0]
            Rt, tt = R0 @ Rp, t0 + R0 @ x[:3, p]
            base, out.corr[it, p], _, _ = plref.record_one(src, tgt, nrm, cand, Rt, tt, max_dist, delta)
            if Lf is None:
                rec[p] = base
            else:
                with np.errstate(all="ignore"):
                    H, b = record(A, base, R0.reshape(9), Rp.reshape(9), x[:3, p], mean6, Lf, plane=True)
                rec[p] = np.array([float(v) for v in H] + [float(v) for v in b])
        if lib.orc_sp_update(s.h, it, rec.ctypes.data_as(C.POINTER(C.c_double))):
            break
    lib.orc_sp_finish(s.h)
    out.H, out.b = tr["H"], tr["b"]
    out.particles = s.get_particles()
    out.solver = s
    return out
