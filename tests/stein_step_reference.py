"""The SVN Stein step of one iteration, restated from the reference's source for two arithmetics (test infrastructure).

Everything after the 22 Gauss-Newton sums per particle: H, b, the Newton step, the RBF bandwidth from the lower median, the
Stein direction, the pose update, the float32 early-stop compare and the history row.  Written from
src/core/SVNICP.cpp of the reference (line numbers below), not from oracle/svnicp_oracle.c and not from the kernels:

    H, b from the 22 sums         SVNICP.cpp:145-157 with the sums as stein_iter.hip:15-19 defines them
    Newton step                   SVNICP.cpp:162          (solve)
    Exp and left Jacobian         SVNICP.cpp:166-194      (so3_exp)
    Log                           SVNICP.cpp:196-215      (so3_log)
    bandwidth, kernel             SVNICP.cpp:254-266      (rbf)
    default / full direction      SVNICP.cpp:218-227 / 229-252
    pose update                   SVNICP.cpp:268-279
    early stop, history           SVNICP.cpp:42,95-107

`MP` runs it in mpmath at 60 digits (mp.lu_solve / mp.inverse for the solves, a full sort for the median): the reference of
tests/golden/stein_step.npz.  `F64` runs the same text in IEEE double with a hand-written LU: the "plain float64 step" whose
deliberately wrong variants (VARIANTS) the CPU test must see rejected.  Discrete outcomes are taken the way the reference's
double program takes them: a squared distance that overflows a double is +inf, NaN poisons the median (torch::median), the
stop compare is done on values rounded to float32, a singular solve gives NaN.
"""
import numpy as np

DPS = 60
QUANTITIES = ("H", "b", "N", "phi", "h", "pose", "pose_t", "hist")   # pose_t: the translation rows of the new pose alone
VARIANTS = ("median_upper", "median_ij", "lu_no_exchange", "lu_pivot_ge", "log_no_clamp", "no_guards", "stop_f64",
            "ksum_no_diag", "pose_old_R", "rank_reverse", "adam_no_bias")
OPTIMIZERS = ("Adam", "RMSprop", "SGD", "Adagrad")


class F64:
    """IEEE double, one rounding per operation (numpy scalars; the caller silences the floating-point warnings)."""
    name = "f64"
    nan, inf = np.float64("nan"), np.float64("inf")

    def __init__(self, variant=()):
        self.V = frozenset(variant)

    def c(self, x):
        return np.float64(x)

    sqrt, sin, cos, exp, log = (staticmethod(f) for f in (np.sqrt, np.sin, np.cos, np.exp, np.log))

    @staticmethod
    def acos(x):
        return np.arccos(x)

    @staticmethod
    def div(a, b):
        return np.float64(a) / np.float64(b)

    @staticmethod
    def key(sq):
        return sq

    @staticmethod
    def dbl(x):
        return float(x)

    def _lu(self, M):
        """LU with partial pivoting, first largest entry wins (LAPACK getrf)."""
        A = [[np.float64(M[6 * r + c]) for c in range(6)] for r in range(6)]
        piv, ok = [], True
        for k in range(6):
            p, mx = k, abs(A[k][k])
            if "lu_no_exchange" not in self.V:
                for r in range(k + 1, 6):
                    v = abs(A[r][k])
                    if (v >= mx) if "lu_pivot_ge" in self.V else (v > mx):
                        mx, p = v, r
            piv.append(p)
            A[k], A[p] = A[p], A[k]
            if A[k][k] == 0.0:
                ok = False
            inv = np.float64(1.0) / A[k][k]
            for r in range(k + 1, 6):
                A[r][k] = A[r][k] * inv
                for c in range(k + 1, 6):
                    A[r][c] = A[r][c] - A[r][k] * A[k][c]
        return A, piv, ok

    @staticmethod
    def _lu_solve(A, piv, rhs):
        x = [np.float64(v) for v in rhs]
        for k in range(6):
            x[k], x[piv[k]] = x[piv[k]], x[k]
        for r in range(1, 6):
            for c in range(r):
                x[r] = x[r] - A[r][c] * x[c]
        for r in range(5, -1, -1):
            for c in range(r + 1, 6):
                x[r] = x[r] - A[r][c] * x[c]
            x[r] = x[r] / A[r][r]
        return x

    def solve(self, M, rhs):
        A, piv, ok = self._lu(M)
        return self._lu_solve(A, piv, rhs) if ok else [self.nan] * 6

    def inv(self, M):
        A, piv, ok = self._lu(M)
        if not ok:
            return [self.nan] * 36
        out = [None] * 36
        for c in range(6):
            col = self._lu_solve(A, piv, [1.0 if r == c else 0.0 for r in range(6)])
            for r in range(6):
                out[6 * r + c] = col[r]
        return out

    def pivots(self, M):
        """(pivot rows, a tie for the pivot was seen) of the LU of M: the cases assert their regime with it."""
        A = [[np.float64(M[6 * r + c]) for c in range(6)] for r in range(6)]
        piv, tie = [], False
        for k in range(6):
            col = [abs(A[r][k]) for r in range(k, 6)]
            mx = max(col)
            tie = tie or (mx > 0 and sum(1 for v in col if v == mx) > 1)
            p = k + col.index(mx)
            piv.append(p)
            A[k], A[p] = A[p], A[k]
            if A[k][k] == 0.0:
                return piv + [None] * (5 - k), tie
            for r in range(k + 1, 6):
                A[r][k] = A[r][k] / A[k][k]
                for c in range(k + 1, 6):
                    A[r][c] = A[r][c] - A[r][k] * A[k][c]
        return piv, tie


class MP:
    """mpmath at DPS digits.  No signed zeros, no overflow: div() and key() supply what the double program would see."""
    name = "mp"

    def __init__(self):
        import mpmath
        self.m = mpmath
        self.m.mp.dps = DPS
        self.V = frozenset()
        self.nan, self.inf = mpmath.nan, mpmath.inf
        self.sqrt, self.sin, self.cos, self.exp, self.log, self.acos = (mpmath.sqrt, mpmath.sin, mpmath.cos, mpmath.exp,
                                                                        mpmath.log, mpmath.acos)

    def c(self, x):
        return self.m.mpf(float(x))

    def div(self, a, b):
        if b == 0:
            if a != a or a == 0:
                return self.nan
            return self.inf if a > 0 else -self.inf
        return a / b

    def key(self, sq):
        return self.inf if sq == sq and float(sq) == float("inf") else sq

    @staticmethod
    def dbl(x):
        return float(x)

    @staticmethod
    def _bad(vals):
        return any(v != v for v in vals)

    def solve(self, M, rhs):
        if self._bad(M) or self._bad(rhs):
            return [self.nan] * 6
        try:
            x = self.m.lu_solve(self.m.matrix([list(M[6 * r:6 * r + 6]) for r in range(6)]), self.m.matrix(list(rhs)))
        except ZeroDivisionError:   # exactly singular
            return [self.nan] * 6
        return [x[i] for i in range(6)]

    def inv(self, M):
        if self._bad(M):
            return [self.nan] * 36
        try:
            X = self.m.inverse(self.m.matrix([list(M[6 * r:6 * r + 6]) for r in range(6)]))
        except ZeroDivisionError:
            return [self.nan] * 36
        return [X[r, c] for r in range(6) for c in range(6)]


def reduce_sums(sums, reverse=False):
    """[W][P][22] -> [P][22]: the rank records added in rank order, in double (svnicp_hip.h: svnicp_set_row_shard)."""
    s = np.asarray(sums, np.float64)
    order = range(s.shape[0] - 1, -1, -1) if reverse else range(s.shape[0])
    acc = None
    for w in order:
        acc = s[w].copy() if acc is None else acc + s[w]
    return acc


def so3_exp(A, r):
    """SVNICP.cpp:166-194: R = cos I + (1 - cos) a a^T + sin a^, J_l = sin/angle I + (1 - sin/angle) a a^T + (1 - cos)/angle a^."""
    angle = A.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if angle < 1e-12 and "no_guards" not in A.V:   # :171-173
        a = [A.c(0.0)] * 3
    else:
        a = [A.div(r[i], angle) for i in range(3)]
    c, s = A.cos(angle), A.sin(angle)
    z = A.c(0.0)
    ah = [z, -a[2], a[1], a[2], z, -a[0], -a[1], a[0], z]
    soa, omc = A.div(s, angle), A.div(1 - c, angle)   # 0 / 0 at a zero step (:188,192)
    R, J = [None] * 9, [None] * 9
    for i in range(3):
        for j in range(3):
            eye = A.c(1.0 if i == j else 0.0)
            aa = a[i] * a[j]
            R[3 * i + j] = (c * eye + (1 - c) * aa) + s * ah[3 * i + j]
            J[3 * i + j] = (soa * eye + (1 - soa) * aa) + omc * ah[3 * i + j]
    return R, J


def so3_log(A, R):
    """SVNICP.cpp:196-215."""
    c = A.c(0.5) * (R[0] + R[4] + R[8] - 1)
    if "log_no_clamp" not in A.V:   # torch::clip: NaN stays NaN
        c = A.c(-1.0) if c < -1 else c
        c = A.c(1.0) if c > 1 else c
    angle = A.acos(c)
    sa = A.sin(angle)
    nonzero = bool(abs(sa) > 1e-12) or "no_guards" in A.V   # :205
    f = A.div(A.c(0.5), sa if nonzero else A.c(1.0)) * angle
    w = [f * (R[7] - R[5]), f * (R[2] - R[6]), f * (R[3] - R[1])]
    return w if nonzero else [A.c(0.0)] * 3


def mat3_mul(a, b):
    return [a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j] for i in range(3) for j in range(3)]


def mat3_vec(a, v):
    return [a[3 * i] * v[0] + a[3 * i + 1] * v[1] + a[3 * i + 2] * v[2] for i in range(3)]


def finalize_Hb(A, s, Rc):
    """H = sum J^T w J + 1e-6 I, b = sum J^T (w e) with J = [Rc | -Rc s^] (SVNICP.cpp:145-157) from the 22 sums."""
    sw, a = s[0], s[1:4]
    xx, xy, xz, yy, yz, zz = s[4:10]
    tr = xx + yy + zz
    z = A.c(0.0)
    H = [z] * 36
    H[0] = H[7] = H[14] = sw
    H[4], H[5], H[6 + 3], H[6 + 5], H[12 + 3], H[12 + 4] = a[2], -a[1], -a[2], a[0], a[1], -a[0]      # -sum w s^
    H[18 + 1], H[18 + 2], H[24 + 0], H[24 + 2], H[30 + 0], H[30 + 1] = -a[2], a[1], a[2], -a[0], -a[1], a[0]   # +sum w s^
    H[21], H[22], H[23] = tr - xx, -xy, -xz
    H[27], H[28], H[29] = -xy, tr - yy, -yz
    H[33], H[34], H[35] = -xz, -yz, tr - zz
    for i in range(6):
        H[7 * i] = H[7 * i] + A.c(1e-6)   # :153
    RcT = [Rc[3 * j + i] for i in range(3) for j in range(3)]
    bt = mat3_vec(RcT, s[10:13])
    G = mat3_mul(RcT, s[13:22])   # Rc^T C, C[i][j] = sum (w e)_i s_j
    return H, bt + [G[7] - G[5], G[2] - G[6], G[3] - G[1]]


def rbf(A, x, P):
    """SVNICP.cpp:254-266: squared pair distances, h = lower median / log(P + 1), K = exp(-sq / h)."""
    sq = [[A.c(0.0)] * P for _ in range(P)]
    for i in range(P):
        for j in range(i):
            v = A.c(0.0)
            for d in range(6):
                df = x[i][d] - x[j][d]
                v = v + df * df
            sq[i][j] = sq[j][i] = A.key(v)
        v = A.c(0.0)
        for d in range(6):
            df = x[i][d] - x[i][d]   # inf - inf on the diagonal of a non-finite particle
            v = v + df * df
        sq[i][i] = v
    if "median_ij" in A.V:
        keys = [sq[i][j] for i in range(P) for j in range(i + 1, P)]
    else:
        keys = [sq[i][j] for i in range(P) for j in range(P)]
    if any(k != k for k in keys):
        med = A.nan   # torch::median propagates NaN
    else:
        keys.sort()
        med = keys[len(keys) // 2 if "median_upper" in A.V else (len(keys) - 1) // 2]
    h = A.div(med, A.log(A.c(P + 1)))
    K = [[A.exp(A.div(-sq[i][j], h)) for j in range(P)] for i in range(P)]
    return K, h, med


def direction_default(A, x, N, Hs, P):
    """SVNICP.cpp:85,218-227."""
    K, h, med = rbf(A, x, P)
    Hm = [A.c(0.0)] * 36
    for p in range(P):
        Hm = [Hm[e] + Hs[p][e] for e in range(36)]
    Hm = [v / P for v in Hm]
    Hinv = A.inv(Hm)
    phi = []
    two_h = A.div(A.c(2.0), h)
    for i in range(P):
        g, kn, ks = [A.c(0.0)] * 6, [A.c(0.0)] * 6, A.c(0.0)
        for j in range(P):
            k = K[i][j]
            g = [g[d] + (x[i][d] - x[j][d]) * k for d in range(6)]
            kn = [kn[d] + k * (-N[j][d]) for d in range(6)]
            if not ("ksum_no_diag" in A.V and i == j):
                ks = ks + k
        g = [two_h * v for v in g]
        row = []
        for r in range(6):
            hg = A.c(0.0)
            for c in range(6):
                hg = hg + Hinv[6 * r + c] * g[c]
            row.append(A.div(kn[r] + hg, ks))
        phi.append(row)
    return phi, h, med, dict(Hmean=Hm)


def direction_full(A, x, b, Hs, P, lr):
    """SVNICP.cpp:229-252."""
    K, h, med = rbf(A, x, P)
    two_h = A.div(A.c(2.0), h)
    phi, Hms = [], []
    for i in range(P):
        Hm, u = [A.c(0.0)] * 36, [A.c(0.0)] * 6
        for j in range(P):
            k = K[i][j]
            g = [two_h * ((x[i][d] - x[j][d]) * k) for d in range(6)]
            k2 = k * k
            Hm = [Hm[6 * r + c] + (k2 * Hs[j][6 * r + c] + g[r] * g[c]) for r in range(6) for c in range(6)]
            u = [u[r] + (k * (-b[j][r]) + g[r]) for r in range(6)]
        Hm = [v / P for v in Hm]
        u = [v / P for v in u]
        Hi = A.inv(Hm)
        row = []
        for r in range(6):
            acc = A.c(0.0)
            for c in range(6):
                acc = acc + Hi[6 * r + c] * u[c]
            row.append(A.c(lr) * acc)
        phi.append(row)
        Hms.append(Hm)
    return phi, h, med, dict(Hm=Hms)


def svn_step(A, init, sums, full_grad, lr, check_early_stop, thr):
    """One SVN iteration on `init` [6][P] (t ; rotation vector) and the reduced sums [P][22].  Returns a dict of float64
    arrays H [P][36], b, N, phi [P][6], h, pose [6][P], hist float32 [6 P], stop, med, and `aux` (intermediates in A)."""
    init = np.asarray(init, np.float64)
    P = init.shape[1]
    with np.errstate(all="ignore"):
        Rs, ts, xs, Hs, bs, Ns = [], [], [], [], [], []
        for p in range(P):
            R, _ = so3_exp(A, [A.c(init[3 + d, p]) for d in range(3)])   # :34
            t = [A.c(init[d, p]) for d in range(3)]
            Rs.append(R); ts.append(t)
            xs.append(t + so3_log(A, R))                                  # :74-77
            H, b = finalize_Hb(A, [A.c(v) for v in sums[p]], R)           # R0 = I
            Hs.append(H); bs.append(b)
            Ns.append(A.solve(H, b))                                      # :162
        aux = {}
        if P > 1:
            if full_grad:
                phi, h, med, aux = direction_full(A, xs, bs, Hs, P, lr)
            else:
                phi, h, med, aux = direction_default(A, xs, Ns, Hs, P)
        else:
            phi, h, med = [[-v for v in Ns[0]]], A.nan, A.nan            # :89
        pose, norms = np.zeros((6, P)), []
        for p in range(P):                                                # :268-279
            dR, Jl = so3_exp(A, phi[p][3:])
            dt = mat3_vec(Jl, phi[p][:3])
            Rn = mat3_mul(Rs[p], dR)
            Rdt = mat3_vec(Rs[p] if "pose_old_R" in A.V else Rn, dt)
            xn = [Rdt[d] + ts[p][d] for d in range(3)] + so3_log(A, Rn)
            pose[:, p] = [A.dbl(v) for v in xn]
            n2 = A.c(0.0)
            for d in range(6):
                n2 = n2 + phi[p][d] * phi[p][d]
            norms.append(A.sqrt(n2))
        stop, mean = False, A.c(0.0)
        for n in norms:
            mean = mean + n
        mean = mean / P
        if check_early_stop:                                              # :42,95-101: lt(f64 0-dim, f32 1-dim) runs in float32
            stop = bool(mean < A.c(thr)) if "stop_f64" in A.V else bool(np.float32(A.dbl(mean)) < np.float32(thr))
        hist = np.zeros(6 * P, np.float32) if stop else pose.reshape(-1).astype(np.float32)   # :103-107
        arr = lambda rows: np.array([[A.dbl(v) for v in row] for row in rows], np.float64)
        aux.update(mean=mean, norms=norms, phi=phi, N=Ns, H=Hs)
        return dict(H=arr(Hs), b=arr(bs), N=arr(Ns), phi=arr(phi), h=np.float64(A.dbl(h)), med=np.float64(A.dbl(med)),
                    pose=pose, hist=hist, stop=stop, aux=aux)


def euler_partials(A, roll, pitch, yaw):
    """SVGDICP.cpp:335-396 with R0 = I: the partial derivatives of Rz(yaw) Ry(pitch) Rx(roll), row-major 3x3 each."""
    a, b, c, d, e, f = A.cos(yaw), A.sin(yaw), A.cos(pitch), A.sin(pitch), A.cos(roll), A.sin(roll)
    de, df, ac, af, ae = d * e, d * f, a * c, a * f, a * e
    ade, adf, bc, be, bf, bde = a * de, a * df, b * c, b * e, b * f, b * de
    z = A.c(0.0)
    pr = [z, ade + bf, be - adf, z, -af + bde, b * (-df) - ae, z, c * e, c * (-f)]
    pp = [a * -d, ac * f, ac * e, b * -d, bc * f, bc * e, -c, -df, -de]
    py = [-bc, -b * df - ae, af - bde, ac, -be + adf, ade + bf, z, z, z]
    return pr, pp, py


def optimizer_update(A, name, lr, g, v, st, step):
    """torch::optim with the options of SVGDICP.cpp:142-170 and torch's defaults, one parameter: (new value, new state);
    st = (first moment or square average, second moment or momentum buffer, Adagrad's sum)."""
    m1, m2, m3 = st
    if name == "Adam":       # betas (0.9, 0.999), eps 1e-8
        b1, b2 = A.c(0.9), A.c(0.999)
        m1 = b1 * m1 + (1 - b1) * g
        m2 = b2 * m2 + (1 - b2) * g * g
        bc1, bc2 = (A.c(1.0), A.c(1.0)) if "adam_no_bias" in A.V else (1 - b1 ** step, 1 - b2 ** step)
        v = v - A.div(A.c(lr), bc1) * A.div(m1, A.div(A.sqrt(m2), A.sqrt(bc2)) + A.c(1e-8))
    elif name == "RMSprop":  # alpha 0.99, eps 1e-8, weight_decay 1e-8, momentum 0.9
        g = g + A.c(1e-8) * v
        m1 = A.c(0.99) * m1 + (1 - A.c(0.99)) * g * g
        m2 = A.c(0.9) * m2 + A.div(g, A.sqrt(m1) + A.c(1e-8))
        v = v - A.c(lr) * m2
    elif name == "SGD":
        v = v - A.c(lr) * g
    else:                    # Adagrad: eps 1e-10, no decay
        m3 = m3 + g * g
        v = v - A.c(lr) * A.div(g, A.sqrt(m3) + A.c(1e-10))
    return v, (m1, m2, m3)


def svgd_steps(A, init, sums, lr, optimizer, n_src, steps=1):
    """`steps` consecutive SVGD-ICP iterations (SVGDICP.cpp:106-133, no early stop) on the parameters `init` [6][P]
    (x, y, z, roll, pitch, yaw), every one with the same reduced sums [P][22], whose slot 4 is the count of nonzero rows.
    sgd_grad :398-455 (R0 = I, normalize_factor_ = 1, gradient_scaling_factor_ = n_src), svgd_grad and rbf_kernel :457-474 on
    pose_particles_, pose_update :476-494.  Returns the LAST iteration's gradient (N), direction (phi) and h, and the pose."""
    init = np.asarray(init, np.float64)
    P = init.shape[1]
    with np.errstate(all="ignore"):
        eul = [[A.c(init[d, p]) for d in range(6)] for p in range(P)]
        state = [[(A.c(0.0), A.c(0.0), A.c(0.0)) for _ in range(6)] for _ in range(P)]
        for step in range(1, steps + 1):
            G = []
            for p in range(P):
                s = [A.c(v) for v in sums[p]]
                cnt1 = s[4] + 1                                           # :404,414
                row = [A.div(s[10 + j], cnt1) * A.c(n_src) for j in range(3)]
                for dR in euler_partials(A, eul[p][3], eul[p][4], eul[p][5]):
                    v = A.c(0.0)
                    for i in range(3):
                        for j in range(3):
                            v = v + dR[3 * i + j] * s[13 + 3 * i + j]
                    row.append(A.div(v, cnt1) * A.c(n_src))
                G.append(row)
            if P > 1:
                K, h, med = rbf(A, eul, P)
                two_h = A.div(A.c(2.0), h)
                phi = []
                for i in range(P):
                    gr, kg = [A.c(0.0)] * 6, [A.c(0.0)] * 6
                    for j in range(P):
                        k = K[i][j]
                        gr = [gr[d] + (eul[i][d] - eul[j][d]) * k for d in range(6)]
                        kg = [kg[d] + k * (-G[j][d]) for d in range(6)]
                    phi.append([(kg[d] + two_h * gr[d]) / P for d in range(6)])
            else:
                phi, h, med = [[-v for v in G[0]]], A.nan, A.nan          # :112
            for p in range(P):
                for d in range(6):
                    eul[p][d], state[p][d] = optimizer_update(A, optimizer, lr, -phi[p][d], eul[p][d], state[p][d], step)
        pose = np.array([[A.dbl(eul[p][d]) for p in range(P)] for d in range(6)], np.float64)
        arr = lambda rows: np.array([[A.dbl(v) for v in row] for row in rows], np.float64)
        nanHb = np.full((P, 36), np.nan), np.full((P, 6), np.nan)
        return dict(H=nanHb[0], b=nanHb[1], N=arr(G), phi=arr(phi), h=np.float64(A.dbl(h)), med=np.float64(A.dbl(med)),
                    pose=pose, hist=pose.reshape(-1).astype(np.float32), stop=False, aux={})


def same_median(h, med, P):
    """The exact comparison of the median's key: h log(P + 1) recovers `med` to 2 ulp (h itself carries the rounding of the
    logarithm and of the division); a zero, infinite or NaN median must come back as such."""
    h, med = np.float64(h), np.float64(med)
    if not np.isfinite(med) or med == 0:
        return bool(np.array_equal(h, med, equal_nan=True))
    return bool(np.isfinite(h) and abs(h * np.log(np.float64(P + 1)) - med) <= 2 * np.spacing(med))


def rel_err(v, ref):
    """E of the issue per particle (rows of a 2-D array; a scalar is one row): max |v - ref| / max(max |ref|, 1e-300) over the
    entries where the reference is finite.  The non-finite patterns must be equal: returns None where they are not."""
    v, ref = np.atleast_2d(np.asarray(v, np.float64)), np.atleast_2d(np.asarray(ref, np.float64))
    if v.shape != ref.shape:
        return None
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        same = np.where(fin, np.isfinite(v), (np.isnan(ref) & np.isnan(v)) | (ref == v))
    if not same.all():
        return None
    out = np.zeros(ref.shape[0])
    for r in range(ref.shape[0]):
        if fin[r].any():
            out[r] = np.abs(v[r][fin[r]] - ref[r][fin[r]]).max() / max(np.abs(ref[r][fin[r]]).max(), 1e-300)
    return out


def compared(out, q):
    """Quantity q of a step's outputs as rows per particle."""
    if q == "pose":
        return out["pose"].T
    if q == "pose_t":
        return out["pose"][:3].T
    if q == "hist":
        return np.asarray(out["hist"], np.float64).reshape(6, -1).T
    return out[q]


def errors(out, ref):
    """{quantity: max over particles of E}, None for a quantity whose non-finite pattern differs."""
    e = {}
    for q in QUANTITIES:
        x = rel_err(compared(out, q), compared(ref, q))
        e[q] = None if x is None else float(x.max())
    return e
