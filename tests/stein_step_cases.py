"""Crafted inputs of the Stein step driven alone (test infrastructure; numpy only, deterministic, no GPU, no mpmath).

A case is a particle set, one record of 22 sums per (rank, particle), the gradient branch and the early-stop settings — and
the regime it claims to hit, which is asserted here, on the host, while the case is built (AssertionError, never a skip).
The sums need not come from any cloud: the step does not care.  With a zero initial rotation and R0 = I the sums give
b = (s[10:13], s[20] - s[18], s[15] - s[19], s[16] - s[14]) and H = [[sw I, -a^], [a^, tr I - S]] + 1e-6 I exactly.

all_cases() is what tests/golden/make_stein_step.py, tests/test_stein_step_cpu.py and tests/test_stein_step_gpu.py walk.
"""
from dataclasses import dataclass, field

import numpy as np

import stein_step_reference as ref

F = ref.F64()
FRONT_BUF, SEL_LDS_KEYS, HB_NB, HB_EXP0 = 2048, 16384, 48 * 256, 1023 - 40   # stein_step_device.hpp
PI = float(np.pi)
N_SRC = 256               # source rows of the context the GPU test makes: SVGD-ICP scales its gradient by it (SVGDICP.cpp:58,454)


@dataclass
class Case:
    name: str
    init: np.ndarray          # [6][P]: t ; rotation vector
    sums: np.ndarray          # [W][P][22]
    full: bool = False        # SVN_full_grad
    lr: float = 1.0
    es: bool = False          # check_early_stop
    thr: float = 1e-5
    regime: str = ""
    exact_h: bool = False     # translations on a binary grid: the median is one definite double
    well: bool = False        # every 6x6 of the case has a condition number below 1e4
    tags: tuple = ()
    info: dict = field(default_factory=dict)
    mode: str = "svn"         # "svgd": SVGD-ICP, init is (x, y, z, roll, pitch, yaw), slot 4 of the sums is the nonzero count
    optimizer: str = "Adam"
    steps: int = 1            # consecutive updates on one context (SVGD-ICP), all with the same sums

    @property
    def P(self):
        return self.init.shape[1]

    @property
    def W(self):
        return self.sums.shape[0]

    def reduced(self):
        return ref.reduce_sums(self.sums)

    def step(self, variant=()):
        """The plain float64 step (a wrong variant of it when asked)."""
        A = ref.F64(variant)
        if self.mode == "svgd":
            return ref.svgd_steps(A, self.init, self.reduced(), self.lr, self.optimizer, N_SRC, self.steps)
        return ref.svn_step(A, self.init, ref.reduce_sums(self.sums, reverse="rank_reverse" in A.V), self.full, self.lr,
                            self.es, self.thr)

    def checksum(self):
        """A fingerprint of the inputs, stored in the fixture."""
        import zlib
        blob = b"".join(np.ascontiguousarray(a, np.float64).tobytes() for a in (self.init, self.sums)) + \
            repr((self.full, float(self.lr), self.es, float(self.thr), self.mode, self.optimizer, self.steps)).encode()
        return np.int64(zlib.crc32(blob))


def shapes(P):
    """Launch shapes that admit P particles: name -> options (svnicp_set_option), see registration_plan.hpp: plan_step."""
    if P == 1:
        return {"single": (("single", "split"),)}
    if P <= 128:
        return {"inline": (("chain", "general"),),
                "stream": (("chain", "general"), ("median", "stream")),
                "hist": (("chain", "general"), ("fused_update_max_p", 1)),
                "fused": (("update", "fused"),)}
    return {"hist": (("chain", "general"),), "fused": (("update", "fused"), ("fused_update_max_p", P))}


def sums_row(sw=1.0, a=(0, 0, 0), S=(.5, 0, 0, .5, 0, .5), bt=(0, 0, 0), br=(0, 0, 0)):
    s = np.zeros(22)
    s[0], s[1:4], s[4:10], s[10:13] = sw, a, S, bt
    s[20], s[15], s[16] = br
    return s


def hmat(s):
    with np.errstate(all="ignore"):
        H, _ = ref.finalize_Hb(F, [np.float64(v) for v in s], [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0])
    return [float(v) for v in H]


def cond(M):
    with np.errstate(all="ignore"):
        return float(np.linalg.cond(np.array(M, np.float64).reshape(6, 6)))


def key_bin(sq):
    k = (np.asarray(sq, np.float64).view(np.uint64) >> np.uint64(44)).astype(np.int64) - (HB_EXP0 << 8)
    return np.clip(k, 0, HB_NB - 1)


def pair_keys(init):
    """All P^2 squared pair distances of a translation-only set, as the kernels add them (x, y, z in order)."""
    x = np.asarray(init, np.float64).T
    with np.errstate(all="ignore"):
        d = x[:, None, :] - x[None, :, :]
        sq = np.zeros(d.shape[:2])
        for k in range(6):
            sq = sq + d[:, :, k] * d[:, :, k]
    return sq


def tinit(xyz):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    init = np.zeros((6, xyz.shape[0]))
    init[:3] = xyz.T
    return init


BENIGN = sums_row(sw=1.0, bt=(0.01, -0.02, 0.015), br=(0.001, 0.002, -0.0015))


def rep(row, P, W=1):
    return np.broadcast_to(np.asarray(row, np.float64), (W, P, 22)).copy()


# ---------------------------------------------------------------- LU and solve
def lu_cases():
    out = []
    S0 = (2.0, 0.5, -0.25, 3.0, 0.125, 4.0)
    bvec = dict(bt=(0.3, -0.2, 0.1), br=(0.05, 0.07, -0.02))
    rows = {
        "lu_k0_sw0": (sums_row(sw=0.0, a=(0.0, 6.0, 8.0), S=S0, **bvec), "swap at k = 0: sw = 0, |a| = 10"),
        "lu_k0_sw1e-3": (sums_row(sw=1e-3, a=(0.0, 6.0, 8.0), S=S0, **bvec), "swap at k = 0: sw = 1e-3, |a| = 10"),
        "lu_multi": (sums_row(sw=0.5, a=(3.0, -2.0, 1.0), S=(0.25, 2.0, 1.5, 0.5, -1.0, 0.125), **bvec), "swaps at two or more k"),
        # (among tie matrices this one is kept because the other pivot order moves N by 42 times the right order's own error:
        #  most ties change the result by a rounding only, and the bar could not tell the orders apart)
        "lu_tie": (sums_row(sw=0.0, a=(0.0, 1.5, 1.5), S=(20.0, 5.0, -2.0, 30.0, 1.0, 40.0), **bvec),
                   "two equal pivot candidates at k = 0, the first wins"),
        "lu_cond1e12": (sums_row(sw=0.0, a=(0.3, -0.2, 0.1), S=(3e5, 1e5, 0.0, 4e5, 2e5, 5e5), **bvec), "condition number about 1e12"),
        "lu_singular": (sums_row(sw=1.0, S=(0.0, 0, 0, -1e-6, 0, 0.0), **bvec), "exactly singular H: N is NaN"),
    }
    for name, (row, regime) in rows.items():
        H = hmat(row)
        piv, tie = F.pivots(H)
        swaps = [k for k, p in enumerate(piv) if p is not None and p != k]
        if name.startswith("lu_k0"):
            assert piv[0] in (4, 5) and abs(H[0]) < 1.1e-3, (name, piv)
        if name == "lu_multi":
            assert len(swaps) >= 2, (name, piv)
        if name == "lu_tie":
            assert tie and piv[0] == 4 and abs(H[24]) == abs(H[30]) > abs(H[0]), (name, piv)
        if name == "lu_cond1e12":
            assert 1e11 < cond(H) < 1e13, cond(H)
        if name == "lu_singular":
            assert None in piv and all(v == 0.0 for v in H[18:24]), (name, piv)
        out.append(Case(name + "_p1", np.zeros((6, 1)), rep(row, 1), regime=regime, tags=("lu",), info=dict(piv=piv)))
        init3 = tinit([[0, 0, 0], [1, 0, 0], [0, 2, 0]])
        c = Case(name + "_p3d", init3, rep(row, 3), regime=regime + "; mean Hessian (inverse_column)", exact_h=True, tags=("lu",))
        if name not in ("lu_singular",):
            pm, _ = F.pivots([float(v) for v in c.step()["aux"]["Hmean"]])
            assert [k for k, p in enumerate(pm) if p != k], (name, pm)
        out.append(c)
        if name in ("lu_k0_sw0", "lu_multi", "lu_tie"):
            c = Case(name + "_p3f", init3, rep(row, 3), full=True, lr=0.75, regime=regime + "; Hm of the full branch", exact_h=True,
                     tags=("lu",))
            for Hm in c.step()["aux"]["Hm"]:
                pm, _ = F.pivots([float(v) for v in Hm])
                assert [k for k, p in enumerate(pm) if p != k], (name, pm)
            out.append(c)
    return out


# ---------------------------------------------------------------- Exp, left Jacobian, Log
def exp_cases():
    out = []
    D = 1.0 + 1e-6                                   # H = D I for the benign S: N = b / D
    u = np.array([2.0, 3.0, 6.0]) / 7.0
    targets = {                                      # wanted rotation step phi_r, regime, bounds on |phi_r|
        "exp_zero": (np.zeros(3), "phi_r exactly zero: NaN translation, zero rotation", (0.0, 0.0)),
        "exp_1e-13": (1e-13 * u, "|phi_r| = 1e-13, below the 1e-12 axis guard", (0.9e-13, 1.1e-13)),
        "exp_1e-9": (1e-9 * u, "|phi_r| = 1e-9: 1 - cos cancels", (0.9e-9, 1.1e-9)),
        "exp_1e-3": (1e-3 * u, "|phi_r| = 1e-3", (0.9e-3, 1.1e-3)),
        "exp_pi-1e-4": ((PI - 1e-4) * u, "|phi_r| = pi - 1e-4", (PI - 1.1e-4, PI - 0.9e-4)),
        "exp_pi-1e-6": ((PI - 1e-6) * u, "|phi_r| = pi - 1e-6: Log loses 2e-4 of 1 + cos", (PI - 1.1e-6, PI - 0.9e-6)),
        "exp_pi": (np.array([0.0, 0.0, PI]), "|phi_r| within an ulp of pi about z: |sin| <= 1e-12, Log returns zeros", (PI - 1e-15, PI + 1e-15)),
    }
    far = tinit([[0, 0, 0], [2.0 ** 100, 0, 0], [0, 2.0 ** 101, 0]])   # phi_i = -N_i to rounding: the repulsion is 2^-100
    for name, (pr, regime, (lo, hi)) in targets.items():
        row = sums_row(bt=tuple(-D * np.array([0.1, 0.2, 0.3])), br=tuple(-D * pr))
        for suffix, init in (("_p1", np.zeros((6, 1))), ("_p3", far)):
            c = Case(name + suffix, init, rep(row, init.shape[1]), regime=regime, tags=("exp",), exact_h=suffix == "_p3",
                     well=name in ("exp_zero", "exp_1e-13", "exp_1e-3", "exp_pi"))   # the others are the cancellation regimes of Exp and Log
            o = c.step()
            for p in range(c.P):
                n = float(np.linalg.norm(o["phi"][p, 3:]))
                assert lo <= n <= hi, (c.name, n)
            if name == "exp_zero":
                assert np.isnan(o["pose"][:3]).all() and (o["pose"][3:] == 0).all(), c.name
            if name == "exp_pi":
                assert (o["pose"][3:] == 0).all() and np.isfinite(o["pose"]).all(), c.name
            out.append(c)
    # the clamp of Log: an initial rotation and a step whose product has 0.5 (trace - 1) outside [-1, 1] by rounding
    found = {}
    for k in range(1, 4000):
        if len(found) == 2:
            break
        for kind, r0, pr in (("above", np.array([0.0, 0.0, 1e-3 * k]), np.array([0.0, 0.0, -1e-3 * k])),
                             ("below", np.array([0.0, 0.0, PI * k / 4001]), np.array([0.0, 0.0, PI - PI * k / 4001]))):
            if kind in found:
                continue
            with np.errstate(all="ignore"):
                R0m, _ = ref.so3_exp(F, [np.float64(v) for v in r0])
            init = np.zeros((6, 1)); init[3:, 0] = r0
            # b_r is the vee part of Rc^T C: C = Rc G with G's vee part -D pr gives N_r = -pr up to rounding
            G = np.zeros((3, 3)); G[2, 1], G[0, 2], G[1, 0] = -D * pr
            row = sums_row(); row[13:22] = (np.array(R0m, np.float64).reshape(3, 3) @ G).reshape(9)
            c = Case("log_clamp_" + kind, init, rep(row, 1), regime="0.5 (trace - 1) %s by rounding: the clamp acts" %
                     ("> 1" if kind == "above" else "< -1"), tags=("exp",), well=True)
            o = c.step()
            with np.errstate(all="ignore"):
                dR, _ = ref.so3_exp(F, [np.float64(v) for v in o["phi"][0, 3:]])
                Rn = ref.mat3_mul(R0m, dR)
                craw = 0.5 * (Rn[0] + Rn[4] + Rn[8] - 1)
            if (kind == "above" and craw > 1) or (kind == "below" and craw < -1):
                c.info = dict(craw=float(craw))
                found[kind] = c
    assert len(found) == 2, sorted(found)
    return out + [found["above"], found["below"]]


# ---------------------------------------------------------------- median and bandwidth
def lattice(P, d):
    i = np.arange(P)
    return tinit(np.stack([i % 4, (i // 4) % 4, i // 16], 1) * d)


def clusters(sizes, centres, step):
    pts = []
    for n, c in zip(sizes, centres):
        for k in range(n):
            pts.append([c[0], c[1], k * step])
    return tinit(pts)


def median_cases():
    out = []

    def add(name, init, regime, full=False, lr=1.0, check=None, sums=None):
        P = init.shape[1]
        c = Case(name, init, rep(BENIGN, P) if sums is None else sums, full=full, lr=lr, regime=regime, exact_h=True, tags=("median",),
                 well=not name.startswith("med_lo"))   # h = 2e-16: the repulsion 2 / h sum (x_i - x_j) k_ij cancels
        sq = pair_keys(init)
        with np.errstate(all="ignore"):
            srt = np.sort(sq.reshape(-1))
        n = P * P
        nan = bool(np.isnan(sq).any())                   # torch::median propagates NaN
        c.info = dict(lower=np.nan if nan else float(srt[(n - 1) // 2]), upper=np.nan if nan else float(srt[n // 2]), sq=sq)
        if check:
            check(c, sq, srt)
        out.append(c)
        return c

    def exact(c, sq, srt):                            # every key exact: the same in any order of the three squares
        x = c.init[:3].T
        d = x[:, None, :] - x[None, :, :]
        assert np.array_equal(sq, d[:, :, 2] ** 2 + d[:, :, 1] ** 2 + d[:, :, 0] ** 2), c.name

    def zero_median(c, sq, srt):
        exact(c, sq, srt); assert c.info["lower"] == 0.0, c.name

    def smallest_positive(c, sq, srt):
        exact(c, sq, srt); assert c.info["lower"] == srt[srt > 0].min(), c.name

    def duplicates(c, sq, srt):
        exact(c, sq, srt); assert (srt == c.info["lower"]).sum() > 2 and c.info["lower"] > 0, c.name

    add("med_p2", tinit([[0, 0, 0], [0.5, 0, 0]]), "P = 2: the lower median is one of the diagonal's zeros, h = 0", check=zero_median)
    add("med_p3", tinit([[0, 0, 0], [0.5, 0, 0], [0, 2, 0]]), "P = 3: the median is the smallest positive key", check=smallest_positive)
    add("med_p4", tinit([[0, 0, 0], [0.5, 0, 0], [0, 2, 0], [0, 0, 4]]), "P = 4, even rank", full=True, lr=0.5, check=exact)
    add("med_p5", lattice(5, 0.25), "P = 5, a key with exact duplicates", check=duplicates)
    for P in (64, 65, 127, 128, 129, 130, 182):
        add("med_p%d" % P, lattice(P, 0.125), "lattice of %d, spacing 2^-3: duplicates; %s" %
            (P, "one workgroup" if P <= 128 else "histogram chain; fused: keys through work.sq" if P >= 182 else "histogram chain"),
            full=(P == 65), lr=0.5, check=duplicates)
    for P in (128, 129):
        def hi(c, sq, srt):
            exact(c, sq, srt)
            assert (key_bin(sq[sq > 0]) == HB_NB - 1).all() and key_bin(c.info["lower"]) == HB_NB - 1, c.name
            m = int((sq > 0).sum())
            assert m // 2 > FRONT_BUF and (P <= 128 or m > SEL_LDS_KEYS), c.name

        def lo(c, sq, srt):
            exact(c, sq, srt)
            assert (key_bin(sq) == 0).all() and 0 < c.info["lower"] < 2.0 ** -40, c.name
            assert (P * P - P) // 2 > FRONT_BUF and (P <= 128 or P * P > SEL_LDS_KEYS), c.name
        add("med_hi_p%d" % P, tinit(np.stack([np.arange(P) * 16.0, np.zeros(P), np.zeros(P)], 1)),
            "every nonzero key >= 2^8: the last bin holds them all (front buffer overflows / select on the global buffer)", check=hi)
        add("med_lo_p%d" % P, tinit(np.stack([np.arange(P) * 2.0 ** -30, np.zeros(P), np.zeros(P)], 1)),
            "every key < 2^-40: bin 0 holds them all, with the zeros (a converged set)", check=lo)
    tri = [(0.0, 0.0), (1031.0 / 256, 0.0), (515.5 / 256, 893.0 / 256)]
    for sizes, want in (((32, 32, 16), FRONT_BUF), ((1, 40, 49), FRONT_BUF + 1)):
        def fb(c, sq, srt, want=want):
            exact(c, sq, srt)
            b = key_bin(sq)
            bstar = key_bin(c.info["lower"])
            iu = np.triu_indices(c.P, 1)
            assert int((b[iu] == bstar).sum()) == want and 0 < bstar < HB_NB - 1, (c.name, int((b[iu] == bstar).sum()))
        add("med_fb%d" % want, clusters(sizes, tri, 2.0 ** -10), "the median's bin holds exactly %d pair keys (FRONT_BUF = 2048)" % want, check=fb)

    def nan_h(c, sq, srt):
        assert np.isnan(c.step()["h"]), c.name
    bad = lattice(5, 0.25); bad[1, 3] = np.nan
    add("med_nan_p5", bad, "a NaN pose entry: h is NaN", check=nan_h)
    bad = lattice(130, 0.125); bad[0, 77] = np.inf
    add("med_inf_entry_p130", bad, "an infinite pose entry: inf - inf on the diagonal, h is NaN", check=nan_h)

    def inf_med(c, sq, srt):
        assert c.info["lower"] == np.inf and np.isinf(c.step()["h"]), c.name
    add("med_inf_p3", tinit([[0, 0, 0], [2.0 ** 515, 0, 0], [-2.0 ** 515, 0, 0]]),
        "particles 2^515 (about 1e155) apart: the squared distance overflows, the lower median is +inf", check=inf_med)
    big = lattice(130, 0.125); big[0, 44:87] += 2.0 ** 515; big[0, 87:] -= 2.0 ** 515
    add("med_inf_p130", big, "three groups 2^515 apart, P = 130: the lower median is +inf", check=inf_med)
    return out


# ---------------------------------------------------------------- the three directions
def direction_cases():
    out = []
    for P in (2, 5, 64, 65, 128, 130):
        p = np.arange(P)
        site = p // 2                                           # coincident pairs: kernel value exactly 1
        init = np.zeros((6, P))
        init[0] = site * 1.0
        init[1] = 0.25 * (site % 3)
        init[3] = 0.1 * ((site % 5) - 2); init[4] = 0.05 * ((site % 3) - 1); init[5] = 0.02 * (site % 7)
        if P == 2:                                              # two particles: the median of {0, 0, d, d} is 0, h = 0, the step is NaN
            init[0] = (0.0, 1.0)
            for mode, full in (("svn", False), ("svn", True), ("svgd", False)):
                c = Case("dir_%s_p2" % ("svgd" if mode == "svgd" else "full" if full else "default"), init, rep(BENIGN, 2), full=full,
                         lr=0.75 if full else 0.01 if mode == "svgd" else 1.0, mode=mode, optimizer="SGD", tags=("dir",),
                         regime="P = 2: the lower median is a diagonal zero, h = 0 and the whole step is NaN, as in the reference")
                o = c.step()
                assert o["h"] == 0 and np.isnan(o["phi"]).all() and np.isnan(o["pose"][:3]).all(), c.name
                out.append(c)
            continue
        init[0, P - 1] = 8192.0                                 # one far particle: its kernel values underflow to 0, ks = 1
        if P > 5:
            init[0, P - 2] = 4096.0
        sums = np.zeros((1, P, 22))
        for q in range(P):
            sums[0, q] = sums_row(sw=1.0 + 0.125 * (q % 4), a=(0.05 * (q % 3), -0.04 * (q % 5), 0.03 * (q % 2)),
                                  S=(0.5 + 0.01 * (q % 6), 0.02, -0.01, 0.6, 0.015, 0.55 + 0.02 * (q % 3)),
                                  bt=(0.01 * ((q % 7) - 3), 0.02 * ((q % 5) - 2), 0.015 * ((q % 3) - 1)),
                                  br=(0.001 * ((q % 4) - 1.5), 0.002 * ((q % 6) - 2.5), -0.0015 * ((q % 5) - 2)))
        for full in (False, True):
            c = Case("dir_%s_p%d" % ("full" if full else "default", P), init, sums, full=full, lr=0.75 if full else 1.0, well=True,
                     regime="coincident pairs (k = 1), far particles (k = 0, ks = 1)", tags=("dir",))
            x = init.T.copy()
            with np.errstate(all="ignore"):
                R = [ref.so3_log(F, ref.so3_exp(F, [np.float64(v) for v in init[3:, q]])[0]) for q in range(P)]
            x[:, 3:] = np.array(R, np.float64)
            d = x[:, None, :] - x[None, :, :]
            sq = (d * d).sum(2)
            med = np.sort(sq.reshape(-1))[(P * P - 1) // 2]
            h = med / np.log(P + 1.0)
            K = np.exp(-sq / h)
            off = ~np.eye(P, dtype=bool)
            assert med > 0 and (K[off] == 1.0).any() and (K[P - 1][:P - 1] == 0.0).all() and K[P - 1].sum() == 1.0, c.name
            Hs = np.array([hmat(sums[0, q]) for q in range(P)]).reshape(P, 6, 6)
            assert max(np.linalg.cond(Hs[q]) for q in range(P)) < 1e4, c.name
            # a finite step (numpy, vectorised: the float64 step in Python takes seconds at 128 particles): every matrix that is
            # inverted is far from singular and every sum is finite
            g = 2 / h * d * K[:, :, None]
            if full:
                Hm = (np.einsum("ij,jrc->irc", K * K, Hs) + np.einsum("ijr,ijc->irc", g, g)) / P
                assert np.isfinite(Hm).all() and max(np.linalg.cond(Hm[q]) for q in range(P)) < 1e8, c.name
            else:
                assert np.linalg.cond(Hs.mean(0)) < 1e4 and (K.sum(1) >= 1.0).all() and np.isfinite(g.sum(1)).all(), c.name
            out.append(c)
        c = Case("dir_svgd_p%d" % P, init, sums, lr=0.01, mode="svgd", optimizer="SGD", well=True, tags=("dir", "svgd"),
                 regime="SVGD-ICP direction: coincident pairs (k = 1), far particles (k = 0)")
        d = init.T[:, None, :] - init.T[None, :, :]
        sq = (d * d).sum(2)
        med = np.sort(sq.reshape(-1))[(P * P - 1) // 2]
        K = np.exp(-sq / (med / np.log(P + 1.0)))
        assert med > 0 and (K[~np.eye(P, dtype=bool)] == 1.0).any() and (K[P - 1][:P - 1] == 0.0).all(), c.name
        out.append(c)
    return out


# ---------------------------------------------------------------- SVGD-ICP: gradient and optimizers
def svgd_cases():
    out = []
    pose1 = np.array([[0.1], [0.2], [0.3], [0.01], [0.02], [0.03]])
    Cm = (0.3, -0.2, 0.1, 0.05, 0.4, -0.25, 0.15, -0.35, 0.2)

    def row(count, es, C=Cm):
        s = np.zeros(22)
        s[4], s[10:13], s[13:22] = count, es, C
        return s
    # svgd_gradient: the (count + 1) normalisation and the Euler partials
    for name, count, pose, regime, well in (
            ("svgd_grad_count0", 0.0, pose1, "count + 1 = 1", True),
            ("svgd_grad_count1e6", 1e6, pose1, "a large count", True),
            ("svgd_grad_pitch", 37.0, np.array([[0.1], [0.2], [0.3], [0.4], [PI / 2 - 0.75e-9], [-0.7]]), "pitch within 1e-9 of pi / 2", False)):
        for P in (1, 5):
            init = np.repeat(pose, P, 1)
            init[0] += np.arange(P) * 0.5
            c = Case("%s_p%d" % (name, P), init, rep(row(count, (0.3, -0.2, 0.1)), P), lr=0.01, mode="svgd", optimizer="SGD",
                     regime=regime, tags=("svgd",),
                     well=well and not (P > 1 and count > 1))   # (the gradient shrinks by 1e6 and the middle particle's repulsion sum cancels against nothing)
            o = c.step()
            assert np.isfinite(o["N"]).all() and np.abs(o["N"]).min() > 0, c.name
            if name == "svgd_grad_pitch":
                assert abs(abs(init[4, 0]) - PI / 2) <= 1e-9 and abs(np.cos(init[4, 0])) < 2e-9, c.name
            out.append(c)
    # the four optimizers, one step from zero state: g = 1e-12, 1e-6 ... per parameter; with count = 0 the translation gradient
    # is es * N_SRC exactly, and C = 0 makes the rotation gradient exactly 0
    for opt in ref.OPTIMIZERS:
        c = Case("opt_%s_p1" % opt.lower(), pose1.copy(), rep(row(0.0, (0.0, 1e-12 / N_SRC, 1.0 / N_SRC), C=(0.0,) * 9), 1), lr=0.02,
                 mode="svgd", optimizer=opt, regime="one step from zero state with g = 0, 1e-12 and 1", well=True, tags=("svgd", "opt"))
        o = c.step()
        assert np.array_equal(o["N"][0], [0.0, 1e-12, 1.0, 0.0, 0.0, 0.0]), (c.name, o["N"])
        if opt != "RMSprop":     # (its weight decay moves a parameter whose gradient is zero)
            assert np.array_equal(o["pose"][[0, 3, 4, 5], 0], pose1[[0, 3, 4, 5], 0]), c.name
        out.append(c)
    # three consecutive updates on one context: bias correction and the moment buffers
    for opt in ref.OPTIMIZERS:
        c = Case("seq3_%s_p1" % opt.lower(), pose1.copy(), rep(row(3.0, (0.03, -0.02, 0.01)), 1), lr=0.02, mode="svgd", optimizer=opt, steps=3,
                 regime="three consecutive updates", well=True, tags=("svgd", "seq"))
        out.append(c)
    for P in (5, 130):
        init = np.repeat(pose1, P, 1)
        init[0] += np.arange(P) * 0.125
        init[4] += 0.01 * (np.arange(P) % 5)
        c = Case("seq3_adam_p%d" % P, init, rep(row(3.0, (0.03, -0.02, 0.01)), P), lr=0.02, mode="svgd", optimizer="Adam", steps=3,
                 regime="three consecutive updates, %s" % ("one workgroup and chain with svgd = 1" if P <= 128 else "P > 128"), tags=("svgd", "seq"))
        out.append(c)
    return out


# ---------------------------------------------------------------- early stop in float32
def early_stop_cases():
    out = []
    t = 2.0 ** -10                                              # a float32 threshold
    D = 1.0 + 1e-6
    for P in (1, 5, 130):
        init = np.zeros((6, P)) if P == 1 else tinit(np.stack([np.arange(P) * 2.0 ** 100, np.zeros(P), np.zeros(P)], 1))
        for kind, m in (("go", t * (1 - 2.0 ** -27)), ("stop", t * (1 - 2.0 ** -23))):
            row = sums_row(bt=(0.0, 0.0, 0.0), br=(0.0, 0.0, -D * m))   # phi = (0, 0, 0, 0, 0, m) to rounding
            c = Case("es_%s_p%d" % (kind, P), init, rep(row, P), es=True, thr=t, well=True, exact_h=P > 1, tags=("es",),
                     regime="mean step norm t (1 - 2^-%d): %s" % (27 if kind == "go" else 23, "rounds up to t in float32, no stop" if kind == "go" else "stops"))
            o = c.step()
            assert o["stop"] == (kind == "stop"), c.name
            mean = float(o["aux"]["mean"])
            assert (mean < t) and (np.float32(mean) < np.float32(t)) == (kind == "stop"), c.name   # the float64 compare would stop both
            out.append(c)
    return out


# ---------------------------------------------------------------- row shards
def shard_cases():
    out = []
    base = sums_row(sw=1.0, a=(0.3, -0.2, 0.1), S=(2.0, 0.5, -0.25, 3.0, 0.125, 4.0), bt=(0.3, -0.2, 0.1), br=(0.05, 0.07, -0.02))
    for P, init in ((1, np.zeros((6, 1))), (3, tinit([[0, 0, 0], [1, 0, 0], [0, 2, 0]]))):
        sums = np.zeros((3, P, 22))
        for p in range(P):
            sums[0, p] = base * (0.7531 + 0.1 * p)
            sums[1, p] = base * (3.337 + 0.017 * np.arange(22)) * (1 + p)
            sums[2, p] = -base * (1.913 + 0.023 * np.arange(22)) * (1 + p)
        c = Case("shard_w3_p%d" % P, init, sums, regime="W = 3 records whose sum depends on the order in the last bits", tags=("shard",),
                 exact_h=P > 1)
        ltr, rev = ref.reduce_sums(sums), ref.reduce_sums(sums, reverse=True)
        other = (sums[0] + sums[2]) + sums[1]
        assert not np.array_equal(ltr, rev) and not np.array_equal(ltr, other), c.name
        out.append(c)
    return out


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = lu_cases() + exp_cases() + median_cases() + direction_cases() + svgd_cases() + early_stop_cases() + shard_cases()
        names = [c.name for c in _CASES]
        assert len(set(names)) == len(names)
    return _CASES


def compared_particles(P):
    """Particles whose outputs the fixture keeps (all up to 16; beyond, the wavefront and workgroup edges and every 8th)."""
    if P <= 16:
        return np.arange(P)
    keep = set(range(0, P, 8)) | {1, 2, 3, 31, 32, 62, 63, 64, 65, 126, 127, 128, 129, P - 2, P - 1}
    return np.array(sorted(i for i in keep if 0 <= i < P))
