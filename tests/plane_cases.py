"""Hand-built inputs of the plane residual's kernels one by one (test infrastructure; tests/test_plane_alone_{cpu,gpu}.py).

NORMAL CASES feed k_target_normals through svnicp_align_begin (residual = plane, no supplied normals).  A target is a union
of isolated clusters of exactly normal_k points, at least 50 cluster diameters apart, so that every member's normal_k
nearest targets are its own cluster (the CPU test asserts it with the oracle's knn_topk): the neighbourhood of a row is known
without a search, and its scatter matrix is an exact rational function of the coordinates (plane_mp_reference.exact_scatter).
Clusters come from +-1 sign patterns (three orthogonal, zero-sum columns), scaled per column to the eigenvalues a kind asks
for and turned by a fixed generic rotation; the exact kinds keep dyadic coordinates on the axes, so that the scatter matrix
is exactly diagonal.  Every kind is placed near the origin and again shifted by SHIFT (whole metres: dyadic offsets stay
exact).  Whatever rounding does to a coordinate, the judged matrix is that of the stored coordinates.

ACCUMULATE CASES are what tests/test_plane_alone_gpu.py hands k_plane_accumulate / k_plane_finalize through the split-phase
ABI, as tests/stage_b_cases.py does for stage B: src, tgt, supplied normals, a candidate table cand [B][K], total poses
[P][12], max_dist, delta.  Every candidate index lies in [0, M).  Options: chain=general and accum_min_steps=1 (one wave pass
per workgroup: the second half of every U = 2 trip lies past the block), except the `trips` cases, which ask for 3 and 4
passes per workgroup so that second trips and prefetches past the first run too.  Winners are decided by a wide margin
(asserted); ties belong to stage B's tests.
"""
import zlib

import numpy as np

import plane_mp_reference as pm
import plane_reference as pr
import stage_b_cases as sc
import stage_b_reference as sb

SHIFT = np.array([4.3e6, -8.8e6, 5e4])
KN = (4, 8, 12, 16, 64)
IDENT = sc.IDENT
SPACING = 512.0           # lattice of the unit-extent clusters: their diameter stays below 6
MARGIN = 1e-7             # every cluster's l1 / l2 stays this far (relative) from MIN_RATIO


def rng_for(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def generic_rotation(az=1.1, ay=-0.4, ax=0.7):
    """Rz(az) Ry(ay) Rx(ax): no entry near 0 or 1, no axis kept."""
    cz, sz, cy, sy, cx, sx = np.cos(az), np.sin(az), np.cos(ay), np.sin(ay), np.cos(ax), np.sin(ax)
    q = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]]) @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    assert 0.05 < np.abs(q).min() and np.abs(q).max() < 0.95, "generic"
    return q


ROT = generic_rotation()


# ------------------------------------------------------------------------------------------------ normals
class Cluster:
    def __init__(self, kind, placement, pts, declared=None, axis=None, judged=True):
        self.kind, self.placement, self.pts = kind, placement, np.asarray(pts, np.float64)
        self.declared, self.axis, self.judged = declared, axis, judged     # declared validity (None: from the eigenvalues)
        self.rows = None


class NormalCase:
    def __init__(self, name, kn, clusters):
        self.name, self.kn, self.clusters = name, kn, clusters
        rng = rng_for(name)
        pts = np.concatenate([c.pts for c in clusters])
        perm = rng.permutation(len(pts))                       # rows of a cluster are scattered over the cloud
        self.tgt = np.ascontiguousarray(pts[perm])
        inv = np.argsort(perm)
        at = 0
        for c in clusters:
            c.rows = inv[at:at + len(c.pts)]
            at += len(c.pts)
            assert np.array_equal(self.tgt[c.rows], c.pts)
        self.M = len(pts)
        self.src = 0.5 * np.arange(24, dtype=np.float64).reshape(8, 3)   # the registration needs a source cloud; nothing reads it

    def checksum(self):
        return np.int64(zlib.crc32(self.tgt.tobytes() + repr((self.kn, [(c.kind, c.placement, c.rows.tolist()) for c in self.clusters])).encode()))

    def kinds(self):
        return sorted({c.kind for c in self.clusters})


def pattern(kn):
    assert kn % 4 == 0
    return np.tile(np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64), (kn // 4, 1))


def spectrum_points(rng, kn, lam, rot=ROT, scale=1.0):
    """kn points whose scatter matrix is rot diag(lam) rot^T up to rounding: sign patterns, blocks of four at amplitudes
    f_g with sum f_g^2 = kn / 4 (more than four distinct points from kn = 8 on)."""
    f = rng.uniform(0.6, 1.4, kn // 4)
    f *= np.sqrt((kn / 4) / (f * f).sum())
    X = pattern(kn) * np.repeat(f, 4)[:, None] * np.sqrt(np.asarray(lam, np.float64) / kn)[None, :]
    return scale * (X @ rot.T)


def axis_points(kn, a):
    """Dyadic, mirror-symmetric: scatter matrix exactly diag(kn a^2)."""
    return pattern(kn) * np.asarray(a, np.float64)[None, :]


def unit_kinds(kn, rng):
    """[(kind, points about 0, declared validity, axis)] of the unit-extent kinds of one normal_k."""
    out = []
    if kn & (kn - 1) == 0:
        a1 = 2.0 ** -int(np.ceil(np.log2(kn) / 2))
        for kind, a, valid, axis in (("exact_planar_z", (1, 0.5, 0), True, 2), ("exact_planar_y", (0.5, 0, 1), True, 1), ("exact_planar_x", (0, 1, 0.5), True, 0),
                                     ("exact_collinear", (0, 1, 0), False, None), ("exact_coincident", (0, 0, 0), False, None), ("exact_cube", (1, 1, 1), True, -1),
                                     ("exact_at_ratio", (10 * a1, 0, a1), True, 1)):
            out.append((kind, axis_points(kn, a), valid, axis))
        l1, l2 = kn * a1 * a1, kn * 100 * a1 * a1
        assert pr.MIN_RATIO * l2 == l1, "l1 == fl(0.01 l2): valid under '>=', not under '>'"
    for kind, lam in (("threshold_above", (1e-4, pr.MIN_RATIO * (1 + 1e-6), 1.0)), ("threshold_below", (1e-4, pr.MIN_RATIO * (1 - 1e-6), 1.0)),
                      ("disc", (0.05, 1.0, 1.0 + 1e-9)), ("needle_gap_1e-3", (0.04, 0.04 * (1 + 1e-3), 1.0)), ("needle_gap_1e-6", (0.04, 0.04 * (1 + 1e-6), 1.0)),
                      ("needle_gap_1e-9", (0.04, 0.04 * (1 + 1e-9), 1.0)), ("needle_gap_0", (0.04, 0.04, 1.0))):
        out.append((kind, spectrum_points(rng, kn, lam), None, None))
    Ct = np.array([[1.0, 0.6, 0.3], [0.6, 1.0, -0.4], [0.3, -0.4, 1.0]])       # equal diagonal, large off-diagonals: first rotations at 45 degrees
    lam, V = np.linalg.eigh(Ct)
    out.append(("equal_diagonal", spectrum_points(rng, kn, lam, rot=V), None, None))
    flat = np.concatenate([rng.uniform(-1, 1, (kn, 2)), 1e-9 * rng.uniform(-1, 1, (kn, 1))], 1)
    out.append(("plane_noise_1e-9", flat @ ROT.T, None, None))
    v = ROT @ np.array([0.7, 0.0, 0.0])
    out.append(("two_points", np.tile(np.stack([v, -v]), (kn // 2, 1)), None, None))
    return out


def normal_case(kn):
    name = "normals_kn%d" % kn
    rng = rng_for(name)
    cl = []
    for placement, off in (("origin", np.zeros(3)), ("shifted", SHIFT)):
        for i, (kind, pts, valid, axis) in enumerate(unit_kinds(kn, rng)):
            centre = SPACING * np.array([i % 3, (i // 3) % 3, i // 9], np.float64) + off
            cl.append(Cluster(kind, placement, pts + centre, valid, axis))
    return NormalCase(name, kn, cl)


def magnitude_case():
    """Extents of 1e-6 m, 1e3 m and 1e-170 m, and a point at 1e20 m (kn = 8).  The 1e-170 cluster sits at the exact origin: its
    squares underflow, the scatter matrix is 0 in float64, there is no normal.  The point at 1e20 is one target more beside
    a full cluster: its 8 nearest targets are all farther than 2^64, so it has no normal, and it is no other row's
    neighbour (a cluster of 8 WITH such a member would borrow a foreign 8th neighbour for its other 7 rows)."""
    kn, name = 8, "normals_magnitudes"
    rng = rng_for(name)
    plate, needle = (0.02, 0.3, 1.0), (0.04, 0.04 * (1 + 1e-6), 1.0)
    cl = [Cluster("extent_1e-170", "origin", spectrum_points(rng, kn, plate, scale=1e-170), declared=False)]
    for placement, off in (("origin", np.zeros(3)), ("shifted", SHIFT)):
        for lam, c6, c3 in ((plate, (1.0, 0, 0), (2.0 ** 19, 0, 0)), (needle, (0, 1.0, 0), (0, 2.0 ** 19, 0))):
            cl.append(Cluster("extent_1e-6", placement, spectrum_points(rng, kn, lam, scale=1e-6) + np.array(c6) + off))
            cl.append(Cluster("extent_1e3", placement, spectrum_points(rng, kn, lam, scale=1e3) + np.array(c3) + off))
    cl.append(Cluster("beside_1e20", "origin", spectrum_points(rng, kn, plate) + np.array([0, 0, 4096.0])))
    cl.append(Cluster("point_1e20", "origin", np.array([[1e20, 0.0, 0.0]]), declared=False, judged=False))
    return NormalCase(name, kn, cl)


_NORMAL = None


def normal_cases():
    global _NORMAL
    if _NORMAL is None:
        _NORMAL = [normal_case(kn) for kn in KN] + [magnitude_case()]
    return _NORMAL


def normal_truth(case):
    """Per cluster, in exact rationals and mpmath: dict(C, lam [3] Fractions, valid, gap = (l1 - l0) / l2).  Asserts the
    premises that need them: every cluster whose validity comes from its eigenvalues lies MARGIN away from the threshold."""
    import mpmath
    out = []
    for c in case.clusters:
        C = pm.exact_scatter(c.pts)
        lam = [pm.as_fraction(v) for v in pm.mp_eigenvalues(C)]
        valid = c.declared
        gap = None
        if lam[2] > 0:
            ratio = float(lam[1] / lam[2])
            gap = float((lam[1] - lam[0]) / lam[2])
            if c.declared is None:
                assert abs(ratio / pr.MIN_RATIO - 1.0) >= MARGIN, (case.name, c.kind, ratio)
                valid = ratio >= pr.MIN_RATIO
            elif c.kind.startswith("exact"):
                assert c.declared == (lam[1] >= pm.Fraction(1, 100) * lam[2]) or c.kind == "exact_at_ratio", (case.name, c.kind)
            if c.kind.startswith("threshold"):
                assert 0.5e-6 <= abs(ratio / pr.MIN_RATIO - 1.0) <= 2e-6 and valid == c.kind.endswith("above"), (case.name, c.kind, ratio)
        else:
            assert c.declared is False
        out.append(dict(C=C, lam=lam, valid=bool(valid), gap=gap))
    del mpmath
    return out


def cluster_isolation(case):
    """Smallest (distance to a foreign cluster's point) / (own diameter) over the clusters; the premise is >= 50."""
    worst = np.inf
    cent = np.array([c.pts.mean(0) for c in case.clusters])
    rad = np.array([np.linalg.norm(c.pts - c.pts.mean(0), axis=1).max() for c in case.clusters])
    for i, c in enumerate(case.clusters):
        if not c.judged:
            continue
        d = np.linalg.norm(cent - cent[i], axis=1) - rad
        d[i] = np.inf
        diam = 2 * rad[i]
        if diam > 0:
            worst = min(worst, float(d.min() / diam))
    return worst


# ------------------------------------------------------------------------------------------------ supplied normals
def pack_table():
    """(tgt [M][3], supplied normals [M][3], expected kept rows [M][3] or None where the bar is 2 ulp of the unit row, note [M])."""
    big, tiny, sub = 1e160, 1e-170, 5e-324
    rows = [((3.0, 4.0, 0.0), (0.6, 0.8, 0.0), "3-4-5"), ((1.0, 0.0, 0.0), (1.0, 0.0, 0.0), "unit axis"), ((0.0, -1.0, 0.0), (0.0, -1.0, 0.0), "unit axis"),
            ((0.6, 0.0, 0.8), (0.6, 0.0, 0.8), "already unit"), ((2.0 / 3, -1.0 / 3, 2.0 / 3), (2.0 / 3, -1.0 / 3, 2.0 / 3), "already unit"),
            ((0.0, 0.0, 0.0), None, "zero"), ((np.nan, 0.0, 1.0), None, "nan"), ((0.0, np.inf, 0.0), None, "inf"), ((-np.inf, np.nan, 0.0), None, "inf and nan"),
            ((0.0, 0.0, 1.0), None, "non-finite point"), ((big, 0.0, 0.0), None, "1e160: the squared norm overflows"),
            ((tiny, tiny, 0.0), None, "1e-170: the squared norm underflows"), ((0.0, sub, 0.0), None, "subnormal: the squared norm underflows"),
            ((1e150, 1e150, 0.0), (np.sqrt(0.5), np.sqrt(0.5), 0.0), "1e150: the squared norm is finite"), ((0.0, 1e-150, 0.0), (0.0, 1.0, 0.0), "1e-150: the squared norm is normal")]
    M = len(rows)
    tgt = np.arange(3 * M, dtype=np.float64).reshape(M, 3)
    tgt[9] = (np.nan, 1.0, 2.0)
    nrm = np.array([r[0] for r in rows], np.float64)
    want = np.array([(0.0, 0.0, 0.0) if r[1] is None else r[1] for r in rows], np.float64)
    return tgt, nrm, want, [r[2] for r in rows]


# ------------------------------------------------------------------------------------------------ accumulate
class PlaneCase:
    def __init__(self, name, tags, src, tgt, nrm, cand, poses, max_dist, delta, min_steps=1, grid_x=None, facts=None):
        self.name, self.tags = name, frozenset(tags)
        self.src = np.ascontiguousarray(src, np.float64)
        self.tgt = np.ascontiguousarray(tgt, np.float64)
        self.nrm_supplied = np.ascontiguousarray(nrm, np.float64)
        self.nrm = pr.normalise_supplied(self.nrm_supplied, self.tgt)       # what k_pack_normals keeps
        self.cand = np.ascontiguousarray(cand, np.int32)
        self.poses = np.ascontiguousarray(poses, np.float64)
        self.max_dist, self.delta, self.min_steps, self.grid_x = float(max_dist), float(delta), int(min_steps), grid_x
        self.facts = dict(facts or {})
        self.B, self.K, self.M, self.P = self.src.shape[0], self.cand.shape[1], self.tgt.shape[0], self.poses.shape[0]
        assert self.src.shape == (self.B, 3) and self.tgt.shape == (self.M, 3) and self.nrm.shape == (self.M, 3) and self.poses.shape == (self.P, 12)
        assert self.cand.shape[0] == self.B and 1 <= self.K <= 16 and self.B <= 4112
        assert self.cand.min() >= 0 and self.cand.max() < self.M, "every candidate index lies in [0, M)"
        assert np.isfinite(self.src).all() and np.isfinite(self.tgt).all() and np.isfinite(self.poses).all() and np.isfinite(self.nrm).all()
        assert self.delta > 0
        self._D = None

    def options(self):
        return (("chain", "general"), ("accum_min_steps", str(self.min_steps)))

    def discrete(self, variant=()):
        if variant:
            return pm.discrete(self.src, self.tgt, self.nrm, self.cand, self.poses, self.max_dist, variant)
        if self._D is None:
            self._D = pm.discrete(self.src, self.tgt, self.nrm, self.cand, self.poses, self.max_dist)
        return self._D

    def f64(self, variant=()):
        return pm.sums_f64(self.src, self.tgt, self.nrm, self.cand, self.poses, self.max_dist, self.delta, self.discrete(variant), variant)

    def mp_particles(self):
        return sb.mp_particles(self.P)

    def geometry(self):
        """(PW, WP, points per pass, grid_y, Ppad) of registration_plan.hpp for the split variant, which plane mode keeps at any P."""
        PW, WP = sc.stage_b_shape(self.P)
        gy = -(-self.P // (PW * WP))
        return PW, WP, (64 // PW) * (4 // WP), gy, gy * PW * WP

    def expected_grid(self):
        """{grid_x, grid_y, pts_per_block, Ppad} where one resident round holds every workgroup (plan_accumulate's size_grid)."""
        PW, WP, pp, gy, Ppad = self.geometry()
        steps = -(-self.B // pp)
        g = max(1, steps // self.min_steps) if self.min_steps > 1 else steps
        ppb = -(-steps // g) * pp
        return -(-self.B // ppb), gy, ppb, Ppad

    def checksum(self):
        blob = b"".join(a.tobytes() for a in (self.src, self.tgt, self.nrm_supplied, self.cand, self.poses)) + \
            repr((self.max_dist, self.delta, self.min_steps)).encode()
        return np.int64(zlib.crc32(blob))

    def winner_margin(self):
        """Smallest (second least d2) / (least d2 + 1e-12) over the pairs: the winners are decided by a wide margin."""
        if self.K == 1:
            return np.inf
        Ts = self.discrete()["Ts"]
        q = self.tgt[self.cand]
        dx, dy, dz = (Ts[:, :, None, i] - q[None, :, :, i] for i in range(3))
        d2 = np.sort((dx * dx + dy * dy) + dz * dz, -1)
        return float((d2[..., 1] / (d2[..., 0] + 1e-12)).min())

    def edge_distance(self):
        """(smallest |d2 / max_dist - 1|, smallest ||r| / delta - 1| over the accepted pairs) of the float64 restatement."""
        D = self.discrete()
        with np.errstate(all="ignore"):
            g = np.abs(D["d2"] / self.max_dist - 1.0).min()
            e = D["Ts"] - self.tgt[D["widx"]]
            r = (self.nrm[D["widx"]] * e).sum(-1)[D["ok"]]
            k = np.abs(np.abs(r) / self.delta - 1.0).min() if r.size and np.isfinite(self.delta) else np.inf
        return float(g), float(k)


AXES = np.eye(3)


def exact_case(name, rows, shifts, max_dist, delta, tags=(), K=4):
    """rows: (s, normal, off[, 'zero']) — the winner sits exactly at s - off (e = off at the identity pose) at slot b mod K and
    carries `normal`; the other slots are 50 away.  'zero': the winner has no normal and the next slot holds s - off - 1.5 WITH
    the normal (a farther candidate that must not be taken instead).  Particle p is the identity translated by shifts[p]."""
    B = len(rows)
    src = np.array([r[0] for r in rows], np.float64)
    tgt = np.zeros((B * K, 3))
    nrm = np.tile(AXES[2], (B * K, 1))
    cand = np.arange(B * K, dtype=np.int32).reshape(B, K)
    for b, r in enumerate(rows):
        s, n, off = (np.asarray(x, np.float64) for x in r[:3])
        for k in range(K):
            tgt[cand[b, k]] = s + 50.0 + np.array([k, 2.0 * k, b % 5])
        tgt[cand[b, b % K]] = s - off
        nrm[cand[b, b % K]] = n
        if len(r) > 3:
            nrm[cand[b, b % K]] = 0.0
            tgt[cand[b, (b + 1) % K]] = s - off - 1.5
            nrm[cand[b, (b + 1) % K]] = n
    poses = np.tile(IDENT, (len(shifts), 1))
    poses[:, 9:] = np.asarray(shifts, np.float64)
    return PlaneCase(name, set(tags) | {"exact"}, src, tgt, nrm, cand, poses, max_dist, delta)


def exact_cases():
    out = []
    P = 12
    yz = [(0.0, 0.25 * (p % 3), 0.5 * (p // 3)) for p in range(P)]          # orthogonal to the x normals: r does not change
    rng = rng_for("exact")
    S = rng.integers(-4, 5, (16, 3)).astype(np.float64)
    far = (3.0, 3.0, 3.0)
    ex = AXES[0]
    d = 0.25
    rows = [(S[0], ex, (d, 0.5, 0.0)), (S[1], ex, (-d, 0.0, 0.5)), (S[2], ex, (d, -0.5, -0.25)), (S[3], ex, (-d, 0.25, 0.25)),     # |r| == delta: w = 1
            (S[4], ex, (0.0, 0.5, 0.5)), (S[5], ex, (0.0, 0.0, 0.0)),                                                             # r == 0
            (S[6], ex, (0.125, 0.0, 0.0)), (S[7], ex, (-0.125, 0.5, 0.0)), (S[8], ex, (0.125, 0.25, 0.0), "zero"), (S[9], ex, far),
            (S[10], -ex, (d, 0.0, 0.0)), (S[11], ex, (d, 0.0, 0.25), "zero")]
    c = exact_case("huber_at_delta", rows, yz, 16.0, d, tags=("huber",))
    D = c.discrete()
    e = D["Ts"] - c.tgt[D["widx"]]
    r = (c.nrm[D["widx"]] * e).sum(-1)
    assert (np.abs(r[D["ok"]]) == d).sum() >= 5 * P and (r[D["ok"]] == 0).sum() >= 2 * P and (np.abs(r[D["ok"]]) <= d).all()
    assert not D["ok"][:, [8, 9, 11]].any() and D["mask"][:, [8, 11]].all(), "a winner without a normal is rejected inside the gate"
    assert D["ok"].sum(1).tolist() == [9] * P
    out.append(c)
    up = np.nextafter(d, np.inf)
    rows = [((0.0, 2.0, 0.0), ex, (up, 0.0, 0.0)), ((0.0, 0.0, -4.0), ex, (-up, 0.0, 0.0)), (S[0], ex, far), (S[1], ex, far), (S[2], ex, far)]
    c = exact_case("huber_above_delta", rows, yz, 4.0, d, tags=("huber",))
    D = c.discrete()
    assert D["ok"].sum(1).tolist() == [2] * P
    # H00 = 2 w + 1e-6 with w the correctly rounded delta / |r|: one below 1, and not what '|r| <= delta' -> 1 would give
    w = d / up
    assert w == 1.0 - 2.0 ** -52 and c.f64()[0][0, 0] == 2.0 * w + pr.DAMPING and 2.0 * w + pr.DAMPING != 2.0 + pr.DAMPING
    out.append(c)
    half = [(0.5, 0.5, 0.5), (-0.5, 0.5, -0.5), (0.5, -0.5, 0.0), (0.5, 0.5, 0.75), (0.0, 0.0, 0.0), (-0.5, -0.5, 0.5), (0.25, 0.5, 0.5)] * 2
    xs = [(0.25 * (p % 3), 0.25 * (p // 3), 0.0) for p in range(P)]         # multiples of 0.25: every d2 is exact
    for nm, md in (("gate_at_max_dist", 0.75), ("gate_below_max_dist", float(np.nextafter(0.75, 1.0)))):
        rows = [(S[b], AXES[b % 3] * (1 if b % 2 else -1), off) for b, off in enumerate(half)]
        c = exact_case(nm, rows, xs, md, np.inf, tags=("gate", "delta_inf"))
        D = c.discrete()
        at = D["d2"] == 0.75
        assert at.sum() >= 8 and (D["ok"][at] == (md > 0.75)).all(), "d2 == max_dist is rejected, max_dist one ulp above it accepts"
        assert (c.discrete(("gate_le",))["ok"] != D["ok"]).any() == (md == 0.75)
        out.append(c)
    offs = rng.uniform(-0.5, 0.5, (21, 3))
    rows = [(S[b % 16], AXES[b % 3], offs[b]) for b in range(21)]
    c = exact_case("all_rejected", rows, [(0.001 * (p + 1), 0.0, 0.0) for p in range(P)], 1e-9, 0.1, tags=("all_rejected",))
    assert not c.discrete()["ok"].any()
    out.append(c)
    return out


def random_normals(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def scene_case(name, P, B, tags, K=8, origin=(0.0, 0.0, 0.0), rot=0.002, trans=0.02, max_dist=0.003, delta=0.03, min_steps=1, accept=None,
               grid_x=None, bare_every=11):
    """A jittered 8^3 grid as the target with random unit normals (every bare_every-th target has none); row b's candidates are K
    distinct grid points in random order, its source point lies near the one at slot b mod K.  accept [B] (None: all near):
    True puts the point within 0.04 of the winner per axis, False 0.2 away from it (rejected by the gate, still the winner)."""
    rng = rng_for(name)
    tgt = sc.jitter_grid(rng, 8, origin=origin)
    nrm = random_normals(rng, 512) * rng.uniform(0.5, 2.0, (512, 1))        # supplied normals need not be unit
    if bare_every:
        nrm[::bare_every] = 0.0
    cand = np.stack([rng.permutation(512)[:K] for _ in range(B)]).astype(np.int32)
    planted = np.arange(B) % K
    near = rng.uniform(-0.04, 0.04, (B, 3))
    if accept is not None:
        u = random_normals(rng, B)
        near = np.where(np.asarray(accept)[:, None], near, 0.2 * u)
    src = tgt[cand[np.arange(B), planted]] + near
    c = PlaneCase(name, tags, src, tgt, nrm, cand, sc.lane_poses(rng, P, rot=rot, trans=trans), max_dist, delta, min_steps=min_steps, grid_x=grid_x)
    assert (c.discrete()["win"] == planted[None]).all()
    return c


GEOMETRY_P = (1, 4, 16, 17, 32, 33, 64, 65, 128, 130, 257)


def geometry_cases():
    """Every (PW, WP) — (16,1): P 1, 4, 16; (32,1): 17, 32; (64,1): 33, 64; (64,2): 65, 128; (64,4): 130, 257 (grid_y = 2) —
    meets B in {1, pass - 1, pass, pass + 1, 2 pass + 1, 3 pass}, split between the particle counts of a geometry."""
    out = []
    seen = {}
    for P in GEOMETRY_P:
        pp = sc.points_per_pass(P)
        kinds = [1, pp - 1, pp, pp + 1, 2 * pp + 1, 3 * pp]
        nth = sum(1 for Q in GEOMETRY_P if Q < P and sc.stage_b_shape(Q) == sc.stage_b_shape(P))
        pick = sorted({b for i, b in enumerate(kinds) if b > 0 and (pp == 1 or i % 2 == nth % 2)})
        for B in pick:
            out.append(scene_case("geom_P%d_B%d" % (P, B), P, B, ("geometry",)))
            seen.setdefault(sc.stage_b_shape(P), set()).add(B)
    for (PW, WP), bs in seen.items():
        pp = (64 // PW) * (4 // WP)
        assert bs >= {b for b in (1, pp - 1, pp, pp + 1, 2 * pp + 1, 3 * pp) if b > 0}, (PW, WP, sorted(bs))
    # more than one pass per workgroup (the product's default asks for four): the second trip of the U = 2 loop, its prefetch
    # past the block, and a last workgroup with an odd number of passes
    for P, B, ms in ((12, 16 * 7 + 3, 3), (12, 16 * 13 - 1, 4), (40, 4 * 9 + 1, 3), (130, 11, 4), (257, 7, 3)):
        out.append(scene_case("trips_P%d_B%d_steps%d" % (P, B, ms), P, B, ("geometry", "trips"), min_steps=ms))
    return out


FINALIZE_GRIDS = (1, 15, 16, 17, 127, 128, 129, 145, 257)


def finalize_cases():
    """P = 12 (PW = 16: 16 points per pass, one pass per workgroup): grid_x workgroups, every other count with a partial last
    workgroup.  Workgroup g accepts 1 + (7 g mod 16) of its rows (capped by the rows it has): a skipped or doubled workgroup
    changes the accepted count, which is compared exactly."""
    out = []
    for i, g in enumerate(FINALIZE_GRIDS):
        B = 16 * g - (5 if i % 2 else 0)
        blk = np.arange(B) // 16
        accept = (np.arange(B) % 16) < 1 + (7 * blk) % 16
        c = scene_case("finalize_grid%d" % g, 12, B, ("finalize",), rot=2e-5, trans=1e-4, max_dist=0.01, delta=0.03, accept=accept, grid_x=g, bare_every=0)
        D = c.discrete()
        assert (D["mask"] == accept[None]).all()
        per = np.array([[D["ok"][p, blk == k].sum() for k in range(g)] for p in (0, 11)])
        assert c.expected_grid()[0] == g and c.B <= 4112
        assert per.min() >= 1, "every workgroup adds to the accepted count"
        c.facts = dict(min_block_count=int(per.min()), blocks=g)
        out.append(c)
    return out


def conditioning_cases():
    out = []
    c = scene_case("km_coordinates", 24, 45, ("conditioning", "km"), origin=(3000.0, -2000.0, 50.0), rot=2e-6)
    assert np.abs(np.cross(c.src, c.nrm[c.cand[:, 0]])).max() > 1e3
    out.append(c)
    # b cancels: rows in pairs with one source point, one normal and opposite residuals (not an exact mirror image: that would
    # cancel to exactly 0); identity poses for the first six particles, the others do not cancel
    name = "b_cancels"
    rng = rng_for(name)
    n, K, P = 40, 4, 12
    base = np.array([3000.0, -2000.0, 50.0]) + rng.uniform(-20, 20, (n, 3))
    e = rng.uniform(-0.2, 0.2, (n, 3))
    src = np.repeat(base, 2, 0)
    offs = np.stack([e, -e * (1.0 + 2e-13)], 1).reshape(-1, 3)
    nr = np.repeat(random_normals(rng, n), 2, 0)
    B = 2 * n
    tgt = np.zeros((B * K, 3))
    nrm = np.tile(AXES[2], (B * K, 1))
    cand = np.arange(B * K, dtype=np.int32).reshape(B, K)
    for b in range(B):
        tgt[cand[b]] = src[b] + 50.0 + rng.uniform(0, 5, (K, 3))
        tgt[cand[b, b % K]] = src[b] - offs[b]
        nrm[cand[b, b % K]] = nr[b]
    poses = np.tile(IDENT, (P, 1))
    poses[6:, :9] += rng.uniform(-1e-5, 1e-5, (6, 9))
    poses[6:, 9:] = rng.uniform(-0.01, 0.01, (6, 3))
    c = PlaneCase(name, {"conditioning", "cancel"}, src, tgt, nrm, cand, poses, 1.0, 0.08)
    D = c.discrete()
    assert D["ok"].all()
    v, mag = c.f64()
    ratio = np.abs(v[:6, 21:27]) / mag[:6, 21:27]
    assert ratio.max() <= 1e-11 and (ratio > 0).any(), ratio.max()
    assert (np.abs(v[6:, 21:24]) / mag[6:, 21:24]).min() > 1e-7
    c.facts = dict(cancel=float(ratio.max()))
    out.append(c)
    return out


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        with np.errstate(all="ignore"):
            cs = exact_cases() + geometry_cases() + finalize_cases() + conditioning_cases()
        assert len({c.name for c in cs}) == len(cs)
        for c in cs:
            assert c.winner_margin() >= 4.0, (c.name, c.winner_margin())
            assert not c.discrete()["tie"].any(), c.name
            if "exact" not in c.tags:
                g, k = c.edge_distance()
                assert g >= 1e-9 and k >= 1e-9, (c.name, g, k)
        _CASES = cs
    return _CASES


def by_name(name):
    return {c.name: c for c in all_cases()}[name]


def variants(case):
    """name -> (options, record_trace): k_plane_accumulate<PW, WP, false> and <PW, WP, true>."""
    return {"plain": (case.options(), False), "traced": (case.options(), True)}
