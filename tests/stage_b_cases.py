"""Hand-built inputs of stage B alone (test infrastructure): candidate tables, clouds and total poses.

A case is what tests/test_stage_b_gpu.py hands the kernels through the split-phase ABI: a source cloud, a target cloud, a
candidate table cand [B][K] (written into svnicp_candidates_devptr; stage A never runs), total poses [P][12] (written into
svnicp_total_pose_devptr) and max_dist.  Every candidate index lies in [0, M); no case feeds a kernel anything it would have
to survive.  Clouds come from the seeded generator of this module; a checksum ties each case to tests/golden/stage_b.npz.
Each builder asserts on the host, with the discrete part of tests/stage_b_reference.py, that the case reaches its regime;
what it measured is kept in Case.facts.  Shapes are the smallest that reach the regime (B up to about 300, M <= 512); the
queue-overflow cases are sized from the device's CU count and are not in the fixture.

The search kernel's certificate is restated here for the builders only (f32_scores: EPS = 54 u Cq (Cq + 2 X2) of
stein_split_device.hpp, and a float32 score as numpy evaluates it): a case asserts with it that a float32 pick alone would
be wrong, or that a gap lies on the decided side.  The tests never compare the device against it.
"""
import zlib

import numpy as np

import stage_b_reference as ref

U = 2.0 ** -24
QUEUE_CAP = 1024          # kQueueCap of stein_split_device.hpp
PLACEMENT_K = (1, 15, 16, 17, 32, 33, 64, 65, 96, 97, 100, 101, 112, 113, 128)
GEOMETRY_P = (9, 16, 17, 32, 33, 64, 65, 128, 129, 130, 257)
IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)


class Case:
    def __init__(self, name, tags, src, tgt, cand, poses, max_dist, svgd=False, shard=None, row_shard=None, options=(), mp=True,
                 facts=None):
        self.name, self.tags = name, frozenset(tags)
        self.src = np.ascontiguousarray(src, np.float64)
        self.tgt = np.ascontiguousarray(tgt, np.float64)
        self.cand = np.ascontiguousarray(cand, np.int32)
        self.poses = np.ascontiguousarray(poses, np.float64)
        self.max_dist, self.svgd, self.shard, self.row_shard = float(max_dist), bool(svgd), shard, row_shard
        self.options, self.mp, self.facts = tuple(options), mp, dict(facts or {})
        self.B, self.K, self.M, self.P = self.src.shape[0], self.cand.shape[1], self.tgt.shape[0], self.poses.shape[0]
        assert self.src.shape == (self.B, 3) and self.tgt.shape == (self.M, 3) and self.poses.shape == (self.P, 12)
        assert self.cand.shape[0] == self.B and 1 <= self.K <= 128 and self.M <= 512
        assert self.cand.min() >= 0 and self.cand.max() < self.M, "every candidate index lies in [0, M)"
        assert np.isfinite(self.src).all() and np.isfinite(self.tgt).all() and np.isfinite(self.poses).all()
        self._D = None

    def discrete(self, variant=()):
        if variant:
            return ref.discrete(self.src, self.tgt, self.cand, self.poses, self.max_dist, variant)
        if self._D is None:
            self._D = ref.discrete(self.src, self.tgt, self.cand, self.poses, self.max_dist)
        return self._D

    def particles(self):
        """The shard's particles [lo, hi)."""
        return self.shard if self.shard is not None else (0, self.P)

    def mp_particles(self):
        return ref.mp_particles(self.P, self.shard)

    def checksum(self):
        blob = b"".join(a.tobytes() for a in (self.src, self.tgt, self.cand, self.poses)) + \
            repr((self.max_dist, self.svgd, self.shard, self.row_shard, self.options)).encode()
        return np.int64(zlib.crc32(blob))


def variants(case):
    """Launch variants that admit the case: name -> (options, record_trace).  chain=general throughout, so that
    k_reduce_partials runs; accum_min_steps=1, so that several workgroups feed it at small B.  plain: the product's
    k_stein_accumulate_w<.., true> (and <.., true, true> in SVGD mode) reading kidx; traced: <.., false> reading the slot byte."""
    base = (("chain", "general"), ("accum_min_steps", "1")) + case.options
    v = {"plain": (base + (("accum", "split"),), False), "traced": (base + (("accum", "split"),), True),
         "f64": (base + (("accum", "f64"),), True), "valu": (base + (("accum", "valu"),), True)}
    lo, hi = case.particles()
    assert hi - lo > 8, "a shard of at most 8 particles never reaches the matrix-pipe search"
    return v


# ------------------------------------------------------------------------------------------------ building blocks
def rng_for(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def jitter_grid(rng, n, spacing=1.0, jitter=0.15, origin=(0.0, 0.0, 0.0)):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij"), -1).reshape(-1, 3) * spacing
    return g + rng.uniform(-jitter, jitter, g.shape) + np.asarray(origin, np.float64)


def lane_poses(rng, P, rot=0.002, trans=0.02):
    """Arbitrary doubles near the identity, distinct per particle: a lane that read another lane's rows would be seen."""
    poses = np.tile(IDENT, (P, 1))
    poses[:, :9] += rng.uniform(-rot, rot, (P, 9))
    poses[:, 9:] = rng.uniform(-trans, trans, (P, 3))
    assert len({r.tobytes() for r in poses}) == P
    return poses


def planted_scene(rng, B, K, planted=None, origin=(0.0, 0.0, 0.0)):
    """A jittered 8^3 grid as the target; row b's candidates are K distinct random grid points in random order, and its source
    point lies within 0.09 of the candidate at slot planted[b] (b mod K by default): the others are at least 0.7 away."""
    tgt = jitter_grid(rng, 8, origin=origin)
    cand = np.stack([rng.permutation(512)[:K] for _ in range(B)]).astype(np.int32)
    planted = np.arange(B) % K if planted is None else np.asarray(planted)
    src = tgt[cand[np.arange(B), planted]] + rng.uniform(-0.05, 0.05, (B, 3))
    return src, tgt, cand, planted


def stage_b_shape(n):
    """(PW, WP) of registration_plan.hpp: stage_b_shape for the split variant and a shard of n particles."""
    PW = 16
    while PW < 64 and PW < n:
        PW <<= 1
    WP = 1
    if PW == 64:
        WP = (n + 63) // 64
        if WP >= 3:
            WP = 4
    return PW, WP


def points_per_pass(n):
    PW, WP = stage_b_shape(n)
    return (64 // PW) * (4 // WP)


def f32_scores(case):
    """float32 scores S[P][B][K] as numpy evaluates cc + c . m on the search kernel's float32 inputs, and EPS [P][B]."""
    D = case.discrete()
    q = case.tgt[case.cand]                                  # [B][K][3]
    a = q[:, :1]
    c = (q - a).astype(np.float32).astype(np.float64)
    cc = ((c[..., 0] ** 2 + c[..., 1] ** 2) + c[..., 2] ** 2).astype(np.float32).astype(np.float64)
    x = (D["Ts"] - a[None, :, 0]).astype(np.float32).astype(np.float64)          # [P][B][3]
    m = -2.0 * x
    S = (cc[None] + (c[None] * m[:, :, None, :]).sum(-1)).astype(np.float32)
    C2 = np.sqrt((c ** 2).sum(-1)).max(1) * 1.0000002
    X2 = np.sqrt((x ** 2).sum(-1)) * 1.000002
    Cq = C2[None] + U * X2
    return S, 54.0 * U * Cq * (Cq + 2.0 * X2)


def all_d2(case):
    """float64 d2 [P][B][K] of every slot, the discrete part's expression."""
    Ts = case.discrete()["Ts"]
    q = case.tgt[case.cand]
    dx, dy, dz = (Ts[:, :, None, i] - q[None, :, :, i] for i in range(3))
    return (dx * dx + dy * dy) + dz * dz


# ------------------------------------------------------------------------------------------------ search: winner placement
def placement_case(K, P):
    name = "place_K%d_P%d" % (K, P)
    rng = rng_for(name)
    B = K + 3 if K > 1 else 5
    src, tgt, cand, planted = planted_scene(rng, B, K)
    c = Case(name, {"search", "placement"}, src, tgt, cand, lane_poses(rng, P), 0.003)
    D = c.discrete()
    assert (D["win"] == planted[None]).all() and not D["tie"].any(), name
    won = set(D["win"].reshape(-1).tolist())
    assert won == set(range(K)), "every slot of every tile wins somewhere"
    assert 0 in won and K - 1 in won and all(k in won for k in range(96, min(K, 100)))
    d2 = all_d2(c)[0]
    assert K < 3 or (np.diff(d2, axis=1) < 0).any(axis=1).all(), "the table is unsorted by distance"
    assert D["mask"].any() and (K == 1 or not D["mask"].all())
    c.facts = dict(slots=len(won), accepted=float(D["mask"].mean()))
    return c


# ------------------------------------------------------------------------------------------------ search: exact ties
def mirror_target(rng, n=16, spacing=2.0):
    """n x n cells in the plane z = 0, each with the mirror pair (x, y, +c), (x, y, -c), c in [0.3, 0.5] per cell: target rows
    2 cell and 2 cell + 1.  (c is no float32 value: which of the pair a float32 score prefers differs from cell to cell.)"""
    xy = np.stack(np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij"), -1).reshape(-1, 2) * spacing
    xy = xy + rng.uniform(-0.2, 0.2, xy.shape)
    tgt = np.zeros((2 * n * n, 3))
    tgt[0::2, :2] = xy; tgt[1::2, :2] = xy
    c = rng.uniform(0.3, 0.5, n * n)
    tgt[0::2, 2] = c; tgt[1::2, 2] = -c
    return tgt, n


def mirror_poses(rng, P, untied_every=0, dz=0.25):
    """Identity rotations; translations inside the mirror plane z = 0 (such a particle ties a mirror pair exactly), except
    that every `untied_every`-th particle leaves the plane by +-dz."""
    poses = np.tile(IDENT, (P, 1))
    poses[:, 9:11] = rng.uniform(-0.1, 0.1, (P, 2))
    if untied_every:
        off = np.arange(P) % untied_every == untied_every - 1
        poses[off, 11] = np.where(np.arange(P)[off] % (2 * untied_every) < untied_every, dz, -dz)
    return poses


def neighbour_cells(cell, n, rng, count):
    """`count` distinct cells within three cells of `cell` (not itself): far candidates that keep C2 below 9."""
    i, j = divmod(cell, n)
    near = [a * n + b for a in range(max(0, i - 3), min(n, i + 4)) for b in range(max(0, j - 3), min(n, j + 4)) if (a, b) != (i, j)]
    return rng.permutation(near)[:count]


def ties_case(P):
    """K = 100 (the tail tile is candidates 96..99).  Row kinds, cycling: 0 the same target index at slots 4 and 61; 1 a mirror
    pair inside one tile (slots 5, 6); 2 across tiles (2, 37); 3 with the tail tile (7, 98); 4 all K slots the same index;
    5..8 as 0..3 with the two slots exchanged.  Three particles of four lie in the mirror plane and tie, the fourth does not."""
    name = "ties_K100_P%d" % P
    rng = rng_for(name)
    K, B = 100, 45
    tgt, n = mirror_target(rng, n=15)       # 450 rows
    pairs = {0: (4, 61), 1: (5, 6), 2: (2, 37), 3: (7, 98)}
    cand = np.zeros((B, K), np.int32)
    src = np.zeros((B, 3))
    lowest = np.zeros(B, np.int64)
    for b in range(B):
        kind = b % 9
        base, swapped = (kind, False) if kind < 5 else (kind - 5, True)
        cell = int(rng.integers(n * n))
        src[b, :2] = tgt[2 * cell, :2] + rng.uniform(-0.1, 0.1, 2)
        others = rng.permutation(np.delete(np.arange(n * n), cell))[:50]
        row = rng.permutation(np.concatenate([2 * others, 2 * others + 1]))[:K]
        plus, minus = 2 * cell, 2 * cell + 1
        if base == 4:
            row[:] = plus
        else:
            lo, hi = pairs[base]
            lowest[b] = lo
            if base == 0:
                row[lo] = row[hi] = minus if swapped else plus
            else:
                row[lo], row[hi] = (minus, plus) if swapped else (plus, minus)
        cand[b] = row
    c = Case(name, {"search", "ties"}, src, tgt, cand, mirror_poses(rng, P, untied_every=4), 1.0)
    D = c.discrete()
    plane = c.poses[:, 11] == 0.0
    assert D["tie"][plane].all() and plane.sum() == P - P // 4
    assert (D["win"][plane] == lowest[None]).all(), "the lowest slot wins a tie"
    assert (D["tie"][~plane] == np.isin(np.arange(B) % 9, (0, 4, 5))[None]).all(), "off the plane only equal indices tie"
    assert (D["win"][~plane] != lowest[None]).any(), "off the plane the nearer of a mirror pair wins, at either slot"
    Dle = c.discrete(("argmin_le",))
    assert (Dle["win"] != D["win"])[D["tie"]].all(), "the last index winning is another answer wherever there is a tie"
    c.facts = dict(tied=float(D["tie"].mean()))
    return c


def overflow_cases(num_cus):
    """Two cases that make every search workgroup defer more than its queue holds (P = 64, K = 16, option wgpcu=1,1: one
    workgroup per CU, B / CUs points each).  `full`: the 16 slots hold a mirror pair in turn and every particle lies in the mirror
    plane, so every pair is a 16-way tie: the queue is full after 16 wave steps and the rest is settled in the loop.  `holes`: a
    mirror pair at slots 3 and 9 ties the 48 particles of each 64 that lie in the mirror plane: 21 steps fill 1008 entries, step 22
    straddles the end and leaves 16 sentinel slots."""
    P, K = 64, 16
    B = (2 * QUEUE_CAP * num_cus + P - 1) // P
    out = []
    for kind in ("full", "holes"):
        name = "overflow_%s" % kind
        rng = rng_for(name)
        tgt, n = mirror_target(rng)
        cell = np.arange(B) % (n * n)
        src = np.zeros((B, 3))
        src[:, :2] = tgt[2 * cell, :2] + rng.uniform(-0.1, 0.1, (B, 2))
        if kind == "full":     # the cell's mirror pair alternating over the 16 slots, every particle in the mirror plane
            cand = 2 * cell[:, None] + ((np.arange(K)[None, :] + np.arange(B)[:, None]) & 1)
            poses = mirror_poses(rng, P)
        else:
            cand = np.zeros((B, K), np.int64)
            for b in range(B):
                far = neighbour_cells(int(cell[b]), n, rng, 7)
                cand[b] = np.concatenate([2 * far, 2 * far + 1, 2 * far[:2]])
                cand[b, 3], cand[b, 9] = 2 * cell[b] + (b & 1), 2 * cell[b] + 1 - (b & 1)
            poses = mirror_poses(rng, P, untied_every=4)
        c = Case(name, {"search", "overflow"}, src, tgt, cand, poses, 0.2, options=(("wgpcu", "1,1"),), mp=False)
        D = c.discrete()
        steps = -(-B // 4)                                   # plan_accumulate's size_grid for (PW, WP) = (64, 1): four points per wave step,
        per_wg = -(-steps // min(steps, num_cus)) * 4 * P    # one workgroup per CU; pairs a search workgroup meets
        assert B * P >= 2 * QUEUE_CAP * num_cus and per_wg >= 2 * QUEUE_CAP
        if kind == "full":
            assert D["tie"].all() and (D["win"] == 0).all()
            assert (f32_scores(c)[0].argmin(-1) != 0).mean() > 0.25, "a float32 pick alone names another slot on a quarter of the pairs"
            c.facts = dict(expected_ambiguous=B * P)
        else:
            plane = poses[:, 11] == 0.0
            assert plane.sum() == 48 and D["tie"][plane].all() and not D["tie"][~plane].any()
            assert (D["win"][plane] == 3).all() and set(D["win"][~plane].reshape(-1)) == {3, 9}
            S, eps = f32_scores(c)
            S2 = np.sort(S[~plane].astype(np.float64), axis=-1)
            assert ((S2[..., 1] - S2[..., 0]) > 100 * eps[~plane]).all(), "the other 16 lanes are decided by a wide margin"
            assert 21 * 48 < QUEUE_CAP < 22 * 48, "step 22 straddles the end of the queue"
            c.facts = dict(expected_ambiguous=B * 48)
        assert D["mask"].any() and not D["mask"].all()
        out.append(c)
    return out


# ------------------------------------------------------------------------------------------------ search: certificate
def gap_facts(c, s1, s2):
    """Of the pairs whose two contenders sit at slots s1[b], s2[b]: the float64 gaps against EPS and 1 ulp of d2."""
    d2 = all_d2(c)
    rows = np.arange(c.B)
    a, b = d2[:, rows, s1], d2[:, rows, s2]
    gap = np.abs(a - b)
    S, eps = f32_scores(c)
    wrong = (S[:, rows, s1] < S[:, rows, s2]) != (a < b)
    below = (gap < eps) & (gap > 0)
    return dict(gap=gap, eps=eps, ulp=np.spacing(np.minimum(a, b)), wrong_below=float(wrong[below].mean()) if below.any() else 0.0,
                below=int(below.sum()), above2=int((gap > 2 * eps).sum()), ties=int((gap == 0).sum()))


def cert_gaps_case(P, origin=(0.0, 0.0, 0.0), tag=""):
    """K = 5.  Slot 0 (the anchor) at distance 1 from the point; two contenders at 0.995 of that distance, so that their scores
    |y|^2 - 2 y.x nearly cancel (0.01 against C2 X2 of about 2); they share x and y and differ in z by an amount that sets their d2
    gap: 1 ulp of d2 doubling per row up to beyond 4 EPS.  Coordinates are random doubles, not float32 values.  The particles are
    translated across z only, which leaves every gap as planted up to the rounding of d2."""
    name = "cert_gaps%s_P%d" % (tag, P)
    rng = rng_for(name)
    K, noct = 5, 43
    B = 2 * noct
    tgt = np.zeros((B * K, 3))
    cand = np.arange(B * K, dtype=np.int32).reshape(B, K)
    src = rng.uniform(-2, 2, (B, 3)) + np.asarray(origin)
    s1, s2 = np.ones(B, np.int64), np.where(np.arange(B) % 4 < 2, 2, 4)      # the contenders' slots: one tile, or two

    def unit():
        v = rng.normal(size=3)
        return v / np.linalg.norm(v)
    for b in range(B):
        tgt[cand[b, 0]] = src[b] + unit()
        for k in range(1, K):
            tgt[cand[b, k]] = src[b] + 1.5 * unit()
        r2 = 0.99
        cz = rng.uniform(0.5, 0.8)
        ab = np.sqrt(r2 - cz * cz) * np.array([np.cos(b * 0.7), np.sin(b * 0.7)])
        g = np.spacing(r2) * 2.0 ** (b // 2)
        cz2 = np.sqrt(cz * cz + g)
        near, far = (cz, -cz2) if b % 2 == 0 else (-cz, cz2)
        lo, hi = (s1[b], s2[b]) if (b // 4) % 2 == 0 else (s2[b], s1[b])    # the nearer contender at the lower or at the higher slot
        tgt[cand[b, lo]] = src[b] + np.array([ab[0], ab[1], near])
        tgt[cand[b, hi]] = src[b] + np.array([ab[0], ab[1], far])
    poses = np.tile(IDENT, (P, 1))
    poses[:, 9:11] = rng.uniform(-1e-3, 1e-3, (P, 2))
    c = Case(name, {"search", "certificate"}, src, tgt, cand, poses, 1.0)
    assert not np.array_equal(c.tgt, c.tgt.astype(np.float32).astype(np.float64))
    D = c.discrete()
    assert np.isin(D["win"], (1, 2, 4)).all()
    f = gap_facts(c, s1, s2)
    S, eps = f32_scores(c)
    assert (np.abs(S[:, np.arange(B), s1]) < 0.02 * 2.0).all(), "|score| << C2 X2"
    lg = np.sort(np.log2(f["gap"][0][f["gap"][0] > 0]))
    assert np.diff(lg).max() <= 1.75 and (f["gap"] >= 4 * f["eps"]).any(), "octave steps up to 4 EPS"
    if not tag:     # (kilometre coordinates have a spacing of 9e-13: the smallest gap there is 1e-12, not an ulp of d2)
        assert ((f["gap"] > 0) & (f["gap"] <= 4 * f["ulp"])).any(), "... from a few ulp of d2"
    assert f["wrong_below"] >= 0.1, "a float32 score alone picks the wrong candidate on a tenth of the pairs below EPS"
    assert f["above2"] > 0, "some gaps lie on the decided side"
    c.facts = {k: f[k] for k in ("wrong_below", "below", "above2", "ties")}
    return c


def cert_close_case(name, spacing, dists, P=32):
    """K = 16 candidates within `spacing` of the anchor, the point at dists[b mod len] from it: candidates closer together than
    2^-24 of their distance to the point (the u X2 term of Cq), or so close that |c|^2 underflows in float32."""
    rng = rng_for(name)
    K, B = 16, 32
    tgt = np.zeros((B * K, 3))
    cand = np.stack([rng.permutation(K) + K * b for b in range(B)]).astype(np.int32)
    src = np.zeros((B, 3))
    for b in range(B):
        anchor = rng.uniform(-1, 1, 3) if spacing > 1e-20 else np.zeros(3)
        tgt[K * b:K * (b + 1)] = anchor + spacing * rng.uniform(-1, 1, (K, 3))
        v = rng.normal(size=3)
        src[b] = anchor + dists[b % len(dists)] * v / np.linalg.norm(v)
    poses = lane_poses(rng, P, rot=1e-3, trans=0.0)
    c = Case(name, {"search", "certificate", "close"}, src, tgt, cand, poses, 1e3)
    assert len({r.tobytes() for r in c.tgt}) == c.M, "distinct target rows"
    S, eps = f32_scores(c)
    d2 = np.sort(all_d2(c), -1)
    c.facts = dict(f64_ties=float(c.discrete()["tie"].mean()), gap_over_eps=float(np.median((d2[..., 1] - d2[..., 0]) / eps)))
    return c


def cert_c2_case(P=32):
    """C2 of 1e3 m: slot 0 and the fill-in candidates lie a kilometre from the point, two contenders 0.5 m from it with a gap of
    1e-6 m between their distances."""
    name = "cert_c2_1e3"
    rng = rng_for(name)
    K, B = 8, 48
    tgt = np.zeros((B * K, 3))
    cand = np.arange(B * K, dtype=np.int32).reshape(B, K)
    src = rng.uniform(-2, 2, (B, 3))

    def unit():
        v = rng.normal(size=3)
        return v / np.linalg.norm(v)
    slots = np.zeros((B, 2), np.int64)
    for b in range(B):
        for k in range(K):
            tgt[cand[b, k]] = src[b] + rng.uniform(500, 1000) * unit()
        tgt[cand[b, 0]] = src[b] + 1000.0 * unit()
        s = rng.permutation(np.arange(1, K))[:2]
        tgt[cand[b, s[0]]] = src[b] + 0.5 * unit()
        tgt[cand[b, s[1]]] = src[b] + (0.5 + 1e-6) * unit()
        slots[b] = s
    poses = np.tile(IDENT, (P, 1))
    poses[:, 9:] = rng.uniform(-3e-6, 3e-6, (P, 3))     # enough to exchange the contenders for some particles
    c = Case(name, {"search", "certificate"}, src, tgt, cand, poses, 1.0)
    D = c.discrete()
    assert np.isin(D["win"], slots).all() and D["mask"].all()
    f = gap_facts(c, slots[:, 0], slots[:, 1])
    assert (f["eps"] > 1.0).all() and (f["gap"] < 1e-5).all() and f["below"] > 0.9 * P * B
    assert 0 < (D["win"] == slots[None, :, 1]).mean() < 1, "both contenders win somewhere"
    c.facts = dict(wrong_below=f["wrong_below"], eps=float(f["eps"].mean()))
    return c


# ------------------------------------------------------------------------------------------------ accumulate
def exact_rows(offsets, P=12, K=4, max_dist=1.0, name="", tags=(), src=None, particle_shift=None, svgd=False):
    """Identity poses (particle p > 0 translated by particle_shift[p] along x) and one candidate exactly at src + offsets[b]
    at slot b mod K, the other slots 50 away: d2 of particle 0 is |offsets[b]|^2 as far as it is representable."""
    rng = rng_for(name)
    offsets = np.asarray(offsets, np.float64)
    B = len(offsets)
    src = rng.integers(-8, 9, (B, 3)).astype(np.float64) if src is None else np.asarray(src, np.float64)
    tgt = np.zeros((B * K, 3))
    cand = np.arange(B * K, dtype=np.int32).reshape(B, K)
    for b in range(B):
        tgt[cand[b]] = src[b] + 50.0 + rng.uniform(0, 5, (K, 3))
        tgt[cand[b, b % K]] = src[b] - offsets[b]           # e = Ts - q = offsets[b] at the identity pose
    poses = np.tile(IDENT, (P, 1))
    if particle_shift is not None:
        poses[:, 9] = particle_shift
    return Case(name, set(tags) | {"accumulate"}, src, tgt, cand, poses, max_dist, svgd=svgd)


def mask_edge_cases():
    half = [(0.5, 0.5, 0.5), (-0.5, 0.5, -0.5), (0.5, -0.5, 0.0), (0.5, 0.5, 0.75), (0.0, 0.0, 0.0), (-0.5, -0.5, 0.5), (0.25, 0.5, 0.5)] * 3
    shift = 0.25 * (np.arange(12) % 3)      # dx stays a multiple of 0.25: every d2 is exact
    out = []
    for name, md in (("mask_edge_at", 0.75), ("mask_edge_above", np.nextafter(0.75, 1.0))):
        c = exact_rows(half, max_dist=md, name=name, tags=("mask",), particle_shift=shift)
        D = c.discrete()
        at = D["d2"] == 0.75
        assert at.sum() >= 12 and (D["mask"][at] == (md > 0.75)).all(), "d2 exactly at max_dist is rejected, one ulp above it accepted"
        assert (c.discrete(("mask_le",))["mask"] != D["mask"]).any() == (md == 0.75)
        c.facts = dict(at_edge=int(at.sum()))
        out.append(c)
    rng = rng_for("mask_all")
    offs = rng.uniform(-0.5, 0.5, (37, 3))
    c = exact_rows(offs, max_dist=1e-9, name="mask_all_rejected", tags=("mask", "all_rejected"), particle_shift=0.001 * np.arange(12) + 0.001)
    assert not c.discrete()["mask"].any()
    out.append(c)
    c = exact_rows(offs, max_dist=1e3, name="mask_all_accepted", tags=("mask",), particle_shift=0.001 * np.arange(12))
    assert c.discrete()["mask"].all()
    out.append(c)
    return out


def residual_edge_cases():
    out = []
    tiny = [(0.0, 0.0, 0.0), (1e-155, 0.0, 0.0), (0.0, 2.0 ** -500, 0.0), (0.0, 0.0, 1e-160), (2.0 ** -537, 0.0, 0.0), (0.0, 0.0, 0.0), (1e-100, 1e-100, 0.0)] * 3
    for md in (1e-3, 1.0, 1e3):
        name = "resid_tiny_md%g" % md
        shift = np.where(np.arange(12) % 2 == 0, 0.0, 0.01 * np.sqrt(md) * np.arange(12))
        c = exact_rows(tiny, max_dist=md, name=name, tags=("residual",), src=np.zeros((len(tiny), 3)), particle_shift=shift)
        D = c.discrete()
        d2 = D["d2"][0]
        assert (d2 == 0).sum() == 6 and ((d2 > 0) & (d2 < 2.0 ** -1000)).sum() >= 6 and (d2 == 2.0 ** -1000).sum() == 3
        assert np.isclose(d2[1], 1e-310, rtol=1e-6) and D["mask"][0].all()
        out.append(c)
        name = "resid_band_md%g" % md
        rng = rng_for(name)
        r = np.sqrt(md * (1.0 + 1e-9 * np.array([-1, 1, -0.5, 0.5, -0.01, 0.01, -1, 1, -2, 2, -0.3, 0.3, 0.0])))
        v = rng.normal(size=(len(r), 3))
        offs = r[:, None] * v / np.linalg.norm(v, axis=1, keepdims=True)
        c = exact_rows(offs, max_dist=md, name=name, tags=("residual", "band"), particle_shift=shift)
        D = c.discrete()
        band = np.abs(D["d2"] / md - 1.0) <= 2.1e-9
        assert band[::2].all() and D["mask"][band].any() and not D["mask"][band].all()
        c.facts = dict(in_band=int(band.sum()), accepted=int(D["mask"][band].sum()))
        out.append(c)
    return out


def cancelling_case():
    """Source coordinates of kilometres; rows come in pairs with the same source point and opposite residuals, so that sum we
    and sum (we)_i s_j cancel to 1e-12 of sum |term| for the identity particles (the translated ones do not cancel)."""
    name = "cancel_km"
    rng = rng_for(name)
    n = 40
    base = np.array([5000.0, -3000.0, 200.0]) + rng.uniform(-20, 20, (n, 3))
    e = rng.uniform(-0.6, 0.6, (n, 3))
    src = np.repeat(base, 2, 0)
    offs = np.stack([e, -e * (1.0 + 2e-13)], 1).reshape(-1, 3)     # (an exact mirror image would cancel to exactly 0)
    P = 12
    c = exact_rows(offs, P=P, max_dist=1e3, name=name, tags=("cancel",), src=src, particle_shift=np.where(np.arange(P) < 6, 0.0, 0.01 * np.arange(P)))
    c.poses[6:, :9] += rng.uniform(-1e-4, 1e-4, (6, 9))
    c = Case(name, c.tags, c.src, c.tgt, c.cand, c.poses, c.max_dist)
    D = c.discrete()
    assert D["mask"].all()
    s, mag = ref.sums_f64(c.src, D, c.max_dist)
    ratio = np.abs(s[:6, 10:]) / mag[:6, 10:]
    assert ratio.max() <= 1e-12 and (ratio > 0).any(), ratio.max()
    assert (np.abs(s[6:, 10:13]) / mag[6:, 10:13]).min() > 1e-6
    c.facts = dict(cancel=float(ratio.max()))
    return c


def svgd_cases():
    out = []
    rng = rng_for("svgd")
    B = 29
    offs = rng.uniform(-0.3, 0.3, (B, 3))
    src = rng.integers(-8, 9, (B, 3)).astype(np.float64)
    src[src.sum(1) == 0, 0] += 1.0
    zero = src.copy()
    zero[::3] = np.array([1.0, 2.0, -3.0])
    shift = np.where(np.arange(12) % 2 == 0, 0.0, 0.125)
    c = exact_rows(offs, max_dist=1.0, name="svgd_zero_row", tags=("svgd",), src=zero, particle_shift=shift, svgd=True)
    D = c.discrete()
    assert D["mask"].all() and not D["cnt"][0, ::3].any() and D["cnt"][0].sum() == B - len(range(0, B, 3)) and D["cnt"][1].all()
    assert (c.discrete(("count_on_mask",))["cnt"] != D["cnt"]).any()
    out.append(c)
    c = exact_rows(offs, max_dist=1.0, name="svgd_count_B", tags=("svgd",), src=src, particle_shift=shift, svgd=True)
    assert c.discrete()["cnt"].all()
    out.append(c)
    c = exact_rows(offs, max_dist=1e-9, name="svgd_count_0", tags=("svgd", "all_rejected"), src=src, particle_shift=shift + 0.001, svgd=True)
    assert not c.discrete()["cnt"].any() and not c.discrete()["mask"].any()
    out.append(c)
    return out


# ------------------------------------------------------------------------------------------------ geometry
def geometry_case(name, P, B, shard=None, row_shard=None, K=8, origin=(0.0, 0.0, 0.0), rot=0.002):
    rng = rng_for(name)
    src, tgt, cand, planted = planted_scene(rng, B, K, origin=origin)
    c = Case(name, {"geometry"}, src, tgt, cand, lane_poses(rng, P, rot=rot), 0.003, shard=shard, row_shard=row_shard)
    D = c.discrete()
    assert (D["win"] == planted[None]).all()
    c.facts = dict(accepted=float(D["mask"].mean()))
    return c


def geometry_cases():
    out = []
    for P in GEOMETRY_P:
        pp = points_per_pass(P)
        for B in sorted({1, pp - 1, pp + 1, 4 * pp - 1, 4 * pp + 1} - {0}):
            out.append(geometry_case("geom_P%d_B%d" % (P, B), P, B))
    out.append(geometry_case("shard_3_20_of_24", 24, 4 * points_per_pass(17) + 1, shard=(3, 20)))
    out.append(geometry_case("shard_64_130_of_130", 130, 4 * points_per_pass(66) + 1, shard=(64, 130)))
    out.append(geometry_case("row_shard_1_of_2", 24, 41, row_shard=(1, 2, 82)))
    c = geometry_case("place_km", 12, 40, origin=(5000.0, -3000.0, 200.0), rot=2e-6)     # (a rotation error of 2e-6 is 1 cm at 5 km)
    c.tags = c.tags | {"km"}
    out.append(c)
    return out


_CASES = None


def all_cases():
    """Every case of the fixture (the queue-overflow cases are built by overflow_cases from the device's CU count)."""
    global _CASES
    if _CASES is None:
        with np.errstate(all="ignore"):
            cs = [placement_case(K, 12) for K in PLACEMENT_K] + [placement_case(K, 64) for K in (16, 100, 128)]
            cs += [ties_case(64), ties_case(16)]
            cs += [cert_gaps_case(64), cert_gaps_case(16), cert_gaps_case(32, origin=(5000.0, -3000.0, 200.0), tag="_km")]
            cs += [cert_close_case("cert_close_1e-9_at_10", 1e-9, (10.0,)), cert_close_case("cert_underflow_1e-25", 1e-25, (1.0, 3e-24)),
                   cert_c2_case()]
            cs += mask_edge_cases() + residual_edge_cases() + [cancelling_case()] + svgd_cases() + geometry_cases()
        assert len({c.name for c in cs}) == len(cs)
        _CASES = cs
    return _CASES


def by_name(name):
    return {c.name: c for c in all_cases()}[name]
