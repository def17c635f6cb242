"""The crafted particle sets and the two-basin scene that tests/test_particle_modes_cpu.py and tests/test_particle_modes_gpu.py
share.  Coordinates are dyadic wherever a test depends on an equality or on which side of a threshold a pair falls."""
import numpy as np

LINK_T, LINK_R = 0.5, 0.05          # the links of the chain cases and of the two-basin scene
CHAINS = (65, 257, 1030)            # one particle past a wave, past four waves, past 1024 threads

_M64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def permutation(n, seed=20251):
    """perm[k] = the particle index of chain position k: positions ordered by the splitmix64 hash of (seed, position)."""
    keys = [(_splitmix64(seed * 1000003 + k), k) for k in range(n)]
    order = [k for _, k in sorted(keys)]
    perm = np.empty(n, np.int64)
    perm[order] = np.arange(n)
    return perm


def _set(t=None, r=None, P=None):
    P = P if P is not None else (np.shape(t)[0] if t is not None else np.shape(r)[0])
    x = np.zeros((6, P))
    if t is not None:
        x[:3] = np.asarray(t, np.float64).reshape(P, 3).T
    if r is not None:
        x[3:] = np.asarray(r, np.float64).reshape(P, 3).T
    return x


def chain(n, gap_at=None):
    """n particles 0.875 * LINK_T apart along x (0.4375: every coordinate exact), one gap of 1.125 * LINK_T after chain
    position ``gap_at``; the particle at chain position k has index permutation(n)[k]."""
    pos = np.arange(n, dtype=np.float64) * (0.875 * LINK_T)
    if gap_at is not None:
        pos[gap_at + 1:] += 0.25 * LINK_T
    x = np.zeros((6, n))
    x[0, permutation(n)] = pos
    x[1], x[2] = 3.0, -1.5
    x[3:] = np.array([[0.0078125], [-0.015625], [0.0]])
    return x


def case(name, x, link_trans=LINK_T, link_rot=LINK_R, max_modes=8, weights=None, **expect):
    return dict(name=name, x=np.ascontiguousarray(x, np.float64), link_trans=float(link_trans), link_rot=float(link_rot), max_modes=max_modes,
                weights=None if weights is None else np.asarray(weights, np.float64), expect=expect)


def _weights_for(P):
    """Deterministic non-uniform weights in (0.5, 1.5], multiples of 2^-10."""
    return np.array([(1 + (_splitmix64(77 * 1000003 + p) >> 54)) / 1024.0 + 0.5 for p in range(P)])


def crafted():
    out = []
    out.append(case("single", _set(t=[[1.0, 2.0, 3.0]], r=[[0.01, 0.0, 0.0]]), n_modes=1, counts=[1]))
    # two particles split by one criterion alone
    out.append(case("pair_rot_splits", _set(t=[[0, 0, 0], [0.25, 0, 0]], r=[[0, 0, 0], [0, 0.0625, 0]]), n_modes=2, counts=[1, 1]))
    out.append(case("pair_trans_splits", _set(t=[[0, 0, 0], [0.75, 0, 0]], r=[[0, 0, 0], [0, 0.03125, 0]]), n_modes=2, counts=[1, 1]))
    out.append(case("pair_linked", _set(t=[[0, 0, 0], [0.25, 0, 0]], r=[[0, 0, 0], [0, 0.03125, 0]]), n_modes=1, counts=[2]))
    # the threshold itself: 0.375^2 + 0.5^2 = 0.390625 = 0.625^2 exactly
    edge = _set(t=[[1.0, 1.0, 1.0], [1.375, 1.5, 1.0]])
    out.append(case("edge_linked", edge, link_trans=0.625, n_modes=1, counts=[2]))
    out.append(case("edge_not_linked", edge, link_trans=np.nextafter(0.625, 0.0), n_modes=2, counts=[1, 1]))
    for n in CHAINS:
        out.append(case(f"chain_{n}", chain(n), n_modes=1, counts=[n]))
        half = n // 2 - 1 if n % 2 == 0 else n // 2      # even n: two equal halves, the order falls to the label
        out.append(case(f"broken_chain_{n}", chain(n, gap_at=half), n_modes=2, counts=sorted([half + 1, n - half - 1], reverse=True)))
    # mass, not count: three light particles against two heavy ones
    out.append(case("mass_not_count", _set(t=[[0, 0, 0], [0.25, 0, 0], [0, 0.25, 0], [8, 0, 0], [8.25, 0, 0]]),
                    weights=[0.125, 0.125, 0.125, 0.25, 0.375], n_modes=2, counts=[2, 3], labels_first=3))
    # more modes than are reported
    out.append(case("forty_singletons", _set(t=[[4.0 * k, 0.5 * (k % 3), 0] for k in range(40)]), max_modes=4, n_modes=40, counts=[1, 1, 1, 1]))
    # a NaN and an inf particle that would bridge two clusters
    t = [[0, 0, 0], [0.25, 0, 0], [0.625, 0, 0], [0.625, 0.125, 0], [1.0, 0, 0], [1.25, 0, 0]]
    x = _set(t=t)
    x[4, 2], x[0, 3] = np.nan, np.inf                    # particle 2: a NaN rotation component; particle 3: an infinite x
    out.append(case("nonfinite_between", x, n_modes=2, counts=[2, 2], nonfinite=2))
    # link 0: equal particles link, the rest are singletons
    d = _set(t=[[1, 2, 3], [1, 2, 3], [1, 2, 3.0000000000000004], [5, 5, 5], [1, 2, 3], [5, 5, 5]], r=[[0.01, 0, 0]] * 6)
    out.append(case("duplicates_link_zero", d, link_trans=0.0, link_rot=0.0, n_modes=3, counts=[3, 2, 1]))
    # translations near 1e6 m, differences of centimetres
    base = np.array([1.0e6, -2.0e6, 1.5e6])
    big = [base + [0.0, 0.0, 0.0], base + [0.03125, 0.0, 0.0], base + [0.0625, 0.015625, 0.0], base + [1.0, 0.0, 0.0], base + [1.03125, 0.0, 0.0]]
    out.append(case("large_coordinates", _set(t=big), link_trans=0.046875, n_modes=2, counts=[3, 2]))
    # every set once more with non-uniform weights
    for c in list(out):
        if c["weights"] is None:
            out.append(dict(c, name=c["name"] + "_weighted", weights=_weights_for(c["x"].shape[1])))
    return out


# ---- the two-basin scene: a corridor along x with identical posts every POST_PERIOD metres --------------------------------
POST_PERIOD = 3.0
BASIN_B, BASIN_M, BASIN_P = 1024, 4096, 16
BASIN_OFFSET = 0.1                  # the source is a stretch of the same structure, displaced by this much along x
# K: stage A searches once, at the initial mean, so the candidates of a post point must reach the NEXT post (K = 256 does not:
# the second basin then drifts); iterations: three move both groups towards their basins and leave the margins wide
BASIN_K, BASIN_I, BASIN_LR, BASIN_MAX_DIST = 384, 3, 1.0, 1.0
BASIN_SPREAD = 0.2                  # the initial particles lie within +-BASIN_SPREAD of x = 0 and of x = POST_PERIOD
_TGT_X = (-30.0, 34.0)              # the target's stretch
_SRC_X = (-3.0, 3.0)                # the source's
_WALL_Y, _WALL_Z, _POST_Y = 1.0, 1.5, 0.6        # half-width, height; the posts reach from the walls in to +-_POST_Y


def _corridor(pkg, n, x_lo, x_hi, stream):
    """n points: half on the posts (flat pilasters at x = k * POST_PERIOD that reach from either wall in to y = +-_POST_Y), a quarter on the two walls, a
    quarter on the floor."""
    u = pkg.scans.uniform01(stream, 4 * n, seed=20251).reshape(4, n)
    pts = np.zeros((n, 3))
    n_post, n_wall = n // 2, n // 4
    k_lo, k_hi = int(np.ceil(x_lo / POST_PERIOD)), int(np.floor(x_hi / POST_PERIOD))
    posts = np.arange(k_lo, k_hi + 1) * POST_PERIOD
    i = np.arange(n_post)
    which = i % (2 * len(posts))                             # every post gets the same share
    side = np.where(which % 2 == 0, 1.0, -1.0)
    pts[:n_post, 0] = posts[which // 2]                      # thin in x: the face of a post is the plane x = k * POST_PERIOD
    pts[:n_post, 1] = side * (_POST_Y + (_WALL_Y - _POST_Y) * u[0, :n_post])
    pts[:n_post, 2] = _WALL_Z * u[1, :n_post]
    w = slice(n_post, n_post + n_wall)
    pts[w, 0] = x_lo + (x_hi - x_lo) * u[0, w]
    pts[w, 1] = np.where(u[2, w] < 0.5, _WALL_Y, -_WALL_Y)
    pts[w, 2] = _WALL_Z * u[1, w]
    f = slice(n_post + n_wall, n)
    pts[f, 0] = x_lo + (x_hi - x_lo) * u[0, f]
    pts[f, 1] = _WALL_Y * (2.0 * u[1, f] - 1.0)
    pts[f, 2] = 0.0
    return pts.astype(np.float32).astype(np.float64)


def two_basin(pkg):
    """(source [B, 3], target [M, 3], initial particles [6, P]): the correction that registers the source is x = BASIN_OFFSET,
    and x = BASIN_OFFSET + POST_PERIOD registers it just as well.  The first half of the particles starts around x = 0, the
    second around x = POST_PERIOD."""
    tgt = _corridor(pkg, BASIN_M, *_TGT_X, stream=7001)
    src = _corridor(pkg, BASIN_B, *_SRC_X, stream=7002)
    src[:, 0] -= BASIN_OFFSET
    src = src.astype(np.float32).astype(np.float64)
    u = pkg.scans.uniform01(7003, 6 * BASIN_P, seed=20251).reshape(6, BASIN_P)
    half = np.array([BASIN_SPREAD, 0.05, 0.02, 0.002, 0.002, 0.006]).reshape(6, 1)
    init = half * (2.0 * u - 1.0)
    init[0, BASIN_P // 2:] += POST_PERIOD
    return src, tgt, init


def margins(x, labels, link_trans=LINK_T, link_rot=LINK_R):
    """(inter, near) in units of the link, with s(p, q) = max(dt / link_trans, dr / link_rot) (p and q link iff s <= 1):
    inter = the smallest s over the pairs of different modes; near = the largest, over the particles, of the smallest s to
    another particle of its own mode."""
    x = np.asarray(x, np.float64).reshape(6, -1)
    d = x[:, :, None] - x[:, None, :]
    s = np.maximum(np.sqrt((d[:3] ** 2).sum(0)) / link_trans, np.sqrt((d[3:] ** 2).sum(0)) / link_rot)
    labels = np.asarray(labels)
    same = labels[:, None] == labels[None, :]
    own = same & ~np.eye(len(labels), dtype=bool)
    return float(s[~same].min()), float(np.where(own, s, np.inf).min(axis=1).max())


def two_basin_params(pkg):
    return pkg.SteinICPParam(iterations=BASIN_I, lr=BASIN_LR, max_dist=BASIN_MAX_DIST, KNN_count=BASIN_K, SVN_full_grad=False)
