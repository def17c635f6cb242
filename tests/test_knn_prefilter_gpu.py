"""Stage A's tile scan with its pre-filter on the bf16 matrix pipe (option knn_prefilter = mfma)
against the float32 VALU loop (knn_prefilter = valu), the streaming kernel (knn = v1) and the oracle's float64 brute force.
Indices and d² are compared bit for bit; the pre-filter may only change how many survivors reach the select kernel.

The tile kernels take targets of 16 to 8192 tiles of 512 slots (stage_a_plan.hpp: knn_tiles_applicable), so M = 1 100 is
served by the streaming kernel whatever knn_prefilter says; that shape is kept and compared all the same, and the smallest
shape that reaches the scan kernel with a partly filled last tile, M = 7 780 = 15 x 512 + 100, stands beside it.
"""
import functools

import numpy as np
import pytest

import nonfinite_reference as nf

pytestmark = pytest.mark.gpu

R0_T0 = ((0.01, -0.02, 0.03), np.array([0.3, -0.2, 0.1]))


def _mean(hip):
    return hip.scans.rot_zyx(*R0_T0[0]), R0_T0[1]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _run(hip, src, tgt, K, knn, prefilter=None, trace=False, mean=True):
    init = np.zeros((6, 2)); init[0, 1] = 0.01
    prm = hip.SteinICPParam(iterations=1, lr=1.0, max_dist=1.0, KNN_count=K, SVN_full_grad=False, record_trace=trace)
    s = hip.SVNICP(prm, init)
    s.add_cloud(src, tgt, init)
    s.set_option("knn", knn)
    if prefilter is not None:
        s.set_option("knn_prefilter", prefilter)
    if mean:
        s.set_initial_mean(_mean(hip))
    s.stein_align()
    n = s.get_knn_survivors() if trace else None
    return s.get_candidates().astype(np.int64), s.get_candidate_dist2(), s.get_knn_fallbacks(), n


def _three_ways(hip, src, tgt, K, want_i, want_d, fallbacks=0, trace=False, mean=True):
    """tiles/mfma, tiles/valu and v1 against the expectation; returns the survivor counts of the two tile runs."""
    out = {}
    for name, knn, pre in (("mfma", "tiles", "mfma"), ("valu", "tiles", "valu"), ("v1", "v1", None)):
        ci, cd, fb, n = _run(hip, src, tgt, K, knn, pre, trace=trace and knn == "tiles", mean=mean)
        print(f"RESULT knn_prefilter case={name} B={src.shape[0]} M={tgt.shape[0]} K={K} fallbacks={fb}"
              + (f" survivors={int(n.sum())}" if n is not None else ""))
        assert np.array_equal(ci, want_i), f"{name}: indices, {(ci != want_i).any(axis=1).sum()} rows differ"
        assert np.array_equal(_bits(cd), _bits(want_d)), f"{name}: d² bits, {(_bits(cd) != _bits(want_d)).any(axis=1).sum()} rows differ"
        if knn == "tiles" and fallbacks is not None:
            assert fb == fallbacks, f"{name}: {fb} fallbacks"
        out[name] = n
    return out


@functools.lru_cache(maxsize=None)
def _clouds(hip, B, M, seed, extent=40.0):
    return hip.scans.random_clouds(B, M, seed=seed, extent=extent)


def _expect(hip, orc, src, tgt, K, mean=True):
    q = orc.transform(src, *_mean(hip)) if mean else src
    return q, orc.knn_topk(q, tgt, K)


# B = 130: two full groups of 64 queries and a group of 2
@pytest.mark.parametrize("K", [100, 1, 16, 128])
@pytest.mark.parametrize("M", [1100, 7780])
def test_partial_shapes(hip, orc, M, K):
    src, tgt = _clouds(hip, 130, M, 130 + M)
    _, (wi, wd) = _expect(hip, orc, src, tgt, K)
    tiles = M >= 7681
    _three_ways(hip, src, tgt, K, wi, wd, fallbacks=0 if tiles else -1)      # -1: the streaming kernel has no fallback count


def _cluster_target(rng):
    """16 clusters of exactly 512 points, 0.1 m across, on cells (i, j, k) of a 4 x 4 x 4 grid of 10 m: each cluster keeps
    its own 6-bit Morton prefix (the corner cells pin the box), so each tile is exactly one cluster."""
    cells = [(0, 0, 0), (3, 3, 3), (3, 0, 0), (0, 3, 0), (0, 0, 3), (1, 1, 1), (2, 1, 1), (1, 2, 1), (2, 2, 1), (1, 1, 2),
             (2, 1, 2), (1, 2, 2), (2, 2, 2), (3, 3, 0), (0, 3, 3), (3, 0, 3)]
    centres = np.array(cells, np.float64) * 10.0
    tgt = np.concatenate([c + rng.uniform(-0.05, 0.05, size=(512, 3)) for c in centres])
    return centres, tgt[rng.permutation(tgt.shape[0])]


def test_partial_last_batch(hip, orc):
    """One group of 64 queries: 17 of them sit in cluster A (two batches, the second with one column), exactly 1 in
    cluster B, 46 in cluster C (three batches, the last with 14 columns).  K = 8 keeps every threshold inside the query's
    own cluster, ten metres from the next, so a query is live in its own tile only: its survivors are at most 512."""
    rng = np.random.default_rng(17)
    centres, tgt = _cluster_target(rng)
    src = np.concatenate([centres[5] + rng.uniform(-0.04, 0.04, size=(17, 3)), centres[6] + rng.uniform(-0.04, 0.04, size=(1, 3)),
                          centres[7] + rng.uniform(-0.04, 0.04, size=(46, 3))])
    _, (wi, wd) = _expect(hip, orc, src, tgt, 8, mean=False)
    n = _three_ways(hip, src, tgt, 8, wi, wd, trace=True, mean=False)
    assert n["mfma"].max() <= 512 and n["mfma"].min() >= 8


def test_far_from_the_origin(hip, orc):
    """Both clouds at (4 300, 8 800, 0) m: one float32 ulp is 0.5 - 1 mm there; the bound is written in tile-local terms."""
    src, tgt = _clouds(hip, 130, 7780, 31)
    off = np.array([4300.0, 8800.0, 0.0])
    src, tgt = src + off, tgt + off
    _, (wi, wd) = _expect(hip, orc, src, tgt, 16)
    _three_ways(hip, src, tgt, 16, wi, wd)


def test_tile_with_an_outlier(hip, orc):
    """One target a kilometre from the rest: its tile's C_t is about 1000 m, EPS_t about 56 u C_t² = 3.3 m², more than the
    tile is wide — every slot of that tile survives for every query live in it, the result stays exact."""
    src, tgt = _clouds(hip, 130, 7780, 77)
    tgt = tgt.copy()
    tgt[4000] = tgt[4000] + np.array([1000.0, 0.0, 0.0])
    q, (wi, wd) = _expect(hip, orc, src, tgt, 16)
    n = _three_ways(hip, src, tgt, 16, wi, wd, trace=True)
    print(f"RESULT knn_prefilter outlier survivors mfma={int(n['mfma'].sum())} valu={int(n['valu'].sum())}")
    assert n["mfma"].sum() > n["valu"].sum(), "the outlier's tile must let more through"


def test_near_ties_around_the_kth_distance(hip, orc):
    """Targets on rays from a query at distances 1 m + j x 1e-7 m around the K-th neighbour, and exact duplicates of some
    of them: (d², index) decides."""
    K = 16
    src, tgt = _clouds(hip, 130, 7780, 5, extent=40.0)
    src, tgt = src.copy(), tgt.copy()
    rng = np.random.default_rng(5)
    for b in (0, 63, 64, 129):
        d = rng.normal(size=(24, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        rows = rng.choice(7780, 30, replace=False)
        tgt[rows[:24]] = src[b] + d * (1.0 + (np.arange(24) - 12)[:, None] * 1e-7)      # the 16th of them is a near-tie
        tgt[rows[24:]] = tgt[rows[10:16]]                                                 # exact duplicates, other indices
    _, (wi, wd) = _expect(hip, orc, src, tgt, K, mean=False)
    assert (np.diff(wd, axis=1) == 0).any(), "the case must hold exact ties"
    _three_ways(hip, src, tgt, K, wi, wd, mean=False)


@pytest.mark.parametrize("K", [50, 7])
def test_duplicates_overflow_the_pool(hip, orc, K):
    """tests/test_gpu_parity.py's clustered duplicates: 2000 targets at exactly the same distance overflow every query's
    pool; all 300 queries go through the fallback under either pre-filter."""
    rng = np.random.default_rng(3)
    centers = rng.normal(size=(6, 3)) * 5
    tgt = np.repeat(centers, 2000, axis=0).astype(np.float32).astype(np.float64)
    tgt = tgt[rng.permutation(tgt.shape[0])]
    src = centers[rng.integers(0, 6, 300)] + rng.normal(size=(300, 3)) * 0.1
    wi, wd = orc.knn_topk(src, tgt, K)
    _three_ways(hip, src, tgt, K, wi, wd, fallbacks=300, mean=False)


def test_non_finite_points_and_queries_outside_the_box(hip, orc):
    """NaN, inf and 1e20 / 3e38 / 1e160 rows in both clouds (tests/nonfinite_reference.py states the contract), and queries
    half a kilometre outside the target's box.  Fallback counts are whatever the thresholds give: not asserted."""
    K = 16
    src, tgt = _clouds(hip, 130, 7780, 9)
    src = src.copy()
    src[40:50] += np.array([500.0, -500.0, 500.0])
    bad_t = nf.poison(tgt, [K, K + 1] + list(range(K + 37, 7780, 500)), nf.KINDS)
    wi, wd = nf.knn_contract(orc.transform(src, *_mean(hip)), bad_t, K)
    _three_ways(hip, src, bad_t, K, wi, wd, fallbacks=None)
    bad_s = nf.poison(src, [0, 129, 21, 38, 68, 121], nf.KINDS)
    wi, wd = nf.knn_contract(orc.transform(bad_s, *_mean(hip)), tgt, K)
    _three_ways(hip, bad_s, tgt, K, wi, wd, fallbacks=None)
    wi, wd = nf.knn_contract(orc.transform(bad_s, *_mean(hip)), bad_t, K)
    _three_ways(hip, bad_s, bad_t, K, wi, wd, fallbacks=None)


@pytest.mark.parametrize("K,offset", [(16, 0.0), (100, 0.0), (16, 4300.0)])
def test_survivors_are_a_superset(hip, orc, K, offset):
    """For every query the survivors of the matrix-pipe pre-filter are at least the targets whose exact d² is at most the
    K-th distance: none of those may be lost, whatever the filter's rounding."""
    src, tgt = _clouds(hip, 130, 7780, 130 + 7780)
    src, tgt = src + offset, tgt + offset
    q, (wi, wd) = _expect(hip, orc, src, tgt, K)
    n = _three_ways(hip, src, tgt, K, wi, wd, trace=True)
    need = (nf.dist2(q, tgt) <= wd[:, K - 1][:, None]).sum(axis=1)
    assert need.min() >= K
    for name in ("mfma", "valu"):
        short = np.flatnonzero(n[name] < need)
        assert short.size == 0, f"{name}: queries {short[:10]} hold {n[name][short[:10]]} survivors, {need[short[:10]]} needed"
