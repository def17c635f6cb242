"""The seed kernel's bounded tile ranking (option seed_rank = bounded) against the full ranking of
every tile of a visited 64-tile group (seed_rank = full).  A tile that is not scored could not have entered any query's
top-4 list, so the picks are the same set and everything downstream keeps its bits: candidates, d², fallback rows and the
per-query survivor counts of the pre-filter (identical picks give identical thresholds) are compared for equality, and the
indices against the float64 brute force as well.

B = 130 queries throughout: two full groups of 64 and a group of 2.
"""
import functools
import re

import numpy as np
import pytest

import nonfinite_reference as nf

pytestmark = pytest.mark.gpu

R0_T0 = ((0.01, -0.02, 0.03), np.array([0.3, -0.2, 0.1]))
B = 130


def _mean(hip):
    return hip.scans.rot_zyx(*R0_T0[0]), R0_T0[1]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _run(hip, src, tgt, K, rank, mean=True, debug=False):
    init = np.zeros((6, 2)); init[0, 1] = 0.01
    prm = hip.SteinICPParam(iterations=1, lr=1.0, max_dist=1.0, KNN_count=K, SVN_full_grad=False, record_trace=True)
    s = hip.SVNICP(prm, init)
    s.add_cloud(src, tgt, init)
    s.set_option("knn", "tiles")
    s.set_option("seed_rank", rank)
    if debug:
        s.set_option("debug", "1")
    if mean:
        s.set_initial_mean(_mean(hip))
    s.stein_align()
    return s.get_candidates().astype(np.int64), s.get_candidate_dist2(), s.get_knn_fallbacks(), s.get_knn_survivors()


def _both(hip, src, tgt, K, want_i=None, want_d=None, mean=True):
    """bounded against full: everything equal; and both against the expectation where one is given."""
    bi, bd, bf, bn = _run(hip, src, tgt, K, "bounded", mean=mean)
    fi, fd, ff, fn = _run(hip, src, tgt, K, "full", mean=mean)
    print(f"RESULT seed_rank B={src.shape[0]} M={tgt.shape[0]} K={K} fallbacks bounded={bf} full={ff} "
          f"survivors bounded={int(bn.sum())} full={int(fn.sum())}")
    assert np.array_equal(bi, fi), f"indices: {(bi != fi).any(axis=1).sum()} rows differ"
    assert np.array_equal(_bits(bd), _bits(fd)), f"d² bits: {(_bits(bd) != _bits(fd)).any(axis=1).sum()} rows differ"
    assert bf == ff, f"fallbacks: bounded {bf}, full {ff}"
    assert np.array_equal(bn, fn), f"survivor counts: {(bn != fn).sum()} queries differ"
    if want_i is not None:
        assert np.array_equal(bi, want_i), f"indices against the reference: {(bi != want_i).any(axis=1).sum()} rows differ"
        assert np.array_equal(_bits(bd), _bits(want_d)), "d² bits against the reference"
    return bf, bn


@functools.lru_cache(maxsize=None)
def _clouds(hip, M, seed, extent=40.0):
    return hip.scans.random_clouds(B, M, seed=seed, extent=extent)


def _expect(hip, orc, src, tgt, K, mean=True):
    q = orc.transform(src, *_mean(hip)) if mean else src
    return orc.knn_topk(q, tgt, K)


# 16 tiles: the smallest target the tile family takes, with a partly filled last tile.  66 tiles: a second outer group of
# 2 tiles.  521 tiles: more than 8 outer groups, so the group boxes are folded by fewer than 8 lanes per group.
@pytest.mark.parametrize("M,K", [(7780, 16), (7780, 100), (33380, 16), (266240 + 100, 16)])
def test_random_shapes(hip, orc, M, K):
    src, tgt = _clouds(hip, M, 130 + M)
    wi, wd = _expect(hip, orc, src, tgt, K)
    fb, _ = _both(hip, src, tgt, K, wi, wd)
    assert fb == 0


def _cluster_target(rng):
    """16 clusters of exactly 512 points, 0.1 m across, on cells of a 4 x 4 x 4 grid of 10 m; the corner cells pin the box,
    every cluster keeps a 6-bit Morton prefix of its own, so every tile is exactly one cluster."""
    cells = [(0, 0, 0), (3, 3, 3), (3, 0, 0), (0, 3, 0), (0, 0, 3), (1, 1, 1), (2, 1, 1), (1, 2, 1), (2, 2, 1), (1, 1, 2),
             (2, 1, 2), (1, 2, 2), (2, 2, 2), (3, 3, 0), (0, 3, 3), (3, 0, 3)]
    centres = np.array(cells, np.float64) * 10.0
    tgt = np.concatenate([c + rng.uniform(-0.05, 0.05, size=(512, 3)) for c in centres])
    return centres, tgt[rng.permutation(tgt.shape[0])]


def test_all_queries_inside_one_cluster(hip, orc):
    """Every query of every group sits in one cluster's box: that tile's bound is 0 for all of them, and so is the wave-wide
    bound of every tile whose box the wave's box touches; the centre term of the score decides between them."""
    rng = np.random.default_rng(23)
    centres, tgt = _cluster_target(rng)
    src = centres[8] + rng.uniform(-0.04, 0.04, size=(B, 3))
    wi, wd = _expect(hip, orc, src, tgt, 8, mean=False)
    fb, _ = _both(hip, src, tgt, 8, wi, wd, mean=False)
    assert fb == 0


def test_queries_split_over_three_clusters(hip, orc):
    """50 / 50 / 30 queries in three clusters: along the curve the first group of 64 holds two clusters' queries, the second
    two as well, so the wave's box spans ten metres and holds whole tiles."""
    rng = np.random.default_rng(29)
    centres, tgt = _cluster_target(rng)
    src = np.concatenate([centres[c] + rng.uniform(-0.04, 0.04, size=(n, 3)) for c, n in ((5, 50), (12, 50), (3, 30))])
    src = src[rng.permutation(B)]
    wi, wd = _expect(hip, orc, src, tgt, 8, mean=False)
    fb, _ = _both(hip, src, tgt, 8, wi, wd, mean=False)
    assert fb == 0


def test_non_finite_rows_and_queries_outside_the_box(hip, orc):
    """NaN, infinite and huge rows in both clouds (tests/nonfinite_reference.py states the contract) and queries half a
    kilometre outside the target's box.  Fallback counts are whatever the thresholds give; the two rankings must agree."""
    K = 16
    src, tgt = _clouds(hip, 7780, 9)
    src = src.copy()
    src[40:50] += np.array([500.0, -500.0, 500.0])
    bad_t = nf.poison(tgt, [K, K + 1] + list(range(K + 37, 7780, 500)), nf.KINDS)
    bad_s = nf.poison(src, [0, 129, 21, 38, 68, 121], nf.KINDS)
    for s_, t_ in ((src, bad_t), (bad_s, tgt), (bad_s, bad_t)):
        wi, wd = nf.knn_contract(orc.transform(s_, *_mean(hip)), t_, K)
        _both(hip, s_, t_, K, wi, wd)


def test_fewer_than_four_finite_tiles(hip, orc):
    """13 x 512 all-NaN target rows: they share Morton key 0 and fill the first 13 tiles, whose boxes stay empty, and three
    tiles hold the 1 124 finite points.  No query's list of four fills, the largest fourth-best score stays +inf, and the
    bounded ranking may skip nothing."""
    K = 16
    src, tgt = _clouds(hip, 7780, 41)
    rng = np.random.default_rng(41)
    bad = nf.poison(tgt, rng.choice(7780, 13 * 512, replace=False), "nan3")
    wi, wd = nf.knn_contract(orc.transform(src, *_mean(hip)), bad, K)
    _both(hip, src, bad, K, wi, wd)


def test_bounded_scores_no_more_tiles(hip, capfd):
    """Option debug prints the tiles scored in the rank phase; on the 66-tile shape the bounded run scores no more than the
    full run (which scores 64 or 2 per visited group)."""
    src, tgt = _clouds(hip, 33380, 130 + 33380)
    count = {}
    for rank in ("bounded", "full"):
        capfd.readouterr()
        _run(hip, src, tgt, 16, rank, debug=True)
        err = capfd.readouterr().err
        m = re.findall(r"rank tiles scored (\d+)", err)
        assert m, f"no rank count in the debug output of seed_rank = {rank}"
        count[rank] = int(m[0])   # the first search is stage A's
    print(f"RESULT seed_rank tiles scored in the rank phase, 3 groups of queries, 66 tiles: bounded={count['bounded']} full={count['full']}")
    assert 0 < count["bounded"] <= count["full"]
