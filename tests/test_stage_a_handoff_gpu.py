"""Stage A hands its result to stage B: the tile family's select kernel writes the split variant's search table itself
(option table = select, the default) instead of k_build_table3 gathering it again from cand_idx (table = gather), and it
stores no distances: svnicp_get_candidate_dist2 recomputes them on demand.  Both are re-placements
of the same arithmetic, so everything is compared bit for bit between the two options, and against the oracle as
tests/test_gpu_parity.py's _compare defines equality.

The tile kernels need 16 tiles of 512 targets: M = 8 192 + 37 gives a padded last tile.  B = 130 is two full groups of 64
queries, a group of 2, and a last k_build_table3 workgroup that is not full.  The hand-off applies to the split stage B,
which a shard of more than 8 particles gets (registration_plan.hpp: stage_b_variant), so every comparison runs with 12
particles; the 8 particles of the fused float32 stage B run too, where the option must change nothing.

Clouds at (4 300, 8 800, 0) m.  Poses rotate about the origin, so a rotation of 0.01 rad moves a cloud out there by 100 m:
the initial mean of the far case is a translation and the particles' rotations are scaled to 2.4e-6 rad (2.4 cm at that
lever arm), which keeps the clouds on each other; stage A alone is compared under the rotated mean as well, like
tests/test_knn_prefilter_gpu.py's test_far_from_the_origin.  Even so the reference's registration is not a stable function
of its input at that distance: cond(H) = 1.3e8, the first Stein step is 3.5e5 m long and the second bandwidth 1.6e8, and
the ORACLE run on the same clouds with the source rows in reverse order (another order of the same sums) ends with particles
1.9e-4 away from its own, against the 1e-9 of _compare (measured on the CPU; at the origin the same experiment gives
3e-16).  Past the first step, equality to the oracle within _compare's tolerances is therefore nothing an implementation
with its own summation order can have, and the entries of the first H already cancel from terms of 1e8 each to less than
their rtol = 1e-11 leaves room for.  The far case holds to the oracle what is defined: stage A bit for bit and the first
iteration's correspondences; select against gather stays bit for bit over the whole registration.
"""
import functools

import numpy as np
import pytest

import nonfinite_reference as nf
from helpers import TIGHT
from test_gpu_parity import _compare, _hip_solver

pytestmark = pytest.mark.gpu

M_, B_, I_ = 8192 + 37, 130, 3
R0_T0 = ((0.01, -0.02, 0.03), np.array([0.3, -0.2, 0.1]))
OFFSET = np.array([4300.0, 8800.0, 0.0])


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _mean(hip, far=False):
    return (np.eye(3), R0_T0[1] * 0.1) if far else (hip.scans.rot_zyx(*R0_T0[0]), R0_T0[1])


def _cfg(K):
    return dict(iterations=I_, lr=1.0, max_dist=1.0, knn_count=K, svn_full_grad=False)


@functools.lru_cache(maxsize=None)
def _clouds(hip, B, M, seed):
    return hip.scans.random_clouds(B, M, seed=seed, extent=40.0)


def _init(hip, P, far=False):
    init = hip.scans.make_particles(P, seed=P) * 0.2
    if far:
        init[3:] *= 1e-3
    return init


def _device(hip, src, tgt, P, K, table, opts=(), far=False):
    init = _init(hip, P, far)
    s = _hip_solver(hip, init, trace=True, **_cfg(K))
    s.add_cloud(src, tgt, init)
    s.set_initial_mean(_mean(hip, far))
    s.set_option("knn", "tiles")
    s.set_option("table", table)
    for k, v in opts:
        s.set_option(k, v)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    return s


def _oracle(orc, hip, src, tgt, P, K, far=False):
    init = _init(hip, P, far)
    o = orc.Solver(init, **_cfg(K))
    o.add_cloud(src, tgt, init)
    o.set_initial_mean(*_mean(hip, far))
    tro = o.enable_trace()
    o.stein_align()
    return o, tro


def _results(s):
    tr = s.get_trace()
    return dict(cand=s.get_candidates().astype(np.int64), d2=_bits(s.get_candidate_dist2()), corr=tr["corr"], H=_bits(tr["H"]), b=_bits(tr["b"]),
                particles=_bits(s.get_particles()), pose=_bits(s.get_transformation()), cov=_bits(s.get_cov_matrix()),
                var=_bits(s.get_distribution()))


def _same_bits(a, b):
    for key in a:
        assert np.array_equal(a[key], b[key]), f"table=select and table=gather differ in {key}"


def _both(hip, src, tgt, P, K, opts=(), far=False):
    sel, gat = _device(hip, src, tgt, P, K, "select", opts, far), _device(hip, src, tgt, P, K, "gather", opts, far)
    _same_bits(_results(sel), _results(gat))
    assert sel.get_knn_fallbacks() == gat.get_knn_fallbacks()
    return sel, gat


# ---------------------------------------------------------------- 1. the hand-off under both options, and the oracle
@pytest.mark.parametrize("far", [False, True], ids=["origin", "far"])
@pytest.mark.parametrize("K", [17, 100, 128])
@pytest.mark.parametrize("P", [12, 8])
def test_select_writes_the_table(hip, orc, P, K, far):
    src, tgt = _clouds(hip, B_, M_, 11)
    if far:
        src, tgt = src + OFFSET, tgt + OFFSET
    sel, gat = _both(hip, src, tgt, P, K, far=far)
    assert sel.get_knn_fallbacks() == 0
    o, tro = _oracle(orc, hip, src, tgt, P, K, far)
    if not far:
        _compare(sel, o, tro, P)
        _compare(gat, o, tro, P)
    else:        # what is defined out there (module docstring), then stage A and the options under the rotated mean too
        tr = sel.get_trace()
        assert np.array_equal(sel.get_candidates().astype(np.int64), o.candidates())
        assert np.array_equal(_bits(sel.get_candidate_dist2()), _bits(o.candidate_dist2()))
        assert np.array_equal(tr["corr"][0], tro["corr"][0])
        sel, gat = _both(hip, src, tgt, P, K)
        wi, wd = orc.knn_topk(orc.transform(src, *_mean(hip)), tgt, K)
        assert np.array_equal(sel.get_candidates().astype(np.int64), wi) and np.array_equal(_bits(sel.get_candidate_dist2()), _bits(wd))


# ---------------------------------------------------------------- 2. more than K entries kept: ties, ranks >= K
def _tied_clouds(hip, K):
    """Around chosen queries: K - 5 distinct nearer targets, then a block of exact duplicates (same coordinates, other
    indices) that straddles the K-th place — 12 of them (ranked path: at most 128 entries kept, several at ranks >= K), 150
    (more than 128 kept: the sorted path) or 700 (more than the 512 the select kernel sorts: the fallback kernels) — and
    near-ties 1e-7 m apart just behind them."""
    src, tgt = _clouds(hip, B_, M_, 23)
    src, tgt = src.copy(), tgt.copy()
    rng = np.random.default_rng(23)
    q = src @ _mean(hip)[0].T + _mean(hip)[1]
    free = rng.permutation(M_)
    at = 0
    for n, b in enumerate((0, 5, 63, 64, 100, 128, 129, 31, 77)):
        dups = (12, 150, 12, 150, 12, 700, 12, 150, 700)[n]
        d = rng.normal(size=(K + 8, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        rows = free[at:at + K - 5 + dups + 8]; at += rows.size
        tgt[rows[:K - 5]] = q[b] + d[:K - 5] * (0.02 + 0.001 * np.arange(K - 5))[:, None]
        tgt[rows[K - 5:K - 5 + dups]] = q[b] + d[K - 5] * 0.2
        tgt[rows[K - 5 + dups:]] = q[b] + d[K - 4:K + 4] * (0.2 + (1 + np.arange(8))[:, None] * 1e-7)
    return src, tgt


@pytest.mark.parametrize("K", [17, 100])
def test_ties_and_ranks_beyond_k(hip, orc, K):
    P = 12
    src, tgt = _tied_clouds(hip, K)
    q = orc.transform(src, *_mean(hip))
    wi, wd = orc.knn_topk(q, tgt, K)
    assert (np.diff(wd, axis=1) == 0).any(), "the case must hold exact ties"
    kept = (nf.dist2(q, tgt) <= wd[:, K - 1][:, None]).sum(axis=1)       # what any exact threshold keeps at least
    assert (kept > K).sum() >= 9 and (kept > 128).sum() >= 3
    assert (kept > 512).mean() < 0.10, "fewer than 10 % of the rows may need the fallback kernels"
    gat = _device(hip, src, tgt, P, K, "gather")
    o, tro = _oracle(orc, hip, src, tgt, P, K)
    _compare(gat, o, tro, P)                                               # the gather path alone passes
    sel = _device(hip, src, tgt, P, K, "select")
    print(f"RESULT handoff ties K={K} fallbacks={sel.get_knn_fallbacks()} of {B_}")
    assert sel.get_knn_fallbacks() == gat.get_knn_fallbacks() < 0.10 * B_
    _same_bits(_results(sel), _results(gat))
    _compare(sel, o, tro, P)


# ---------------------------------------------------------------- 3. rows the fallback kernels redo
@functools.lru_cache(maxsize=None)
def _duplicated(B):
    """tests/test_gpu_parity.py's test_stage_a_fallback_on_pool_overflow at the small size: 6 points, 1500 copies each."""
    rng = np.random.default_rng(3)
    centers = rng.normal(size=(6, 3)) * 5
    tgt = np.repeat(centers, 1500, axis=0).astype(np.float32).astype(np.float64)
    tgt = tgt[rng.permutation(tgt.shape[0])]
    src = centers[rng.integers(0, 6, B)] + rng.normal(size=(B, 3)) * 0.1
    return src, tgt


@pytest.mark.parametrize("sliced_max", [None, 16])
def test_fallback_rows(hip, orc, sliced_max):
    P, K = 12, 50
    src, tgt = _duplicated(B_)
    opts = () if sliced_max is None else (("fallback_sliced_max", sliced_max),)
    sel, gat = _both(hip, src, tgt, P, K, opts)
    assert sel.get_knn_fallbacks() == B_ > 0
    o, tro = _oracle(orc, hip, src, tgt, P, K)
    assert np.array_equal(sel.get_candidates().astype(np.int64), o.candidates())
    assert np.array_equal(_bits(sel.get_candidate_dist2()), _bits(o.candidate_dist2()))
    assert np.array_equal(sel.get_trace()["corr"], tro["corr"])


def test_fallback_rows_among_others(hip, orc):
    """Some rows through the fallback kernels, most through the select kernel: the list variant of k_build_table3 must
    rewrite exactly the listed rows."""
    P, K = 12, 17
    src, tgt = _tied_clouds(hip, K)
    sel, gat = _both(hip, src, tgt, P, K)
    assert 0 < sel.get_knn_fallbacks() < B_


# ---------------------------------------------------------------- 4. non-finite and huge points
def test_non_finite_and_huge_points(hip, orc):
    P, K = 12, 17
    src, tgt = _clouds(hip, B_, M_, 9)
    rows = [K, K + 1] + list(range(K + 37, M_, 500))
    bad_t = nf.poison(tgt, rows, nf.KINDS)
    # bad target rows are invisible: the oracle on the target without them, candidates through the index map
    sel, gat = _both(hip, src, bad_t, P, K)
    wi, wd = nf.knn_contract(orc.transform(src, *_mean(hip)), bad_t, K)
    assert np.array_equal(sel.get_candidates().astype(np.int64), wi) and np.array_equal(_bits(sel.get_candidate_dist2()), _bits(wd))
    clean, old_to_new = nf.remove_rows(bad_t, rows)
    o, tro = _oracle(orc, hip, src, clean, P, K)
    assert np.array_equal(old_to_new[sel.get_candidates().astype(np.int64)], o.candidates())
    assert np.array_equal(sel.get_trace()["corr"], tro["corr"])
    assert np.abs(sel.get_transformation() - o.get_transformation()).max() < TIGHT
    # huge source rows: the oracle on the same cloud is defined (+inf is a number)
    bad_s = nf.poison(src, [0, 21, 63, 64, 129], ("big32", "big64"))
    sel, gat = _both(hip, bad_s, tgt, P, K)
    o, tro = _oracle(orc, hip, bad_s, tgt, P, K)
    _compare(sel, o, tro, P)
    # every kind in both clouds: stage A against the stated contract, the registration between the options (NaN sums compare
    # as bits)
    bad_s = nf.poison(src, [0, 129, 21, 38, 68, 121], nf.KINDS)
    sel, gat = _both(hip, bad_s, bad_t, P, K)
    wi, wd = nf.knn_contract(orc.transform(bad_s, *_mean(hip)), bad_t, K)
    assert np.array_equal(sel.get_candidates().astype(np.int64), wi) and np.array_equal(_bits(sel.get_candidate_dist2()), _bits(wd))


# ---------------------------------------------------------------- 5. distances on demand
@pytest.mark.parametrize("case", ["plain", "far", "fallback"])
def test_distances_on_demand(hip, orc, case):
    P, K = 12, 50 if case == "fallback" else 100
    if case == "fallback":
        src, tgt = _duplicated(B_)
    else:
        src, tgt = _clouds(hip, B_, M_, 11)
        if case == "far":
            src, tgt = src + OFFSET, tgt + OFFSET
    sel = _device(hip, src, tgt, P, K, "select")
    want_i, want_d = orc.knn_topk(orc.transform(src, *_mean(hip)), tgt, K)
    first, second = sel.get_candidate_dist2(), sel.get_candidate_dist2()
    assert np.array_equal(sel.get_candidates().astype(np.int64), want_i)
    assert np.array_equal(_bits(first), _bits(want_d)) and np.array_equal(_bits(second), _bits(want_d))
    v1 = _device(hip, src, tgt, P, K, "select", (("knn", "v1"),))          # the streaming kernel stores its distances
    assert np.array_equal(_bits(v1.get_candidate_dist2()), _bits(first))
    # a second registration on the same context: other source rows, the particles where the first left them
    src2 = src[::-1] + 0.05
    sel.set_source(src2)
    assert sel.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    want_i, want_d = orc.knn_topk(orc.transform(src2, *_mean(hip)), tgt, K)
    assert np.array_equal(sel.get_candidates().astype(np.int64), want_i)
    assert np.array_equal(_bits(sel.get_candidate_dist2()), _bits(want_d))


# ---------------------------------------------------------------- 6. one sort chain for target and queries
@pytest.mark.parametrize("B", [130, 64])
def test_joint_sort(hip, orc, B):
    """sort = joint against sort = separate: the same Morton permutations, so the same groups, tiles, survivors and results;
    a second registration on the held target sorts its queries alone."""
    P, K = 12, 17
    src, tgt = _tied_clouds(hip, K)           # some rows through the fallback kernels
    src = src[:B]
    out = {}
    for sort in ("joint", "separate"):
        s = _device(hip, src, tgt, P, K, "select", (("sort", sort),))
        out[sort] = (_results(s), s.get_knn_survivors(), s.get_knn_fallbacks(), np.sort(s.get_knn_fallback_rows()))
        if sort == "joint":
            held = s
    (ra, na, fa, la), (rb, nb, fb, lb) = out["joint"], out["separate"]
    _same_bits(ra, rb)
    assert np.array_equal(na, nb) and fa == fb and np.array_equal(la, lb)
    wi, wd = orc.knn_topk(orc.transform(src, *_mean(hip)), tgt, K)
    assert np.array_equal(ra["cand"], wi) and np.array_equal(ra["d2"], _bits(wd))
    src2 = src[::-1] + 0.05                   # the target stays held: the separate path
    held.set_source(src2)
    assert held.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    wi, wd = orc.knn_topk(orc.transform(src2, *_mean(hip)), tgt, K)
    assert np.array_equal(held.get_candidates().astype(np.int64), wi) and np.array_equal(_bits(held.get_candidate_dist2()), _bits(wd))
