"""Non-finite and huge cloud points through stage A, the per-iteration search and both residuals (include/svnicp_hip.h
"non-finite and huge points").  The reference is tests/nonfinite_reference.py — the contract in plain
float64 numpy — and the oracle wherever the oracle is well defined (tests/test_nonfinite_cpu.py pins where that is).
Candidates, d², correspondences and NaN patterns are held to equality; everything else reuses the tolerances of
tests/test_gpu_parity.py (_compare, the zero-bandwidth test), tests/test_minibatch_gpu.py and tests/test_plane_gpu.py."""
import functools

import numpy as np
import pytest

import nonfinite_reference as nf
import plane_reference as pr
from helpers import TIGHT

pytestmark = pytest.mark.gpu


def _scans():
    import __graft_entry__ as graft
    return graft.load_package().scans


def _mean():
    return _scans().rot_zyx(0.01, -0.02, 0.03), np.array([0.3, -0.2, 0.1])      # non-identity, every entry of R0 non-zero


def _hip_solver(pkg, init, trace=True, **cfg):
    prm = pkg.SteinICPParam(iterations=cfg["iterations"], lr=cfg["lr"], max_dist=cfg["max_dist"],
                            check_early_stop=cfg.get("check_early_stop", False),
                            convergence_threshold=cfg.get("convergence_threshold", 1e-5), KNN_count=cfg["knn_count"],
                            SVN_full_grad=cfg.get("svn_full_grad", False), optimizer=cfg.get("optimizer", "Adam"), record_trace=trace)
    return (pkg.SVGDICP if cfg.get("svgd") else pkg.SVNICP)(prm, init)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# =====================================================================================================================
# 1. stage A, every kernel
# =====================================================================================================================
# (variant, B, M, K, options): the smallest shapes each kernel takes
STAGE_A = ([("brute", 67, 1025, K, (("brute_qb", qb),)) for K in (1, 16, 128) for qb in (1, 6)]
           + [("tiles", 600, 8192, K, ()) for K in (7, 128)]
           + [(v, 300, 9000, K, ()) for v in ("v1", "v2") for K in (7, 150)])       # K = 150: the K > 128 path
STAGE_A_IDS = [f"{v}-K{K}" + "".join(f"-{k}{x}" for k, x in o) for v, B, M, K, o in STAGE_A]
TARGET_PATTERNS = ("scattered", "first_k", "run64", "tail", "few", "none")
QUERY_PATTERNS = ("single", "run64", "all")


@functools.lru_cache(maxsize=None)
def _stage_a_clouds(B, M):
    src, tgt = _scans().random_clouds(B, M, seed=B + M, extent=40.0)
    return src, tgt


def _poison_target(tgt, pattern, K):
    M = tgt.shape[0]
    if pattern == "scattered":                     # every kind, behind the first K
        rows = [K, K + 1] + list(range(K + 37, M, max(1, (M - K - 37) // 16)))
        return nf.poison(tgt, rows, nf.KINDS)
    if pattern == "first_k":                       # index 0 (a NaN: the oracle's heap would stall on it) and inside the first K
        return nf.poison(tgt, range(6), nf.KINDS)
    if pattern == "run64":
        return nf.poison(tgt, range(200, 264), nf.KINDS)
    if pattern == "tail":                          # next to the kernels' own NaN padding
        return nf.poison(tgt, range(M - 7, M), nf.KINDS)
    if pattern == "few":                           # five eligible targets
        keep = [3, 100, M // 2, M - 2, M - 1]
        return nf.poison(tgt, [r for r in range(M) if r not in keep], "nan3")
    if pattern == "none":
        return nf.poison(tgt, range(M), ("nan3", "nan1"))
    raise ValueError(pattern)


def _poison_queries(src, pattern, rot=0):
    B = src.shape[0]
    if pattern == "single":                        # one row of each kind: row 0, the last row, mid-wave
        rows = [0, B - 1, 21, 38, B // 2 + 3, B - 9]
        return nf.poison(src, rows, nf.KINDS[rot:] + nf.KINDS[:rot]), rows
    if pattern == "run64":                         # a whole wave / tile of bad rows
        rows = list(range(2, 66))
        return nf.poison(src, rows, nf.KINDS), rows
    if pattern == "all":
        return nf.poison(src, range(B), nf.KINDS), list(range(B))
    raise ValueError(pattern)


def _run_stage_a(hip, src, tgt, K, variant, opts):
    init = np.zeros((6, 2)); init[0, 1] = 0.01
    s = _hip_solver(hip, init, trace=False, iterations=1, lr=1.0, max_dist=1.0, knn_count=K, svn_full_grad=False)
    s.add_cloud(src, tgt, init)
    s.set_option("knn", variant)
    for k, v in opts:
        s.set_option(k, v)
    s.set_initial_mean(_mean())
    s.stein_align()
    fb = s.get_knn_fallbacks()
    assert -1 <= fb <= src.shape[0], "not a count"
    return s.get_candidates().astype(np.int64), s.get_candidate_dist2(), fb


_CLEAN = {}


def _clean_stage_a(hip, orc, variant, B, M, K, opts):
    """The device's rows on the clean clouds (once per configuration), themselves held to the contract."""
    key = (variant, B, M, K, opts)
    if key not in _CLEAN:
        src, tgt = _stage_a_clouds(B, M)
        ci, cd, _ = _run_stage_a(hip, src, tgt, K, variant, opts)
        wi, wd = nf.knn_contract(orc.transform(src, *_mean()), tgt, K)
        assert np.array_equal(ci, wi) and np.array_equal(_bits(cd), _bits(wd)), "clean clouds"
        _CLEAN[key] = (ci, cd)
    return _CLEAN[key]


@pytest.mark.parametrize("pattern", TARGET_PATTERNS)
@pytest.mark.parametrize("variant,B,M,K,opts", STAGE_A, ids=STAGE_A_IDS)
def test_stage_a_bad_target_rows(hip, orc, variant, B, M, K, opts, pattern):
    """Targets whose d² is NaN are never neighbours, +inf is a number, ties by index, zero padding past the eligible rows."""
    src, tgt = _stage_a_clouds(B, M)
    bad = _poison_target(tgt, pattern, K)
    ci, cd, fb = _run_stage_a(hip, src, bad, K, variant, opts)
    print(f"RESULT stage_a variant={variant} K={K} opts={dict(opts)} target={pattern} fallbacks={fb}")
    wi, wd = nf.knn_contract(orc.transform(src, *_mean()), bad, K)
    assert np.array_equal(ci, wi), f"indices: {(ci != wi).any(axis=1).sum()} rows differ"
    assert np.array_equal(_bits(cd), _bits(wd)), f"d² bits: {(_bits(cd) != _bits(wd)).any(axis=1).sum()} rows differ"
    if pattern in ("scattered", "run64", "tail"):          # … where the oracle is defined it says the same
        oi, od = orc.knn_topk(orc.transform(src, *_mean()), bad, K)
        assert np.array_equal(ci, oi) and np.array_equal(_bits(cd), _bits(od))


@pytest.mark.parametrize("pattern", QUERY_PATTERNS)
@pytest.mark.parametrize("variant,B,M,K,opts", STAGE_A, ids=STAGE_A_IDS)
def test_stage_a_bad_query_rows(hip, orc, variant, B, M, K, opts, pattern):
    """A row's result depends on that row and the target only: the finite rows equal the same kernel's rows on the clean
    source (a difference there is a leak), the bad rows follow the contract."""
    src, tgt = _stage_a_clouds(B, M)
    clean_i, clean_d = _clean_stage_a(hip, orc, variant, B, M, K, opts)
    for rot in range(len(nf.KINDS) if pattern == "single" else 1):
        bad, rows = _poison_queries(src, pattern, rot)
        ci, cd, fb = _run_stage_a(hip, bad, tgt, K, variant, opts)
        print(f"RESULT stage_a variant={variant} K={K} opts={dict(opts)} query={pattern}/{rot} fallbacks={fb}")
        ok = np.ones(B, bool); ok[rows] = False
        leak = (ci[ok] != clean_i[ok]).any(axis=1) | (_bits(cd[ok]) != _bits(clean_d[ok])).any(axis=1)
        assert not leak.any(), f"leak into finite rows {np.flatnonzero(ok)[leak][:10]} (rotation {rot})"
        wi, wd = nf.knn_contract(orc.transform(bad[rows], *_mean()), tgt, K)
        wrong = (ci[rows] != wi).any(axis=1) | (_bits(cd[rows]) != _bits(wd)).any(axis=1)
        assert not wrong.any(), f"bad rows {np.asarray(rows)[wrong][:10]} (rotation {rot})"


@pytest.mark.parametrize("sliced_max", [None, "0"])
def test_stage_a_fallback_regimes_with_bad_rows(hip, orc, sliced_max):
    """The duplicated target of test_stage_a_fallback_on_pool_overflow — every query overflows its pool and is redone by the
    streaming fallback, target-sliced or one wave per two queries — with poisoned rows added to both clouds."""
    rng = np.random.default_rng(3)
    K = 50
    centers = rng.normal(size=(6, 3)) * 5
    tgt = np.repeat(centers, 2000, axis=0).astype(np.float32).astype(np.float64)
    tgt = tgt[rng.permutation(tgt.shape[0])]
    M = tgt.shape[0]
    tgt = nf.poison(tgt, list(range(6)) + list(range(K + 3, M, 701)) + list(range(M - 7, M)), nf.KINDS)
    src = centers[rng.integers(0, 6, 300)] + rng.normal(size=(300, 3)) * 0.1
    bad, rows = _poison_queries(src, "single")
    opts = (("fallback_sliced_max", sliced_max),) if sliced_max is not None else ()
    ai, ad, fa = _run_stage_a(hip, src, tgt, K, "tiles", opts)
    bi, bd, fb = _run_stage_a(hip, bad, tgt, K, "tiles", opts)
    print(f"RESULT stage_a variant=tiles-duplicates sliced_max={sliced_max} fallbacks clean-source={fa} bad-source={fb}")
    wi, wd = nf.knn_contract(orc.transform(src, *_mean()), tgt, K)
    assert np.array_equal(ai, wi) and np.array_equal(_bits(ad), _bits(wd))
    ok = np.ones(300, bool); ok[rows] = False
    assert np.array_equal(bi[ok], ai[ok]) and np.array_equal(_bits(bd[ok]), _bits(ad[ok])), "leak into finite rows"
    wi, wd = nf.knn_contract(orc.transform(bad[rows], *_mean()), tgt, K)
    assert np.array_equal(bi[rows], wi) and np.array_equal(_bits(bd[rows]), _bits(wd))


# =====================================================================================================================
# 2. the solver: the grid of stage-B plans
# =====================================================================================================================
I_, M_, K_ = 4, 8192, 32
GRID = ([(P, (("accum", a),), False, False) for P in (1, 4, 9, 64, 130) for a in ("split", "valu", "f64")]
        + [(P, (("chain", "general"),), False, False) for P in (1, 4, 9, 64, 130)]
        + [(1, (("single", "fused"),), False, False), (1, (("single", "split"),), False, False)]
        + [(9, (), True, False),            # svn_full_grad
           (9, (), False, True)])           # SVGD / Adam
GRID_IDS = [f"P{P}" + "".join(f"-{k}={v}" for k, v in o) + ("-fullgrad" if full else "") + ("-svgd" if svgd else "")
            for P, o, full, svgd in GRID]


def _cfg(full, svgd, **over):
    c = dict(iterations=I_, lr=0.01 if svgd else (0.5 if full else 1.0), max_dist=1.0, check_early_stop=True,
             convergence_threshold=1e-5, knn_count=K_, svn_full_grad=full)
    c.update(over)
    return c


@functools.lru_cache(maxsize=None)
def _solver_clouds(B):
    return _scans().random_clouds(B, M_, seed=B + 5)


def _init(P):
    return _scans().make_particles(P, seed=P) * 0.3


def _oracle(orc, src, tgt, P, full, svgd):
    cfg = _cfg(full, svgd)
    init = _init(P)
    o = orc.Solver(init, mode=orc.MODE_SVGD, optimizer="Adam", **cfg) if svgd else orc.Solver(init, **cfg)
    o.add_cloud(src, tgt, init); o.set_initial_mean(*_mean())
    tro = o.enable_trace()
    o.stein_align()
    return o, tro


def _device(hip, src, tgt, P, opts, full, svgd, entry="align"):
    init = _init(P)
    s = _hip_solver(hip, init, svgd=svgd, **_cfg(full, svgd))
    for k, v in opts:
        s.set_option(k, v)
    s.add_cloud(src, tgt, init); s.set_initial_mean(_mean())
    if entry == "align":
        assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    else:
        s.stein_align_async(); s.synchronize()
    return s


def _compare_after_stage_a(s, o, tro, P, svgd):
    """tests/test_gpu_parity.py's _compare without its two stage-A lines (the callers compare those through an index map),
    same tolerances; in SVGD mode what test_hip_svgd_reproduces_golden_and_oracle holds against the oracle."""
    n = o.iterations_run()
    tr = s.get_trace()
    assert s.get_iterations_run() == n
    assert int(s.get_runtime()[2]) == o.finish_iter()
    assert np.array_equal(tr["corr"][:n], tro["corr"][:n]), "per-iteration correspondence positions"
    if svgd:
        assert np.allclose(s.get_particles(), o.get_particles(), rtol=0, atol=TIGHT)
        return
    assert np.allclose(tr["H"][:n], tro["H"][:n], rtol=1e-11, atol=1e-9)
    assert np.allclose(tr["b"][:n], tro["b"][:n], rtol=1e-9, atol=1e-9)
    assert np.allclose(tr["newton"][:n], tro["newton"][:n], rtol=1e-7, atol=1e-10)
    assert np.allclose(tr["phi"][:n], tro["phi"][:n], rtol=1e-7, atol=1e-10)
    if P > 1:
        assert np.allclose(tr["h"][:n], tro["h"][:n], rtol=1e-10)
    assert np.abs(s.get_transformation() - o.get_transformation()).max() < TIGHT
    assert np.allclose(s.get_distribution(), o.get_distribution(), atol=TIGHT)
    assert np.allclose(s.get_cov_matrix(), o.get_cov_matrix(), atol=TIGHT)
    assert np.allclose(s.get_particles(), o.get_particles(), atol=TIGHT)
    assert np.array_equal(s.get_particle_weight(), o.get_particle_weight())
    assert np.allclose(s.get_particle_history(), o.get_particle_history(), atol=1e-6)


def _compare_with_nans(s, o, tro, P, svgd):
    """As test_two_particles_zero_bandwidth_goes_nan_like_the_reference compares: NaN patterns of b, phi and the particles
    equal to the oracle's, values close where they are numbers; H has no NaN where the oracle has a number, and where the
    oracle's H is NaN every entry fed by a sum is."""
    tr = s.get_trace()
    part, opart = s.get_particles(), o.get_particles()
    assert np.array_equal(np.isnan(part), np.isnan(opart)), "NaN pattern of the particles"
    assert np.allclose(part, opart, equal_nan=True)
    if svgd:
        return
    for key in ("b", "phi"):
        assert np.array_equal(np.isnan(tr[key]), np.isnan(tro[key])), key
        assert np.allclose(tr[key], tro[key], rtol=1e-9, atol=1e-9, equal_nan=True), key
    hn, on = np.isnan(tr["H"]), np.isnan(tro["H"])
    assert not (hn & ~on).any()
    nan_step = on.all(axis=2)                                    # [I, P]
    assert hn[:, :, 0][nan_step].all()
    assert np.allclose(tr["H"][~nan_step], tro["H"][~nan_step], rtol=1e-11, atol=1e-9)


_ORACLE = {}


def _bad_target():
    rng = np.random.default_rng(8)
    rows = np.sort(rng.choice(np.arange(K_, M_), 78, replace=False)).tolist()
    head = [0, 1, 2, 3, 5, 7, 11, 30]             # inside the first K: every kind, a NaN at index 0
    src, tgt = _solver_clouds(512)
    bad = nf.poison(nf.poison(tgt, rows, nf.KINDS), head, ("nan1", "+inf", "big32", "nan3", "-inf", "big64"))
    return bad, head + rows


@pytest.mark.parametrize("P,opts,full,svgd", GRID, ids=GRID_IDS)
def test_bad_target_rows_are_invisible(hip, orc, P, opts, full, svgd):
    """1 % of the target rows bad, every kind, at indices >= K and inside the first K: the registration is the one on the
    target without those rows — candidates through the index map, d² bits, correspondences; sums, steps and poses within
    _compare's tolerances of the ORACLE on the cleaned target (tile partitions differ, so the sums are not bit-equal)."""
    src, _ = _solver_clouds(512)
    bad, rows = _bad_target()
    clean, old_to_new = nf.remove_rows(bad, rows)
    key = (P, full, svgd)
    if key not in _ORACLE:
        _ORACLE[key] = _oracle(orc, src, clean, P, full, svgd)
    o, tro = _ORACLE[key]
    a = _device(hip, src, bad, P, opts, full, svgd)
    b = _device(hip, src, clean, P, opts, full, svgd)
    ca = a.get_candidates().astype(np.int64)
    assert (old_to_new[ca] >= 0).all(), "a bad target row is a candidate"
    assert np.array_equal(old_to_new[ca], b.get_candidates().astype(np.int64))
    assert np.array_equal(old_to_new[ca], o.candidates())
    assert np.array_equal(_bits(a.get_candidate_dist2()), _bits(b.get_candidate_dist2()))
    assert np.array_equal(_bits(a.get_candidate_dist2()), _bits(o.candidate_dist2()))
    assert np.array_equal(a.get_trace()["corr"], b.get_trace()["corr"])
    _compare_after_stage_a(a, o, tro, P, svgd)
    _compare_after_stage_a(b, o, tro, P, svgd)


SOURCE_CLOUDS = {"huge": ("big32", "big64"), "inf": ("+inf", "-inf"), "nan1": ("nan1",), "nan3": ("nan3",)}
BAD_SOURCE_ROWS = [0, 17, 63, 64, 150, 299]


@pytest.mark.parametrize("cloud", list(SOURCE_CLOUDS))
@pytest.mark.parametrize("P,opts,full,svgd", GRID, ids=GRID_IDS)
def test_bad_source_rows_follow_the_reference(hip, orc, P, opts, full, svgd, cloud):
    """The mask is a multiplication, as in the reference: huge rows are masked to zero and everything stays finite (the
    oracle on the SAME cloud is the reference — a masked row still adds the identity block); a NaN or infinite row makes
    the sums it enters NaN for every particle, the early-stop flag never fires and the loop ends after I iterations."""
    src, tgt = _solver_clouds(300)
    bad = nf.poison(src, BAD_SOURCE_ROWS, SOURCE_CLOUDS[cloud])
    o, tro = _oracle(orc, bad, tgt, P, full, svgd)
    s = _device(hip, bad, tgt, P, opts, full, svgd)
    tr = s.get_trace()
    cand, d2 = s.get_candidates().astype(np.int64), s.get_candidate_dist2()
    if cloud in ("huge", "inf"):                    # the oracle's stage A is defined: +inf is a number
        assert np.array_equal(cand, o.candidates()) and np.array_equal(_bits(d2), _bits(o.candidate_dist2()))
    else:                                           # a NaN query has no eligible target: zero padding
        ok = np.isfinite(bad).all(axis=1)
        assert np.array_equal(cand[ok], o.candidates()[ok]) and np.array_equal(_bits(d2[ok]), _bits(o.candidate_dist2()[ok]))
        assert not cand[~ok].any() and not _bits(d2[~ok]).any()
    if cloud == "huge":
        assert np.isfinite(o.get_particles()).all() and np.isfinite(tro["H"]).all()
        _compare_after_stage_a(s, o, tro, P, svgd)
        for key in ("b", "phi"):
            assert not np.isnan(tr[key]).any(), key
        amb = s.get_ambiguous_pairs()
        print(f"RESULT search cloud=huge P={P} opts={dict(opts)} ambiguous_pairs={amb}")
        if amb >= 0:                                # the bf16 search ran: a big32 row must take the exact pass
            assert amb >= (len(BAD_SOURCE_ROWS) // 2) * P
        return
    assert s.get_iterations_run() == I_ == o.iterations_run()
    assert np.array_equal(tr["corr"], tro["corr"])
    if cloud != "inf":
        assert not tr["corr"][:, :, BAD_SOURCE_ROWS].any()         # a NaN first distance is never replaced
    assert np.isnan(o.get_particles()).any(), "0 · inf and 0 · NaN: these rows poison the oracle's sums"
    _compare_with_nans(s, o, tro, P, svgd)
    b = _device(hip, bad, tgt, P, opts, full, svgd, entry="async")
    assert b.get_iterations_run() == I_
    assert np.array_equal(np.isnan(b.get_particles()), np.isnan(s.get_particles()))
    assert np.allclose(b.get_particles(), s.get_particles(), rtol=0, atol=0, equal_nan=True)


def test_huge_source_rows_raise_the_ambiguous_pair_count(hip):
    """The default search at P = 64 is the bf16 matrix-pipe kernel: every (big32 row, particle) pair goes to its exact pass."""
    src, tgt = _solver_clouds(300)
    bad = nf.poison(src, BAD_SOURCE_ROWS, "big32")
    counts = []
    for cloud in (src, bad):
        s = _device(hip, cloud, tgt, 64, (), False, False)
        counts.append(s.get_ambiguous_pairs())
    print(f"RESULT search big32 P=64 ambiguous_pairs clean={counts[0]} bad={counts[1]}")
    assert counts[0] >= 0, "P = 64 no longer runs the bf16 search: pick a configuration that does"
    assert counts[1] >= len(BAD_SOURCE_ROWS) * 64


# =====================================================================================================================
# 3. mini-batch
# =====================================================================================================================
def _chain(orc, cfg, src, tgt, idx, init):
    """tests/test_minibatch_gpu.py's chained oracle: one full-batch iteration per table row."""
    p = np.array(init, np.float64)
    o = None
    for i in range(idx.shape[0]):
        o = orc.Solver(p, **dict(cfg, iterations=1))
        o.add_cloud(src[idx[i]], tgt, p)
        o.stein_align()
        p = o.get_particles().reshape(6, -1)
    return o


def test_minibatch_draws_decide_whether_a_nan_row_counts(hip, orc):
    P, B, M, K, I, batch = 8, 300, 2000, 16, 3, 64
    src, tgt = _scans().random_clouds(B, M, seed=31)
    src = nf.poison(src, [17], "nan3")
    init = _scans().make_particles(P, seed=P) * 0.3
    cfg = dict(iterations=I, lr=1.0, max_dist=1.0, knn_count=K, svn_full_grad=False)
    rng = np.random.default_rng(4)
    never = rng.integers(0, B - 1, size=(I, batch)).astype(np.int32)
    never[never >= 17] += 1
    assert not (never == 17).any()
    once = never.copy(); once[1, 40] = 17
    for name, idx in (("never", never), ("once", once)):
        s = _hip_solver(hip, init, **cfg)
        s.set_minibatch_indices(idx)
        s.add_cloud(src, tgt, init)
        assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
        o = _chain(orc, cfg, src, tgt, idx, init)
        part, opart = s.get_particles(), o.get_particles()
        assert s.get_iterations_run() == I
        assert np.array_equal(np.isnan(part), np.isnan(opart)), name
        assert np.allclose(part, opart, rtol=0, atol=TIGHT, equal_nan=True), name
        if name == "never":
            assert np.isfinite(part).all() and np.isfinite(s.get_trace()["H"]).all()
            assert np.allclose(s.get_transformation(), o.get_transformation(), rtol=0, atol=TIGHT)
            assert np.allclose(s.get_cov_matrix(), o.get_cov_matrix(), rtol=0, atol=TIGHT)
        else:
            assert np.isnan(opart).any()


# =====================================================================================================================
# 4. plane mode
# =====================================================================================================================
PB, PM, PK, PI = 300, 2000, 16, 4
PLANE = dict(max_dist=1.0, delta=0.05)
GAP_FLOOR = 1e-3          # tests/test_plane_gpu.py: normals are compared where the eigenvalue gap determines them


@functools.lru_cache(maxsize=None)
def _plane_clouds():
    return _scans().random_clouds(PB, PM, seed=13, extent=6.0)


def _plane_mean():
    return _scans().rot_zyx(0.002, 0.001, -0.003), np.array([0.01, 0.02, -0.01])     # tests/test_plane_gpu.py's size of initial mean


def _contract_normals(tgt, kn):
    """tests/plane_reference.py's normals() with the neighbours of the contract: itself included, NaN distances never, and
    an offset whose square float32 cannot hold (|d| >= 2^64, NaN included) counts as non-finite."""
    idx, _ = nf.knn_contract(tgt, tgt, kn)
    with np.errstate(all="ignore"):
        d = tgt[idx] - tgt[:, None, :]
        finite = (np.abs(d) < 2.0 ** 64).all(axis=(1, 2))
        d = np.where(finite[:, None, None], d, 0.0)
        mean = np.zeros((tgt.shape[0], 3))
        for k in range(kn):
            mean = mean + d[:, k, :]
        mean = mean / kn
        c = d - mean[:, None, :]
        cov = np.zeros((tgt.shape[0], 3, 3))
        for k in range(kn):
            cov = cov + c[:, k, :, None] * c[:, k, None, :]
    cov[~finite] = np.eye(3)
    lam, vec = np.linalg.eigh(cov)
    valid = finite & (lam[:, 2] > 0.0) & (lam[:, 1] >= pr.MIN_RATIO * lam[:, 2])
    n = vec[:, :, 0].copy()
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[~valid] = 0.0
    return n, valid, lam


def _plane_solver(hip, src, tgt, init, kn=16):
    prm = hip.SteinICPParam(iterations=PI, lr=1.0, max_dist=PLANE["max_dist"], KNN_count=PK, SVN_full_grad=False, record_trace=True)
    s = hip.SVNICP(prm, init, hip.ParticleWeightOpt())
    s.set_residual("plane", PLANE["delta"], kn)
    s.add_cloud(src, tgt, init)
    s.set_initial_mean(_plane_mean())
    return s


def _plane_compare(s, ref, keep=None):
    run = s.get_iterations_run()
    assert run == ref.iterations_run
    tr = s.get_trace()
    corr = tr["corr"][:run] if keep is None else tr["corr"][:run][:, :, keep]
    assert np.array_equal(corr, ref.corr[:run])
    for k, r in (("H", ref.H), ("b", ref.b), ("newton", ref.newton), ("phi", ref.phi)):
        assert np.allclose(tr[k][:run], r[:run], rtol=TIGHT, atol=TIGHT), k
    assert np.abs(s.get_particles() - ref.particles).max() <= TIGHT
    stats, _ = s.get_plane_stats()
    assert np.array_equal(stats[:, 0], ref.stats[:, 0])
    assert np.allclose(stats[:, 1], ref.stats[:, 1], rtol=TIGHT, atol=TIGHT)


@pytest.mark.parametrize("P", [1, 4, 64])
def test_plane_mode_rejects_bad_rows(hip, orc, P):
    """A non-finite or huge source row, and a target row that cannot be a neighbour, are rejected pairs: exact zeros, so the
    registration equals the helper's on the clouds without those rows."""
    src, tgt = _plane_clouds()
    R0, t0 = _plane_mean()
    nrm, _, _ = pr.normals(orc, tgt, 16)
    bad_s = [0, 17, 63, 64, 150, 299]
    bad_t = [PK, PK + 1, 300, 301, 302, 1000, PM - 2, PM - 1]
    src_b, tgt_b = nf.poison(src, bad_s, nf.KINDS), nf.poison(tgt, bad_t, nf.KINDS)
    init = _scans().make_particles(P, seed=3)
    keep_s = np.ones(PB, bool); keep_s[bad_s] = False
    keep_t = np.ones(PM, bool); keep_t[bad_t] = False
    ref = pr.run(orc, src[keep_s], tgt[keep_t], nrm[keep_t], init, PK, PI, PLANE["max_dist"], PLANE["delta"], svn_full_grad=False,
                 R0=R0, t0=t0)
    assert 0 < ref.stats[:, 0].min() and np.isfinite(ref.particles).all(), "every particle must keep accepted pairs"
    s = _plane_solver(hip, src_b, tgt_b, init)
    s.set_target_normals(nrm)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    assert np.isfinite(s.get_trace()["H"]).all() and np.isfinite(s.get_trace()["b"]).all()
    _plane_compare(s, ref, keep_s)


@pytest.mark.parametrize("P", [1, 4, 64])
def test_plane_mode_supplied_normals_without_a_normal(hip, orc, P):
    """Supplied rows of NaN, inf and zero mean "no normal here": they come back as zero rows and their points are never
    accepted."""
    src, tgt = _plane_clouds()
    R0, t0 = _plane_mean()
    nrm, _, _ = pr.normals(orc, tgt, 16)
    nrm = nrm.copy()
    none = np.arange(0, PM, 3)                                     # a third of the target: many winners among them
    nrm[none[0::4]] = np.nan
    nrm[none[1::4], 1] = np.inf
    nrm[none[2::4]] = 0.0
    nrm[none[3::4], 2] = -np.inf
    kept = pr.normalise_supplied(nrm, tgt)
    assert not kept[none].any()
    init = _scans().make_particles(P, seed=3)
    s = _plane_solver(hip, src, tgt, init)
    s.set_target_normals(nrm)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    got = s.get_target_normals()
    assert np.array_equal(got[none], np.zeros((none.size, 3)))
    assert np.allclose(got, kept, rtol=0, atol=1e-15)
    ref = pr.run(orc, src, tgt, kept, init, PK, PI, PLANE["max_dist"], PLANE["delta"], svn_full_grad=False, R0=R0, t0=t0)
    cand, _ = orc.knn_topk(orc.transform(src, R0, t0), tgt, PK)
    Rt, tt = pr.total_pose(orc, init[:, 0], R0, t0)
    slot, ok, _, _ = pr.pairs(src, tgt, kept, cand, Rt, tt, PLANE["max_dist"])
    lost = np.isin(cand[np.arange(PB), slot], none)
    assert lost.sum() > PB // 6 and not ok[lost].any(), "the case must have winners without a normal"
    _plane_compare(s, ref)


@pytest.mark.parametrize("kn", [8, 16])
def test_estimated_normals_on_a_target_with_bad_rows(hip, orc, kn):
    src, tgt = _plane_clouds()
    rng = np.random.default_rng(kn)
    rows = np.sort(rng.choice(PM, PM // 100, replace=False)).tolist() + [0, PM - 1]
    bad = nf.poison(tgt, rows, nf.KINDS)
    ref_n, ref_valid, lam = _contract_normals(bad, kn)
    assert not ref_valid[rows].any()
    s = _plane_solver(hip, src, bad, np.zeros((6, 1)), kn=kn)
    assert s._L.svnicp_align_begin(s.handle) == 0, s._L.svnicp_last_error(s.handle)
    n = s.get_target_normals()
    valid = (n != 0.0).any(axis=1)
    assert np.isfinite(n).all()
    assert not valid[rows].any(), "a bad target point itself has no normal"
    l2 = np.where(lam[:, 2] > 0, lam[:, 2], 1.0)
    near_thr = np.abs(lam[:, 1] / l2 - pr.MIN_RATIO) <= 1e-6 * pr.MIN_RATIO
    assert near_thr.sum() <= 0.001 * PM
    assert np.array_equal(valid[~near_thr], ref_valid[~near_thr])
    assert np.abs(np.linalg.norm(n[valid], axis=1) - 1.0).max() <= 1e-12
    both = valid & ref_valid
    low_gap = both & ((lam[:, 1] - lam[:, 0]) / l2 < GAP_FLOOR)
    cmp = both & ~low_gap
    assert low_gap.sum() <= 0.02 * PM
    assert (1.0 - np.abs((n[cmp] * ref_n[cmp]).sum(axis=1))).max() <= TIGHT
