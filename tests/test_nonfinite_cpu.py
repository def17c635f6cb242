"""CPU side of the non-finite-point contract: tests/nonfinite_reference.py against the oracle wherever the oracle is well
defined, the three places where it is not (asserted as divergences, so the next reader sees why the GPU tests do not use
the oracle there), and the oracle solver runs that tests/test_nonfinite_gpu.py leans on."""
import numpy as np
import pytest

import nonfinite_reference as nf


def _clouds(pkg, B=50, M=400, seed=5):
    return pkg.scans.random_clouds(B, M, seed=seed)


def _equal(orc, q, tgt, K):
    oi, od = orc.knn_topk(q, tgt, K)
    ci, cd = nf.knn_contract(q, tgt, K)
    return np.array_equal(oi, ci) and np.array_equal(od.view(np.int64), cd.view(np.int64))


# ---------------------------------------------------------------- the helpers themselves
def test_poison_and_remove_rows():
    c = np.arange(30, dtype=np.float64).reshape(10, 3) + 1.0
    for kind in nf.KINDS:
        p = nf.poison(c, [2, 7], kind)
        assert np.array_equal(np.delete(p, [2, 7], 0), np.delete(c, [2, 7], 0))
        bad = p[[2, 7]]
        if kind == "nan1":
            assert (np.isnan(bad).sum(axis=1) == 1).all()
        elif kind == "nan3":
            assert np.isnan(bad).all()
        elif kind in ("+inf", "-inf"):
            assert (np.isinf(bad).sum(axis=1) == 1).all() and (np.sign(bad[np.isinf(bad)]) == (1 if kind == "+inf" else -1)).all()
        elif kind == "big32":
            f = bad.astype(np.float32)
            with np.errstate(over="ignore"):
                assert np.isfinite(f).all() and (np.isinf(f * f).sum(axis=1) == 2).all() and np.isfinite(bad * bad).all()
        else:
            with np.errstate(over="ignore"):
                assert np.isfinite(bad).all() and np.isinf(bad * bad).any(axis=1).all()
    mixed = nf.poison(c, range(6), nf.KINDS)
    assert np.isnan(mixed[0]).sum() == 1 and np.isnan(mixed[1]).all() and mixed[5, 1] == 1e160
    kept, m = nf.remove_rows(c, [0, 3, 9])
    assert kept.shape == (7, 3) and m.tolist() == [-1, 0, 1, -1, 2, 3, 4, 5, 6, -1]
    assert np.array_equal(kept, c[m >= 0])


def test_nearest_of_k_rules():
    tgt = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0]])
    Ts = np.array([[0.9, 0, 0], [0.9, 0, 0], [0.9, 0, 0], [np.nan, 0, 0], [0.9, 0, 0]])
    cand = np.array([[0, 1, 2], [2, 1, 0], [3, 1, 0], [0, 1, 2], [4, 3, 4]])
    pos, d = nf.nearest_of_k(Ts, tgt, cand)
    assert pos.tolist() == [1, 0, 0, 0, 0]          # first of a tie; NaN first never replaced; all-NaN and inf/NaN rows keep 0
    assert d[0] == d[1] and np.isnan(d[2]) and np.isnan(d[3]) and d[4] == np.inf
    pos2, _ = nf.nearest_of_k(np.stack([Ts, Ts]), tgt, cand)       # leading particle axis
    assert pos2.shape == (2, 5) and (pos2 == pos).all()


# ---------------------------------------------------------------- knn_contract == oracle where the oracle is well defined
@pytest.mark.parametrize("B,M,K", [(50, 400, 16), (33, 257, 1), (7, 5, 9), (20, 130, 128)])
def test_contract_equals_oracle_on_finite_clouds(pkg, orc, B, M, K):
    q, tgt = _clouds(pkg, B, M, seed=B + K)
    assert _equal(orc, q, tgt, K)
    grid = np.floor(tgt * 2.0)                      # massive exact ties: (d², index) order
    assert _equal(orc, np.floor(q * 2.0), grid, K)


def test_contract_equals_oracle_with_nan_targets_behind_the_first_k(pkg, orc):
    q, tgt = _clouds(pkg)
    K = 16
    for kind in nf.NAN_KINDS:
        t = nf.poison(tgt, [K, K + 1, 100, 101, 102, 399], kind)
        assert _equal(orc, q, t, K), kind
        assert not (nf.knn_contract(q, t, K)[0][..., None] == np.array([K, K + 1, 100, 101, 102, 399])).any()


@pytest.mark.parametrize("kind", nf.NUMBER_KINDS)
def test_contract_equals_oracle_with_inf_and_huge_targets_anywhere(pkg, orc, kind):
    q, tgt = _clouds(pkg)
    K = 16
    t = nf.poison(tgt, [0, 3, K - 1, K, 200, 399], kind)
    assert _equal(orc, q, t, K)
    few = nf.poison(tgt[:20], range(12), kind)      # more bad rows than M - K: +inf distances ARE neighbours, ordered by index
    assert _equal(orc, q, few, K)
    ci, cd = nf.knn_contract(q, few, K)
    assert (cd[:, 8:] >= 9e76).all() and (np.sort(ci[:, 8:], axis=1) == np.arange(8)).all()
    if kind != "big32":                             # big32: 9e76 + ..., finite in float64
        assert np.isinf(cd[:, 8:]).all() and (ci[:, 8:] == np.arange(8)).all()


@pytest.mark.parametrize("kind", nf.NUMBER_KINDS)
def test_contract_equals_oracle_for_inf_and_huge_queries(pkg, orc, kind):
    q, tgt = _clouds(pkg)
    K = 16
    qq = nf.poison(q, [0, 17, 49], kind)
    assert _equal(orc, qq, tgt, K)
    ci, cd = nf.knn_contract(qq, tgt, K)
    if kind != "big32":                             # d² = +inf against every target: rows 0..K-1 (big32: 9e76 + ..., finite)
        assert (ci[[0, 17, 49]] == np.arange(K)).all() and np.isinf(cd[[0, 17, 49]]).all()
    keep = np.setdiff1d(np.arange(50), [0, 17, 49])
    oi, od = orc.knn_topk(q, tgt, K)                # every other row: as on the clean queries
    assert np.array_equal(ci[keep], oi[keep]) and np.array_equal(cd[keep], od[keep])


# ---------------------------------------------------------------- … and the three places where it is not
def test_oracle_diverges_nan_target_inside_the_first_k(pkg, orc):
    """The reference's heap inserts while size < K whatever the distance.  A NaN at target 0 is the heap's root, nothing
    sifts past it (x < NaN is false) and `dist < top` is false ever after: the first K targets come back.  A NaN further
    into the first K stays in the heap as an entry that compares with nothing, and comes back as a neighbour."""
    q, tgt = _clouds(pkg)
    K = 16
    oi, od = orc.knn_topk(q, nf.poison(tgt, [0], "nan3"), K)
    assert (np.sort(oi, axis=1) == np.arange(K)).all() and np.isnan(od).any(axis=1).all()
    t = nf.poison(tgt, [3], "nan3")
    oi, od = orc.knn_topk(q, t, K)
    ci, cd = nf.knn_contract(q, t, K)
    assert (oi == 3).any(axis=1).all() and np.isnan(od).any(axis=1).all()
    assert not (ci == 3).any() and not np.isnan(cd).any()
    clean, m = nf.remove_rows(t, [3])
    ki, kd = orc.knn_topk(q, clean, K)              # the contract: as if the row were not there
    assert np.array_equal(m[ci], ki) and np.array_equal(cd, kd)


def test_oracle_diverges_nan_query(pkg, orc):
    q, tgt = _clouds(pkg)
    K = 16
    qq = nf.poison(q, [5], "nan1")
    oi, od = orc.knn_topk(qq, tgt, K)
    ci, cd = nf.knn_contract(qq, tgt, K)
    assert np.isnan(od[5]).all() and (np.sort(oi[5]) == np.arange(K)).all()
    assert (ci[5] == 0).all() and (cd[5] == 0.0).all() and not np.signbit(cd[5]).any()
    keep = np.arange(50) != 5
    assert np.array_equal(oi[keep], ci[keep]) and np.array_equal(od[keep], cd[keep])


def test_oracle_diverges_fewer_than_k_eligible_targets(pkg, orc):
    q, tgt = _clouds(pkg)
    K = 16
    t = nf.poison(tgt[:40], range(5, 40), "nan3")   # 5 eligible targets
    oi, od = orc.knn_topk(q, t, K)
    ci, cd = nf.knn_contract(q, t, K)
    assert np.isnan(od).any(axis=1).all() and (oi >= 5).any(axis=1).all()       # NaN rows returned as neighbours
    assert (np.sort(ci[:, :5], axis=1) == np.arange(5)).all() and (ci[:, 5:] == 0).all() and (cd[:, 5:] == 0.0).all()
    ki, kd = orc.knn_topk(q, tgt[:5], K)            # = the oracle's own zero padding for M < K
    assert np.array_equal(ci, ki) and np.array_equal(cd, kd)
    ci, cd = nf.knn_contract(q, nf.poison(tgt[:40], range(40), "nan1"), K)      # no eligible target at all
    assert not ci.any() and not cd.any()


# ---------------------------------------------------------------- nearest_of_k == the oracle's first search
def test_nearest_of_k_equals_oracle_first_iteration(pkg, orc):
    P, B, M, K = 4, 300, 1000, 10
    src, tgt = pkg.scans.random_clouds(B, M, seed=9)
    src = nf.poison(src, [7, 8, 9, 10], ("nan1", "+inf", "big32", "big64"))
    init = pkg.scans.make_particles(P, seed=4) * 0.3
    o = orc.Solver(init, iterations=1, lr=1.0, max_dist=1.0, knn_count=K, svn_full_grad=False)
    o.add_cloud(src, tgt, init); tro = o.enable_trace(); o.stein_align()
    Ts = np.stack([orc.transform(src, orc.so3_exp(init[3:, p])[0], init[:3, p]) for p in range(P)])
    pos, d = nf.nearest_of_k(Ts, tgt, o.candidates())
    assert np.array_equal(pos, tro["corr"][0])
    assert np.array_equal(d < 1.0, tro["mask"][0].astype(bool))
    assert (pos[:, 7] == 0).all() and not tro["mask"][0][:, 7:11].any()


# ---------------------------------------------------------------- oracle solver runs the GPU tests rely on
CFG = dict(iterations=4, lr=1.0, max_dist=1.0, check_early_stop=True, convergence_threshold=1e-5, knn_count=10, svn_full_grad=False)


def _run(orc, src, tgt, init, mode=None, **over):
    cfg = dict(CFG, **over)
    o = orc.Solver(init, **cfg) if mode is None else orc.Solver(init, mode=mode, **cfg)
    o.add_cloud(src, tgt, init)
    tro = o.enable_trace()
    o.stein_align()
    return o, tro


@pytest.fixture(scope="module")
def solver_clouds(pkg):
    src, tgt = pkg.scans.random_clouds(300, 1000, seed=21)
    return src, tgt, pkg.scans.make_particles(4, seed=2) * 0.3


def test_oracle_nan_source_row(orc, solver_clouds):
    src, tgt, init = solver_clouds
    I, P = CFG["iterations"], init.shape[1]
    o, tro = _run(orc, nf.poison(src, [17], "nan1"), tgt, init)
    assert np.isnan(tro["H"]).all()                         # the mask is a multiplication: 0 · NaN, from iteration 0
    assert (tro["corr"][:, :, 17] == 0).all()               # a NaN first distance is never replaced
    assert o.iterations_run() == I                          # the stop flag compares a NaN norm: never fires
    part = o.get_particles().reshape(6, P)
    assert np.isnan(part[:3]).all() and np.isfinite(part[3:]).all()     # partial: the rotation entries stay numbers
    g, _ = _run(orc, nf.poison(src, [17], "nan1"), tgt, init, mode=orc.MODE_SVGD, lr=0.01, optimizer="Adam")
    assert np.isnan(g.get_particles()).all()                # SVGD mode: every entry
    for kind in ("nan3", "+inf", "-inf"):                   # an infinite row is masked by 0 · inf = NaN: the same
        o, tro = _run(orc, nf.poison(src, [17], kind), tgt, init)
        assert np.isnan(tro["H"]).all() and (tro["corr"][:, :, 17] == 0).all() and o.iterations_run() == I, kind
        part = o.get_particles().reshape(6, P)
        assert np.isnan(part[:3]).all() and np.isfinite(part[3:]).all(), kind


@pytest.mark.parametrize("kind", ["big32", "big64"])
def test_oracle_huge_source_rows_are_masked_but_not_removed(orc, solver_clouds, kind):
    src, tgt, init = solver_clouds
    rows = [0, 17, 299]
    o, tro = _run(orc, nf.poison(src, rows, kind), tgt, init)
    for key in ("H", "b", "phi"):
        assert np.isfinite(tro[key]).all(), key
    assert np.isfinite(o.get_particles()).all() and not tro["mask"][:, :, rows].any()
    c, trc = _run(orc, nf.remove_rows(src, rows)[0], tgt, init)
    assert not np.array_equal(o.get_particles(), c.get_particles())     # a masked row still adds RᵀR = I to H's translation block
    assert np.allclose(tro["H"][0][:, 0] - len(rows), trc["H"][0][:, 0], rtol=1e-9)


def test_oracle_bad_target_rows_behind_the_first_k_are_invisible(orc, solver_clouds):
    src, tgt, init = solver_clouds
    rows = [10, 11, 500, 501, 502, 998, 999]
    t = nf.poison(tgt, rows, ("nan1", "nan3", "+inf", "-inf", "big64"))
    clean, m = nf.remove_rows(t, rows)
    a, tra = _run(orc, src, t, init)
    b, trb = _run(orc, src, clean, init)
    assert np.array_equal(m[a.candidates()], b.candidates()) and np.array_equal(a.candidate_dist2(), b.candidate_dist2())
    assert np.array_equal(tra["corr"], trb["corr"])
    assert np.array_equal(a.get_particles(), b.get_particles())
