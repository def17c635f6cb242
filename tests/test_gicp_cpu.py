"""The generalized-ICP residual without a GPU: pins tests/gicp_reference.py (the float64 numpy
restatement the GPU tests compare the device against) on its own, the gicp_refusal ladder of registration_plan.hpp compiled
on the host, the per-pair arithmetic of the kernel (csrc/gicp_pair_device.hpp) as a stand-alone program under the address and
undefined-behaviour sanitizers, and the presence of the new interface."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import gicp_reference as gr
import plane_reference as pr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "svn-icp_amd", "csrc")
U = 2.0 ** -52
NEW_EXPORTS = ("svnicp_set_residual_gicp", "svnicp_set_source_normals", "svnicp_get_source_normals", "svnicp_get_gicp_stats")


def _exp(w):
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if a == 0:
        return np.eye(3), np.eye(3)
    R = np.eye(3) + np.sin(a) / a * K + (1 - np.cos(a)) / a ** 2 * K @ K
    J = np.eye(3) + (1 - np.cos(a)) / a ** 2 * K + (a - np.sin(a)) / a ** 3 * K @ K      # left Jacobian
    return R, J


def _huber(rho, delta):
    return np.where(rho <= delta, 0.5 * rho * rho, delta * rho - 0.5 * delta * delta)


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


_SCENE = {}


def _scene(pkg, orc):
    """512 x 2048 random clouds, normals of both from 12 neighbours (every fifth source row made bare), one pose; shared by the
    tests below, never changed."""
    if not _SCENE:
        src, tgt = pkg.scans.random_clouds(512, 2048, seed=5)
        nt, _, _ = gr.normals(orc, tgt, 12)
        ns, _, _ = gr.normals(orc, src, 12)
        ns[::5] = 0.0                                       # every fifth source row has no normal (the random cloud's all have one)
        x6 = np.array([0.03, -0.02, 0.015, 0.004, -0.006, 0.005])
        R0 = _exp(np.array([0.002, 0.001, -0.003]))[0]
        t0 = np.array([0.01, 0.02, -0.01])
        Rt, tt = gr.total_pose(orc, x6, R0, t0)
        cand, _ = orc.knn_topk(orc.transform(src, R0, t0), tgt, 8)
        _SCENE.update(src=src, tgt=tgt, nt=nt, ns=ns, Rt=Rt, tt=tt, cand=cand)
    return _SCENE


# ---------------------------------------------------------------------------------------------
# 1. the weight
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1e-6, 1e-3, 0.1, 1.0])
def test_weight_is_spd_with_eigenvalues_in_eps_one_and_the_scaled_inverse(eps):
    """W = 2 eps S^-1 for random unit-normal pairs and the adversarial ones (m = +-n, orthogonal, nearly parallel, nearly
    antiparallel): symmetric, eigenvalues in [eps, 1], equal to 2 eps numpy.linalg.inv(S).

    Bound.  S has eigenvalues in [2 eps, 2], so cond(S) <= 1/eps.  The cofactor inverse forms every entry of adj(S) and
    det(S) from products of entries of S that are themselves a few roundings off: each result carries an absolute error of a
    few u |S|^2 resp. u |S|^3, which relative to S^-1 is a few u cond(S) (the classical bound for an inverse by Cramer's rule
    on a 3 x 3).  LAPACK's inverse carries the same cond(S) u.  Both together: |W - 2 eps inv(S)|_max <= 16 cond(S) u |W|_max,
    and an eigenvalue of a symmetric matrix moves by at most the 2-norm of the perturbation, <= 3 x the largest entry."""
    rng = np.random.default_rng(11)
    m, n = _unit(rng, 400), _unit(rng, 400)
    tiny = 1e-7 * _unit(rng, 50)
    near = m[:50] + tiny
    near /= np.linalg.norm(near, axis=1, keepdims=True)
    ortho = np.cross(m[:50], n[:50])
    ortho /= np.linalg.norm(ortho, axis=1, keepdims=True)
    M = np.concatenate([m, m[:50], m[:50], m[:50], m[:50], m[:50]])
    N = np.concatenate([n, m[:50], -m[:50], near, -near, ortho])
    W = gr.weight(M, N, eps)
    S = gr.surface_sum(M, N, eps)
    assert np.array_equal(W, np.transpose(W, (0, 2, 1)))
    cond = np.linalg.cond(S)
    assert cond.max() <= (1.0 / eps) * (1 + 1e-9)
    ref = 2.0 * eps * np.linalg.inv(S)
    err = np.abs(W - ref).max(axis=(1, 2)) / np.abs(ref).max(axis=(1, 2))
    bound = 16.0 * cond * U
    print(f"eps {eps:g}: max cond(S) {cond.max():.3e}, max |W - 2 eps inv(S)| / |W| = {err.max():.3e}, worst ratio to the bound {(err / bound).max():.3e}")
    assert (err <= bound).all()
    lam = np.linalg.eigvalsh(W)
    slack = 3.0 * bound                                     # |W| <= 1: the absolute perturbation of an eigenvalue
    assert (slack < 0.05 * eps).all(), "the slack must stay far below the smallest eigenvalue"
    assert (lam[:, 0] >= eps - slack).all() and (lam[:, 2] <= 1.0 + slack).all()
    if eps == 1.0:
        assert np.array_equal(W, np.broadcast_to(np.eye(3), W.shape)), "eps = 1: W = I exactly"
    par = gr.weight(M[400:450], N[400:450], eps)            # m = n: (1 - eps) m m^T + eps I
    want = (1.0 - eps) * M[400:450, :, None] * M[400:450, None, :] + eps * np.eye(3)
    assert np.abs(par - want).max() <= 16.0 * (1.0 / eps) * U


# ---------------------------------------------------------------------------------------------
# 2. the record
# ---------------------------------------------------------------------------------------------
def test_b_is_the_gradient_of_the_huber_cost_with_the_weight_frozen(pkg, orc):
    """b = d/dxi sum Huber(rho(T Exp xi)) at xi = 0 by central differences, pairs, winners and W as at xi = 0; H against an
    independent loop.

    Tolerance of the gradient, from the step h alone.  Per pair y(tau) = W^(1/2) u(tau) along coordinate k, rho = |y|, and
    |W| <= 1, so y's derivatives are bounded by u's.  A translation coordinate makes u linear with |u'| = 1; a rotation
    coordinate turns s about a unit axis, so |u'|, |u''|, |u'''| <= L := 1 + |s|.
    Inside (rho <= delta) g = y.y / 2:  g''' = 3 y'.y'' + y.y''',  |g'''| <= 3 L^2 + delta L.
    Outside g = delta |y| + const.  With n = |y|:  n' = yh.y',  n'' = (|y'|^2 - n'^2) / n + yh.y'',  and differentiating once
    more, |n'''| <= 6 L^2 / n + 3 L^3 / n^2 + L.  Over the stencil n >= delta / 2 (h L << delta, asserted), so
    |g'''| = delta |n'''| <= 12 L^2 + 12 L^3 / delta + delta L.  The central difference is off by at most h^2 / 6 of that.
    A pair whose rho is within h L of delta may cross the kink inside the stencil: g' is Lipschitz there with constant
    K = max(L^2 + delta L, delta (L^2 / n + L)) <= 2 L^2 + delta L, which bounds its error by h K.  Round-off: the two cost sums
    carry at most N eps cost each, divided by 2 h."""
    sc = _scene(pkg, orc)
    src, tgt, nt, ns, Rt, tt, cand = (sc[k] for k in ("src", "tgt", "nt", "ns", "Rt", "tt", "cand"))
    delta, max_dist, h, eps = 0.015, 0.003, 1e-6, 1e-3
    rec, slot, stats, rho0 = gr.record_one(src, tgt, nt, ns, cand, Rt, tt, max_dist, delta, eps)
    _, ok, e, n = gr.pairs(src, tgt, nt, ns, cand, Rt, tt, max_dist)
    _, ok_plane, _, _ = pr.pairs(src, tgt, nt, cand, Rt, tt, max_dist)
    assert 0 < ok.sum() < ok_plane.sum() < src.shape[0], "the gate and the source normals must each reject some pairs and keep some"
    out = rho0 > delta
    assert 0.05 <= out.mean() <= 0.95, f"{out.mean():.3f} of the accepted pairs lie outside delta"
    s, q = src[ok], tgt[cand[np.arange(src.shape[0]), slot]][ok]
    W, u0, _, w0, G = gr.pair_terms(s, e[ok], n[ok], ns[ok], Rt, delta, eps)

    def cost(xi):
        dR, J = _exp(xi[3:])
        Rp, tp = Rt @ dR, tt + Rt @ (J @ xi[:3])          # T Exp(xi): the solver's right perturbation (SVNICP.cpp:268-279)
        u = ((s @ Rp.T) + tp - q) @ Rt                    # Rt^T e with Rt frozen, like W
        rho = np.sqrt(np.einsum("ni,nij,nj->n", u, W, u))
        return _huber(rho, delta).sum()

    L = 1.0 + np.linalg.norm(s, axis=1)
    assert (h * L < 0.01 * delta).all()
    kink = np.abs(rho0 - delta) <= h * L
    third = np.where(out, 12 * L * L + 12 * L ** 3 / delta + delta * L, 3 * L * L + delta * L)
    tol = (h * h / 6.0) * third.sum() + h * (2 * L * L + delta * L)[kink].sum() + len(rho0) * np.finfo(float).eps * cost(np.zeros(6)) / h
    g = np.zeros(6)
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        g[k] = (cost(d) - cost(-d)) / (2 * h)
    err = np.abs(g - rec[36:]).max()
    print(f"gradient: max |central difference - b| = {err:.3e}, bound {tol:.3e}, |b| max {np.abs(rec[36:]).max():.3e}, "
          f"{kink.sum()} pairs at the kink, {len(rho0)} accepted")
    assert err <= tol
    assert tol < 1e-3 * np.abs(rec[36:]).max(), "the bound must be far below b itself, or the check shows nothing"
    H = 1e-6 * np.eye(6)
    b = np.zeros(6)
    for i in range(len(rho0)):
        Gi = np.concatenate([np.eye(3), -np.array([np.cross(s[i], ek) for ek in np.eye(3)]).T], axis=1)   # [I | -[s]x], column k of [s]x = s x e_k
        H += w0[i] * Gi.T @ W[i] @ Gi
        b += w0[i] * Gi.T @ W[i] @ u0[i]
    assert np.allclose(rec[:36].reshape(6, 6), H, rtol=1e-12, atol=1e-12)
    assert np.allclose(rec[36:], b, rtol=1e-12, atol=1e-12)
    assert np.array_equal(rec[:36].reshape(6, 6), rec[:36].reshape(6, 6).T)
    assert stats[0] == ok.sum()


def test_epsilon_one_is_the_unweighted_point_to_point_record(pkg, orc):
    """eps = 1: W = I exactly, so with delta = +inf the record is the point-to-point Gauss-Newton one of the accepted pairs in
    the world frame, J = [Rt | -Rt [s]x]: H = sum J^T J + 1e-6 I, b = sum J^T e (Rt orthonormal to round-off: 1e-12)."""
    sc = _scene(pkg, orc)
    src, tgt, nt, ns, Rt, tt, cand = (sc[k] for k in ("src", "tgt", "nt", "ns", "Rt", "tt", "cand"))
    rec, slot, stats, rho = gr.record_one(src, tgt, nt, ns, cand, Rt, tt, 0.003, np.inf, 1.0)
    _, ok, e, _ = gr.pairs(src, tgt, nt, ns, cand, Rt, tt, 0.003)
    H, b = 1e-6 * np.eye(6), np.zeros(6)
    for s, ei in zip(src[ok], e[ok]):
        sx = np.array([[0, -s[2], s[1]], [s[2], 0, -s[0]], [-s[1], s[0], 0]])
        J = np.concatenate([Rt, -Rt @ sx], axis=1)
        H += J.T @ J
        b += J.T @ ei
    assert np.allclose(rec[:36].reshape(6, 6), H, rtol=1e-12, atol=1e-12)
    assert np.allclose(rec[36:], b, rtol=1e-12, atol=1e-12)
    assert np.allclose(rho, np.linalg.norm(e[ok], axis=1), rtol=1e-12, atol=0)
    assert np.isclose(stats[1], (e[ok] ** 2).sum(), rtol=1e-12)


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["parallel", "antiparallel"])
@pytest.mark.parametrize("eps", [1e-3, 1e-6])
def test_parallel_normals_are_plane_mode_plus_epsilon_of_point_mode(pkg, orc, eps, sign):
    """n_s = +-Rt^T n_q for every pair: W = (1 - eps) m m^T + eps I (weight 1 along the normal, eps across it), so with
    delta = +inf the sums are (1 - eps) x plane mode's (tests/plane_reference.py) + eps x the point-to-point ones of the same
    pairs.  Bound: the relative error 16 cond(S) u = 16 u / eps of W (test above) times the sum of the terms' magnitudes,
    |G^T G| <= L^2 and |G^T u| <= L |e| per pair with L = 1 + |s|."""
    sc = _scene(pkg, orc)
    src, tgt, nt, Rt, tt, cand = (sc[k] for k in ("src", "tgt", "nt", "Rt", "tt", "cand"))
    max_dist = 0.003
    slot, okp, e, nq = pr.pairs(src, tgt, nt, cand, Rt, tt, max_dist)
    ns = sign * (nq @ Rt)                                   # zero rows where the winner has no normal
    rec, _, stats, _ = gr.record_one(src, tgt, nt, ns, cand, Rt, tt, max_dist, np.inf, eps)
    plane, _, pstats, _ = pr.record_one(src, tgt, nt, cand, Rt, tt, max_dist, np.inf)
    point, _, _, _ = gr.record_one(src, tgt, nt, ns, cand, Rt, tt, max_dist, np.inf, 1.0)
    assert stats[0] == pstats[0] == okp.sum() > 0
    damp = np.concatenate([(gr.DAMPING * np.eye(6)).reshape(36), np.zeros(6)])
    want = (1.0 - eps) * (plane - damp) + eps * (point - damp) + damp
    L = 1.0 + np.linalg.norm(src[okp], axis=1)
    bound_H = 16.0 * U / eps * (L * L).sum()
    bound_b = 16.0 * U / eps * (L * np.linalg.norm(e[okp], axis=1)).sum()
    dH, db = np.abs(rec[:36] - want[:36]).max(), np.abs(rec[36:] - want[36:]).max()
    print(f"eps {eps:g} sign {sign:+.0f}: |H - want| {dH:.3e} (bound {bound_H:.3e}), |b - want| {db:.3e} (bound {bound_b:.3e})")
    assert dH <= bound_H and db <= bound_b
    assert bound_H < 1e-6 * np.abs(want[:36]).max()


def test_rejected_pairs_are_the_gate_a_winner_and_a_source_row_without_a_normal(pkg, orc):
    sc = _scene(pkg, orc)
    src, tgt, nt, ns, Rt, tt, cand = (sc[k] for k in ("src", "tgt", "nt", "ns", "Rt", "tt", "cand"))
    slot, okp, _, _ = pr.pairs(src, tgt, nt, cand, Rt, tt, 0.003)
    ns2 = ns.copy()
    ns2[::3] = 0.0
    _, ok, _, _ = gr.pairs(src, tgt, nt, ns2, cand, Rt, tt, 0.003)
    assert np.array_equal(ok, okp & (ns2 != 0).any(axis=1))
    rec, _, stats, _ = gr.record_one(src, tgt, nt, np.zeros_like(src), cand, Rt, tt, 0.003, 0.1, 1e-3)
    assert np.array_equal(rec[:36].reshape(6, 6), gr.DAMPING * np.eye(6)) and not rec[36:].any() and not stats.any()


# ---------------------------------------------------------------------------------------------
# 3. the kernel's per-pair arithmetic as a stand-alone program under the sanitizers
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("gicp_accum")
    exe = d / "gicp_accum_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-I", CSRC, os.path.join(HERE, "gicp_accum_driver.cpp"), "-o", str(exe)], check=True)
    return exe, d


def _run_driver(exe, d, groups):
    """groups: list of arrays [n, 15] = ok s u m n eps delta -> [len(groups), 29]."""
    with open(d / "cases.txt", "w") as f:
        for g in groups:
            for row in g:
                f.write(" ".join(float(v).hex() for v in row) + "\n")
            f.write("=\n")
    r = subprocess.run([str(exe), str(d / "cases.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return np.array([[float.fromhex(t) for t in line.split()] for line in r.stdout.splitlines()])


def _sums_of(rows):
    """The 29 sums of the driver's layout from the restatement's terms, for rows [n, 15] (all accepted or not by column 0)."""
    ok = rows[:, 0] != 0
    s, u, m, n = rows[ok, 1:4], rows[ok, 4:7], rows[ok, 7:10], rows[ok, 10:13]
    out = np.zeros(29)
    if not ok.any():
        return out
    eps, delta = rows[0, 13], rows[0, 14]
    W = gr.weight(m, n, eps)
    v = np.einsum("nij,nj->ni", W, u)
    rho = np.sqrt(np.maximum((u * v).sum(axis=1), 0.0))
    w = gr.huber_weight(rho, delta)
    G = np.concatenate([np.broadcast_to(np.eye(3), (len(s), 3, 3)), -gr.skew(s)], axis=2)
    H = np.einsum("n,nji,njk,nkl->il", w, G, W, G)
    out[:21] = H[np.triu_indices(6)]
    out[21:27] = np.einsum("n,nji,nj->i", w, G, v)
    out[27], out[28] = ok.sum(), (w * rho * rho).sum()
    return out


def test_pair_program_agrees_with_the_restatement_on_graded_and_adversarial_pairs(driver):
    """eps at both ends, m = +-n_s, orthogonal normals, zero normals on a rejected pair, points at kilometres, delta = +inf and a
    delta every rho exceeds.  Compared per group of 64 pairs within 64 (cond(S) + 8) u times the sum of the terms' magnitudes
    (the inverse's cond(S) u, and a few u for the products and the 64 additions in another order)."""
    exe, d = driver
    rng = np.random.default_rng(5)
    groups, conds = [], []
    for eps in (1e-6, 1e-3, 1.0):
        for kind in ("random", "parallel", "antiparallel", "orthogonal"):
            for scale, delta in ((1.0, np.inf), (1000.0, 1e-3), (1.0, 0.02)):
                n = 64
                m = _unit(rng, n)
                ns = {"random": _unit(rng, n), "parallel": m, "antiparallel": -m}.get(kind)
                if ns is None:
                    ns = np.cross(m, _unit(rng, n))
                    ns /= np.linalg.norm(ns, axis=1, keepdims=True)
                s = scale * rng.standard_normal((n, 3))
                u = 0.05 * rng.standard_normal((n, 3))
                ok = np.ones(n)
                ok[::7] = 0.0
                rows = np.column_stack([ok, s, u, m, ns, np.full(n, eps), np.full(n, delta)])
                rows[::7, 1:13] = np.nan                     # a rejected pair's operands are never used
                groups.append(rows)
                conds.append(1.0 / eps)
    got = _run_driver(exe, d, groups)
    worst = 0.0
    for rows, cond, g in zip(groups, conds, got):
        with np.errstate(invalid="ignore"):
            want = _sums_of(rows)
        acc = rows[rows[:, 0] != 0]
        Ls = 1.0 + np.linalg.norm(acc[:, 1:4], axis=1)
        un = np.linalg.norm(acc[:, 4:7], axis=1)
        mag = np.concatenate([np.full(21, (Ls * Ls).sum()), np.full(6, (Ls * un).sum()), [0.0], [(un * un).sum()]])
        bound = 64.0 * (cond + 8.0) * U * mag
        assert np.isfinite(g).all()
        assert g[27] == want[27]
        worst = max(worst, float((np.abs(g - want) / np.maximum(bound, 1e-300))[mag > 0].max()))
        assert (np.abs(g - want) <= bound).all(), (np.abs(g - want) / np.maximum(bound, 1e-300)).max()
    print(f"{len(groups)} groups: worst |program - restatement| / bound = {worst:.3e}")


def test_pair_program_exact_cases(driver):
    exe, d = driver
    m = np.array([0.0, 0.0, 1.0])
    z = np.zeros(3)

    def row(ok, s, u, mm, nn, eps, delta):
        return np.concatenate([[ok], s, u, mm, nn, [eps, delta]])

    s = np.array([1.0, 2.0, 4.0])
    u = np.array([0.5, 0.25, 0.125])
    groups = [
        np.array([row(1, s, u, m, m, 1.0, np.inf)]),                      # eps = 1: W = I exactly
        np.array([row(0, s, u, m, m, 1e-3, 0.1), row(0, np.full(3, np.nan), np.full(3, np.inf), z, z, 1e-3, 0.1)]),   # all rejected
        np.array([row(1, s, np.array([0.0, 0.0, 0.5]), m, m, 1.0, 0.5)]),                 # rho = delta: weight 1
        np.array([row(1, s, np.array([0.0, 0.0, 0.5]), m, m, 1.0, np.nextafter(0.5, 0.0))]),   # delta one ulp below rho
    ]
    got = _run_driver(exe, d, groups)
    sx = np.array([[0, -4.0, 2.0], [4.0, 0, -1.0], [-2.0, 1.0, 0]])
    G = np.concatenate([np.eye(3), -sx], axis=1)
    assert np.array_equal(got[0][:21], (G.T @ G)[np.triu_indices(6)])     # small dyadic numbers: every product and sum is exact
    assert np.array_equal(got[0][21:27], G.T @ u) and got[0][27] == 1 and got[0][28] == u @ u
    assert not got[1].any()
    assert got[2][28] == 0.25 and got[2][23] == 0.5
    w = np.nextafter(0.5, 0.0) / 0.5
    assert got[3][23] == w * 0.5 and got[3][28] == w * 0.25 and got[3][0] == w


# ---------------------------------------------------------------------------------------------
# 4. the refusal ladder, compiled on its own
# ---------------------------------------------------------------------------------------------
GICP = "svnicp_align: the generalized-ICP residual (svnicp_set_residual_gicp) is not available here: "
LADDER = [
    ("off", "f.svgd = true;", "-"),
    ("fine", "f.gicp = true;", "-"),
    ("svgd", "f.gicp = true; f.svgd = true;", GICP + "SVGD mode has no Hessian to put the plane residual in"),
    ("partial-shard", "f.gicp = true; f.shard_set = true; f.p_hi = 8;", GICP + "a partial particle shard (svnicp_set_shard) is set"),
    ("row-shard", "f.gicp = true; f.row_world = 2;",
     GICP + "a source-row shard (svnicp_set_row_shard) is set: the rank exchange carries the 22 point-to-point sums"),
    ("minibatch", "f.gicp = true; f.batch = 100;", GICP + "mini-batch mode (svnicp_set_minibatch) is set"),
    ("full-corr", "f.gicp = true; t.full_corr = 1;", GICP + "option correspondence=full is set"),
    ("persistent", "f.gicp = true; t.persistent = 1;", GICP + "option chain=persistent is set"),
    ("accum", "f.gicp = true; t.accum = 1;", GICP + "option accum is not split: the plane kernel consumes the search kernel's winner index"),
    ("K129", "f.gicp = true; f.K = 129;", GICP + "knn_count exceeds 128: the plane kernel consumes the matrix-pipe search kernel's winner index"),
    ("few-targets", "f.gicp = true; f.M = 15;", GICP + "the target has fewer points than normal_k and no normals were supplied"),
    ("few-targets-supplied", "f.gicp = true; f.M = 15; f.normals_supplied = true;", "-"),
    ("few-sources", "f.gicp = true; f.B = 15;", GICP + "the source has fewer points than normal_k and no source normals were supplied"),
    ("few-sources-supplied", "f.gicp = true; f.B = 15; f.source_normals_supplied = true;", "-"),
    ("few-sources-normal-k", "f.gicp = true; f.B = 15; f.normal_k = 15;", "-"),
    ("target-before-source", "f.gicp = true; f.B = 15; f.M = 15;", GICP + "the target has fewer points than normal_k and no normals were supplied"),
    ("plane-flag-alone-is-not-gicp", "f.plane = true; f.B = 15;", "-"),
]
PROBE = r"""
#include <cstdio>
#include <string>
#include "registration_plan.hpp"
using namespace svnicp;
static RegistrationFacts base() { RegistrationFacts f; f.P = 16; f.p_lo = 0; f.p_hi = 16; f.K = 100; f.I = 12; f.B = 1100; f.M = 20000; return f; }
int main() {
@CASES@
  return 0;
}
"""


@pytest.fixture(scope="module")
def ladder(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("gicp_plan")
    lines = "\n".join('  { RegistrationFacts f = base(); Tuning t; (void)t; %s const char* w = gicp_refusal(f, t); '
                      'std::printf("%d|%%s\\n", w ? (std::string(kGicpRefusal) + w).c_str() : "-"); }' % (setup, i)
                      for i, (_, setup, _) in enumerate(LADDER))
    (d / "probe.cpp").write_text(PROBE.replace("@CASES@", lines))
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(d / "probe.cpp"), "-o", str(d / "probe")], check=True)
    out = subprocess.run([str(d / "probe")], check=True, capture_output=True, text=True).stdout
    return dict((int(i), v) for i, v in (l.split("|", 1) for l in out.splitlines()))


@pytest.mark.parametrize("i", range(len(LADDER)), ids=[c[0] for c in LADDER])
def test_gicp_refusal_ladder(ladder, i):
    assert ladder[i] == LADDER[i][2], LADDER[i][:2]


# ---------------------------------------------------------------------------------------------
# 5. pose accuracy of the three residuals, restatements only
# ---------------------------------------------------------------------------------------------
def test_gicp_ends_closer_to_the_true_pose_than_point_mode(pkg, orc):
    """make_pair(16384, 32768), one particle, 20 iterations, K = 20, max_dist = 1, delta = 0.1, normals of both clouds from 16
    neighbours, eps = 1e-3: the generalized-ICP restatement ends closer to true_pose than the point-mode oracle, in translation
    and in rotation.  Plane mode is measured beside it and not asserted on (the three figures are in DESIGN.md section 4.19)."""
    pair = pkg.scans.make_pair(16384, 32768)
    init = np.zeros((6, 1))
    o = orc.Solver(init, iterations=20, lr=1.0, max_dist=1.0, knn_count=20)
    o.add_cloud(pair.source, pair.target, init)
    o.stein_align()
    pt, pa = gr.pose_error(o.get_transformation(), pair.true_pose)
    nt, vt, _ = gr.normals(orc, pair.target, 16)
    ns, vs, _ = gr.normals(orc, pair.source, 16)
    r = pr.run(orc, pair.source, pair.target, nt, init, K=20, iterations=20, max_dist=1.0, delta=0.1)
    qt, qa = gr.pose_error(r.particles.reshape(6, 1)[:, 0], pair.true_pose)
    g = gr.run(orc, pair.source, pair.target, nt, ns, init, K=20, iterations=20, max_dist=1.0, delta=0.1, eps=1e-3)
    gt, ga = gr.pose_error(g.particles.reshape(6, 1)[:, 0], pair.true_pose)
    print(f"point mode {pt:.4e} m {pa:.4e} rad | plane {qt:.4e} m {qa:.4e} rad | gicp {gt:.4e} m {ga:.4e} rad | "
          f"normals valid: target {vt.mean():.4f}, source {vs.mean():.4f}")
    assert gt < pt and ga < pa


# ---------------------------------------------------------------------------------------------
# 6. the interface
# ---------------------------------------------------------------------------------------------
def test_new_interface_is_declared_exported_and_mirrored(pkg):
    declared = pkg.binding.declared_symbols()
    for name in NEW_EXPORTS:
        assert name in declared, f"include/svnicp_hip.h does not declare {name}"
    L = C.CDLL(pkg.binding.library_path())
    for name in NEW_EXPORTS:
        assert hasattr(L, name), f"libsvnicp_hip.so does not export {name}"
    prm = pkg.SteinICPParam()
    assert (prm.residual, prm.huber_delta, prm.normal_k, prm.gicp_epsilon) == ("point", 0.1, 16, 1e-3)
    for m in ("set_residual", "set_source_normals", "get_source_normals", "get_gicp_stats"):
        assert callable(getattr(pkg.SVNICP, m))
    assert pkg.binding.abi_version() == 1
    hdr = open(pkg.binding._HEADER).read()
    assert "#define SVNICP_RESIDUAL_GICP 2" in hdr
    shim = open(os.path.join(ROOT, "svn-icp_amd", "host", "svnicp_hip_shim.hpp")).read()
    for name in NEW_EXPORTS:
        assert name in shim, f"svnicp_hip_shim.hpp does not call {name}"
    cfg = pkg.pipeline.PipelineConfig(gpu_map=True, map_normals=True, solver=pkg.SteinICPParam(residual="gicp"))
    assert cfg.map_normals and cfg.solver.residual == "gicp"
    with pytest.raises(ValueError):
        pkg.pipeline.PipelineConfig(gpu_map=True, map_normals=True, solver=pkg.SteinICPParam(residual="point"))
