"""The point-to-plane residual without a GPU: pins tests/plane_reference.py (the float64 numpy restatement the GPU tests
compare the device against) on its own, and the presence of the new interface."""
import ctypes as C

import numpy as np

import plane_reference as pr

NEW_EXPORTS = ("svnicp_set_residual", "svnicp_set_target_normals", "svnicp_get_target_normals", "svnicp_get_plane_stats")


def _exp(w):
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if a == 0:
        return np.eye(3), np.eye(3)
    R = np.eye(3) + np.sin(a) / a * K + (1 - np.cos(a)) / a ** 2 * K @ K
    J = np.eye(3) + (1 - np.cos(a)) / a ** 2 * K + (a - np.sin(a)) / a ** 3 * K @ K      # left Jacobian
    return R, J


def _huber(r, delta):
    ar = np.abs(r)
    return np.where(ar <= delta, 0.5 * r * r, delta * ar - 0.5 * delta * delta)


def test_record_is_gradient_and_gauss_newton_hessian_of_the_huber_cost(pkg, orc):
    """b = d/dxi sum rho(r(T Exp xi)) at xi = 0 by central differences (pairs and winners as at xi = 0), H = sum w j j^T +
    1e-6 I by an independent loop.

    Tolerance of the gradient, from the step h alone.  Along coordinate k, g(tau) = sum rho(r(tau e_k)).  A translation
    coordinate makes r linear; a rotation coordinate turns s about a unit axis, so |r'|, |r''|, |r'''| <= L := 1 + |s|.
    Away from the kink, rho'' <= 1, rho''' = 0 and |rho'| <= delta, so |g'''| <= 3 L² + delta L per pair and the central
    difference is off by at most h²/6 of that.  A pair whose |r| is within h L of delta may cross the kink inside the
    stencil: g' is Lipschitz with constant L² + delta L there, which bounds its error by h (L² + delta L).  Round-off:
    the two cost sums carry at most N eps cost each, divided by 2 h."""
    src, tgt = pkg.scans.random_clouds(512, 2048, seed=5)
    K, delta, max_dist, h = 8, 0.015, 0.003, 1e-6
    nrm, valid, _ = pr.normals(orc, tgt, 12)
    x6 = np.array([0.03, -0.02, 0.015, 0.004, -0.006, 0.005])
    R0 = _exp(np.array([0.002, 0.001, -0.003]))[0]
    t0 = np.array([0.01, 0.02, -0.01])
    Rt, tt = pr.total_pose(orc, x6, R0, t0)
    cand, _ = orc.knn_topk(orc.transform(src, R0, t0), tgt, K)
    rec, slot, stats, r0 = pr.record_one(src, tgt, nrm, cand, Rt, tt, max_dist, delta)
    _, ok, e, n = pr.pairs(src, tgt, nrm, cand, Rt, tt, max_dist)
    assert 0 < ok.sum() < src.shape[0], "the gate must reject some pairs and keep some"
    out = np.abs(r0) > delta
    assert 0.05 <= out.mean() <= 0.95, f"{out.mean():.3f} of the accepted pairs lie outside delta"
    s, q, n = src[ok], tgt[cand[np.arange(src.shape[0]), slot]][ok], n[ok]

    def cost(xi):
        dR, J = _exp(xi[3:])
        Rp, tp = Rt @ dR, tt + Rt @ (J @ xi[:3])          # T Exp(xi): the solver's right perturbation (SVNICP.cpp:268-279)
        r = (((s @ Rp.T) + tp - q) * n).sum(axis=1)
        return _huber(r, delta).sum()

    L = 1.0 + np.linalg.norm(s, axis=1)
    kink = np.abs(np.abs(r0) - delta) <= h * L
    tol = (h * h / 6.0) * (3 * L * L + delta * L).sum() + h * (L * L + delta * L)[kink].sum() \
        + len(r0) * np.finfo(float).eps * cost(np.zeros(6)) / h
    g = np.zeros(6)
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        g[k] = (cost(d) - cost(-d)) / (2 * h)
    err = np.abs(g - rec[36:]).max()
    print(f"gradient: max |central difference - b| = {err:.3e}, bound {tol:.3e}, |b| max {np.abs(rec[36:]).max():.3e}, "
          f"{kink.sum()} pairs at the kink")
    assert err <= tol
    assert tol < 1e-3 * np.abs(rec[36:]).max(), "the bound must be far below b itself, or the check shows nothing"
    H = 1e-6 * np.eye(6)
    for i in range(len(r0)):
        m = Rt.T @ n[i]
        j = np.concatenate([m, np.cross(s[i], m)])
        w = 1.0 if abs(r0[i]) <= delta else delta / abs(r0[i])
        H += w * np.outer(j, j)
    assert np.allclose(rec[:36].reshape(6, 6), H, rtol=1e-12, atol=1e-12)
    assert np.array_equal(rec[:36].reshape(6, 6), rec[:36].reshape(6, 6).T)
    assert stats[0] == ok.sum()


def test_plane_residual_halves_the_pose_error_of_point_mode(pkg, orc):
    """make_pair(16384, 32768), one particle, 20 iterations, K = 20, max_dist = 1, delta = 0.1, normals from 16 neighbours:
    the plane reference ends within half of the point-mode oracle's error to true_pose, in translation and in rotation.
    Measured: point mode 10.5 cm / 0.0120 rad, plane 5.9 mm / 4.8e-05 rad (18x and 250x)."""
    pair = pkg.scans.make_pair(16384, 32768)
    init = np.zeros((6, 1))
    o = orc.Solver(init, iterations=20, lr=1.0, max_dist=1.0, knn_count=20)
    o.add_cloud(pair.source, pair.target, init)
    o.stein_align()
    pt, pa = pr.pose_error(o.get_transformation(), pair.true_pose)
    nrm, valid, _ = pr.normals(orc, pair.target, 16)
    r = pr.run(orc, pair.source, pair.target, nrm, init, K=20, iterations=20, max_dist=1.0, delta=0.1)
    qt, qa = pr.pose_error(r.particles.reshape(6, 1)[:, 0], pair.true_pose)
    print(f"point mode {pt:.4e} m {pa:.4e} rad | plane {qt:.4e} m {qa:.4e} rad | normals valid {valid.mean():.4f}")
    assert qt <= 0.5 * pt and qa <= 0.5 * pa


def test_new_interface_is_declared_exported_and_mirrored(pkg):
    declared = pkg.binding.declared_symbols()
    for name in NEW_EXPORTS:
        assert name in declared, f"include/svnicp_hip.h does not declare {name}"
    L = C.CDLL(pkg.binding.library_path())
    for name in NEW_EXPORTS:
        assert hasattr(L, name), f"libsvnicp_hip.so does not export {name}"
    prm = pkg.SteinICPParam()
    assert (prm.residual, prm.huber_delta, prm.normal_k) == ("point", 0.1, 16)
    for m in ("set_residual", "set_target_normals", "get_target_normals", "get_plane_stats"):
        assert callable(getattr(pkg.SVNICP, m))
    assert pkg.binding.abi_version() == 1
    hdr = open(pkg.binding._HEADER).read()
    assert "#define SVNICP_RESIDUAL_POINT 0" in hdr and "#define SVNICP_RESIDUAL_PLANE 1" in hdr
