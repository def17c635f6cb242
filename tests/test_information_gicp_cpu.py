"""The GICP form of the information matrix without a device (svnicp_eval_information_gicp): the numpy
restatement (tests/information_gicp_reference.py) against mpmath on crafted rows and against the point and plane forms where
they must coincide, the host solve with form 3, the per-row function and the solve as a stand-alone program under the address
and undefined-behaviour sanitizers, the new interface, and the pipelines' switch.

Bounds.  Every entry of H and b is held to TIGHT = 1e-9 of A, the sum of the entry's absolute terms taken with |W|.  The one
expression that is not a handful of products is the closed-form inverse behind W: its relative error is a few cond(S) u with
cond(S) <= 1 / eps <= 1e6 and u = 1.1e-16, so at most about 1.2e-10: inside TIGHT at the smallest admitted epsilon."""
import ctypes as C
import os
import shutil
import subprocess

import mpmath
import numpy as np
import pytest

from helpers import TIGHT

import evaluate_cases as ec
import evaluate_reference as er
import gicp_reference as gr
import information_gicp_reference as igr
import information_reference as ir
import plane_reference as pr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "svn-icp_amd", "csrc")
INF = float("inf")
U = 2.0 ** -53
EPSILONS = (1e-3, 1e-6, 1.0)
DELTA_EXACT = 5.0 / 32.0           # |(3, 4, 0) / 32|: a pair exactly at rho = delta when W = I


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def crafted_rows():
    """(R [3, 3], s, e, nq, ns [N, 3]): per group of four rows the normals are parallel, antiparallel, perpendicular and nearly
    parallel (1e-7 rad apart: with eps = 1e-6 the sum S has its worst admitted condition, 1e6); residuals from 1 mm to 0.4 m, so
    that both Huber branches are taken at delta = 5 / 32; the last row has R^T e = (3, 4, 0) / 32 exactly."""
    rng = np.random.default_rng(29)
    R = gr_exp(np.array([0.3, -0.2, 0.5]))
    G = 6
    m = _unit(rng.standard_normal((G, 3)))
    perp = _unit(np.cross(m, rng.standard_normal((G, 3))))
    near = _unit(m + 1e-7 * perp)
    ns = np.stack([m, -m, perp, near], axis=1).reshape(-1, 3)          # source normals, source frame
    nq = np.repeat(m, 4, axis=0) @ R.T                                 # rows R m: so that R^T n_q = m to rounding
    s = rng.uniform(-20, 20, (4 * G, 3))
    e = _unit(rng.standard_normal((4 * G, 3))) * np.geomspace(1e-3, 0.4, 4 * G)[:, None]
    s = np.concatenate([s, [[1.5, -2.0, 0.25]]])
    e = np.concatenate([e, [R @ (np.array([3.0, 4.0, 0.0]) / 32.0)]])
    nq = np.concatenate([nq, [R @ np.array([0.0, 0.0, 1.0])]])
    ns = np.concatenate([ns, [[0.0, 1.0, 0.0]]])
    return R, s, e, nq, ns


def gr_exp(w):
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(a) / a * K + (1 - np.cos(a)) / a ** 2 * K @ K


def _mp_sums(R, s, e, nq, ns, delta, eps):
    """H [6, 6], b [6] of the header's terms at 50 digits, the inverse by mpmath."""
    mp = mpmath
    mp.mp.dps = 50
    Rm = mp.matrix(R.tolist())
    H, b = mp.zeros(6, 6), mp.zeros(6, 1)
    eps_m, a = mp.mpf(eps), 1 - mp.mpf(eps)
    for k in range(s.shape[0]):
        u = Rm.T * mp.matrix(e[k].tolist())
        m = Rm.T * mp.matrix(nq[k].tolist())
        n = mp.matrix(ns[k].tolist())
        S = 2 * mp.eye(3) - a * (m * m.T + n * n.T)
        W = 2 * eps_m * S ** -1
        rho = mp.sqrt((u.T * W * u)[0])
        w = mp.mpf(1) if (delta == INF or rho <= mp.mpf(delta)) else mp.mpf(delta) / rho
        sx = s[k].tolist()
        hat = mp.matrix([[0, -sx[2], sx[1]], [sx[2], 0, -sx[0]], [-sx[1], sx[0], 0]])
        G = mp.zeros(3, 6)
        for i in range(3):
            G[i, i] = 1
            for j in range(3):
                G[i, 3 + j] = -hat[i, j]
        H += w * (G.T * W * G)
        b += w * (G.T * W * u)
    return np.array(H.tolist(), dtype=float), np.array(b.tolist(), dtype=float).reshape(6)


@pytest.mark.parametrize("delta", [DELTA_EXACT, INF])
@pytest.mark.parametrize("eps", EPSILONS)
def test_restatement_against_mpmath_on_crafted_rows(eps, delta):
    R, s, e, nq, ns = crafted_rows()
    H, b, sum_w, sum_wr2, A_H, A_b, w, rho = igr.row_sums(R, s, e, nq, ns, delta, eps)
    Hm, bm = _mp_sums(R, s, e, nq, ns, delta, eps)
    S = gr.surface_sum(nq @ R, ns, eps)
    # eps = 1: W = I, the off-diagonal entries of H's translation block have no term at all (A = 0) and must be exact zeros
    ratio = max(np.max(np.abs(H - Hm) / np.where(A_H > 0, A_H, 1.0)), np.max(np.abs(b - bm) / A_b))
    print(f"eps {eps:g} delta {delta}: max cond(S) {np.linalg.cond(S).max():.3e}  largest |restatement - mpmath| / A = {ratio:.3e} "
          f"(TIGHT {TIGHT:g})  weights below 1: {(w < 1).sum()} of {w.size}")
    assert np.all(A_H > 0) == (eps != 1.0) and np.all(A_b > 0)
    assert np.all(np.abs(H - Hm) <= TIGHT * A_H) and np.all(np.abs(b - bm) <= TIGHT * A_b)
    if eps == 1e-6:
        assert np.linalg.cond(S).max() > 0.9e6, "the nearly parallel rows must reach the worst admitted condition"
    if eps == 1.0:
        assert rho[-1] == DELTA_EXACT and w[-1] == 1.0, "the last row sits exactly on delta, inside"
    if delta != INF:
        assert 0 < (w < 1).sum() < w.size, "both Huber branches"
    else:
        assert sum_w == w.size


# ------------------------------------------------------------------------------------------------ identities
_SCENE = {}


def _scene(pkg, orc):
    """The evaluate tests' "random" clouds at the true pose, gate 0.3, normals of both clouds from 16 neighbours; every seventh
    source row and every ninth target row made bare.  Shared, never changed."""
    if not _SCENE:
        src, tgt, poses = ec.clouds(pkg, "random")
        nt, ns = pr.normals(orc, tgt, 16)[0].copy(), pr.normals(orc, src, 16)[0].copy()
        nt[::9] = 0.0
        ns[::7] = 0.0
        T = poses["true_pose"]
        _SCENE.update(src=src, tgt=tgt, nt=nt, ns=ns, T=T, ev=er.evaluate(orc, src, tgt, T, 0.3, normals=nt))
    return _SCENE


def test_rows_are_the_plane_inliers_with_a_source_normal(pkg, orc):
    c = _scene(pkg, orc)
    S = igr.sums(orc, c["src"], c["tgt"], c["T"], 0.3, 0.1, 1e-3, c["nt"], c["ns"], ev=c["ev"])
    P = ir.sums(orc, c["src"], c["tgt"], c["T"], 0.3, "plane", 0.1, normals=c["nt"], ev=c["ev"])
    assert np.array_equal(S.rows, P.rows & (c["ns"] != 0).any(axis=1))
    assert 0 < S.pairs < P.pairs == c["ev"].plane_inliers
    assert np.array_equal(S.H, S.H.T) or np.all(np.abs(S.H - S.H.T) <= TIGHT * S.A_H)
    lo, hi = np.arange(len(c["src"])) < 1000, np.arange(len(c["src"])) >= 1000
    a, b = (igr.sums(orc, c["src"], c["tgt"], c["T"], 0.3, 0.1, 1e-3, c["nt"], c["ns"], ev=c["ev"], rows=m) for m in (lo, hi))
    assert a.pairs + b.pairs == S.pairs and min(a.pairs, b.pairs) > 0            # row shards add up
    assert np.all(np.abs(a.H + b.H - S.H) <= TIGHT * S.A_H) and np.all(np.abs(a.b + b.b - S.b) <= TIGHT * S.A_b)


@pytest.mark.parametrize("delta", [0.1, INF])
def test_epsilon_one_is_the_point_form_on_the_same_rows(pkg, orc, delta):
    """eps = 1: W = I exactly, rho = |R^T e| = sqrt(d2) to rounding (the Huber weight is continuous): H and b of the point form."""
    c = _scene(pkg, orc)
    S = igr.sums(orc, c["src"], c["tgt"], c["T"], 0.3, delta, 1.0, c["nt"], c["ns"], ev=c["ev"])
    Q = ir.sums(orc, c["src"], c["tgt"], c["T"], 0.3, "point", delta, ev=c["ev"], rows=S.rows)
    assert Q.pairs == S.pairs > 500
    scale = np.where(Q.A_H > 0, Q.A_H, 1.0)
    print(f"delta {delta}: max |dH| / A {np.max(np.abs(S.H - Q.H) / scale):.3e}  max |db| / A {np.max(np.abs(S.b - Q.b) / Q.A_b):.3e}")
    assert np.all(np.abs(S.H - Q.H) <= TIGHT * Q.A_H) and np.all(np.abs(S.b - Q.b) <= TIGHT * Q.A_b)
    assert abs(S.sum_w - Q.sum_w) <= TIGHT * Q.sum_w and abs(S.sum_wr2 - Q.sum_wr2) <= TIGHT * Q.sum_wr2


@pytest.mark.parametrize("eps", [1e-3, 0.1])
def test_parallel_normals_blend_the_plane_and_the_point_form(pkg, orc, eps):
    """n_s = R^T n_q for every row, delta = +inf: W = (1 - eps) m m^T + eps I, so H = (1 - eps) H_plane + eps H_point.
    Bound: the closed-form inverse carries 16 cond(S) u <= 16 u / eps relative (tests/test_gicp_cpu.py), and |m|^2 = 1 + a few u
    moves the eigenvalue 2 eps of S by the same order; 64 u / eps of A covers both."""
    c = _scene(pkg, orc)
    R = c["T"][:3, :3]
    j = np.where(c["ev"].index >= 0, c["ev"].index, 0)
    ns = c["nt"][j] @ R
    S = igr.sums(orc, c["src"], c["tgt"], c["T"], 0.3, INF, eps, c["nt"], ns, ev=c["ev"])
    P = ir.sums(orc, c["src"], c["tgt"], c["T"], 0.3, "plane", INF, normals=c["nt"], ev=c["ev"])
    Q = ir.sums(orc, c["src"], c["tgt"], c["T"], 0.3, "point", INF, ev=c["ev"], rows=P.rows)
    assert S.pairs == P.pairs == Q.pairs > 500
    want = (1.0 - eps) * P.H + eps * Q.H
    A = (1.0 - eps) * P.A_H + eps * Q.A_H
    tol = 64.0 * U / eps
    print(f"eps {eps:g}: max |H - blend| / A {np.max(np.abs(S.H - want) / A):.3e} (bound {tol:.3e})")
    assert np.all(np.abs(S.H - want) <= tol * A)


# ------------------------------------------------------------------------------------------------ the host solve, form 3
def test_solve_accepts_the_gicp_form_with_three_residuals_per_pair(pkg, orc):
    c = _scene(pkg, orc)
    S = igr.sums(orc, c["src"], c["tgt"], c["T"], 0.3, 0.1, 1e-3, c["nt"], c["ns"], ev=c["ev"])
    got = pkg.information_solve("gicp", S.pairs, S.sum_wr2, S.H, S.b)
    want = igr.solve("gicp", S.pairs, S.sum_wr2, S.H, S.b)
    top = want.eigval[5]
    assert got.form == "gicp" and got.rank == want.rank == 6 and want.dof == 3 * S.pairs - 6
    assert np.all(np.abs(got.eigval - want.eigval) <= 1e-12 * top)
    assert abs(got.sigma2 - want.sigma2) <= 1e-12 * want.sigma2 and got.sigma2 > 0
    assert abs(got.sigma2 - S.sum_wr2 / (3 * S.pairs - 6)) <= 1e-15 * got.sigma2
    assert np.all(np.abs(got.step - want.step) <= 1e-9 * np.linalg.norm(want.step))
    assert np.all(np.abs(got.cov - want.cov) <= 1e-9 * np.linalg.norm(want.cov))
    same = pkg.information_solve(3, S.pairs, S.sum_wr2, S.H, S.b)
    assert same.form == "gicp" and same.step.tobytes() == got.step.tobytes()
    plane = pkg.information_solve("plane", S.pairs, S.sum_wr2, S.H, S.b)          # the other forms keep their dim
    assert abs(plane.sigma2 - S.sum_wr2 / (S.pairs - 6)) <= 1e-15 * plane.sigma2


def test_solve_of_a_zero_matrix_has_rank_zero_and_no_nan(pkg):
    z = pkg.information_solve("gicp", 0, 0.0, np.zeros((6, 6)), np.zeros(6))
    assert z.form == "gicp" and z.rank == 0 and z.sigma2 == 0
    for f in ("eigval", "step", "cov"):
        assert not np.any(getattr(z, f)), f
    for f in ("eigvec", "vec_t", "vec_r", "eig_t", "eig_r"):
        assert np.isfinite(getattr(z, f)).all(), f


def test_form_two_stays_unknown(pkg):
    with pytest.raises(pkg.SvnIcpError):
        pkg.information_solve(2, 10, 1.0, np.eye(6), np.zeros(6))
    with pytest.raises(pkg.SvnIcpError):
        pkg.information_solve(4, 10, 1.0, np.eye(6), np.zeros(6))


# ------------------------------------------------------------------------------------------------ the stand-alone program
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    d = tmp_path_factory.mktemp("information_gicp")
    exe = d / "information_gicp_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-I", CSRC, os.path.join(HERE, "information_gicp_driver.cpp"), "-o", str(exe)], check=True)

    def run(groups):
        """groups: [(R, eps, delta, on [N], s, e, nq, ns)] -> [(sums [30], rc, solved fields or None)]."""
        lines = []
        for R, eps, delta, on, s, e, nq, ns in groups:
            lines.append("P " + " ".join(float(x).hex() for x in [*np.ravel(R), eps, delta]))
            for k in range(len(on)):
                lines.append(" ".join(float(x).hex() for x in [on[k], *s[k], *e[k], *nq[k], *ns[k]]))
            lines.append("=")
        (d / "cases.txt").write_text("\n".join(lines) + "\n")
        r = subprocess.run([str(exe), str(d / "cases.txt")], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr        # a sanitizer report goes to stderr and aborts the program
        out, it = [], iter(r.stdout.splitlines())
        for _ in groups:
            sums = np.array([float.fromhex(x) for x in next(it).split()])
            head = next(it).split()
            assert head[0] == "rc" and sums.shape == (30,)
            v = [float.fromhex(x) for x in head[3:]]
            out.append((sums, int(head[1]), None if int(head[1]) else dict(rank=int(head[2]), sigma2=v[0], step=np.array(v[1:7]), eigval=np.array(v[7:13]))))
        return out
    return run


def _expand(sums):
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = sums[3:24]
    return H + np.triu(H, 1).T, sums[24:30]


def test_program_agrees_with_the_restatement(pkg, orc, driver):
    """The crafted rows at every epsilon and both deltas, and the scene's rows (bare rows and rows off the gate included, passed
    with on = evaluate's inlier flag): sums within TIGHT of A, counts exact, the solve against numpy."""
    R, s, e, nq, ns = crafted_rows()
    groups, wants = [], []
    for eps in EPSILONS:
        for delta in (DELTA_EXACT, INF):
            groups.append((R, eps, delta, np.ones(len(s)), s, e, nq, ns))
            wants.append((len(s),) + igr.row_sums(R, s, e, nq, ns, delta, eps)[:6])
    c = _scene(pkg, orc)
    T = c["T"]
    j = np.where(c["ev"].index >= 0, c["ev"].index, 0)
    inl = (c["ev"].index >= 0) & (c["ev"].d2 < 0.09)
    e_all = orc.transform(c["src"], T[:3, :3], T[:3, 3]) - c["tgt"][j]
    S = igr.sums(orc, c["src"], c["tgt"], T, 0.3, 0.1, 1e-3, c["nt"], c["ns"], ev=c["ev"])
    groups.append((T[:3, :3], 1e-3, 0.1, inl.astype(float), c["src"], e_all, c["nt"][j], c["ns"]))
    wants.append((S.pairs, S.H, S.b, S.sum_w, S.sum_wr2, S.A_H, S.A_b))
    assert 0 < S.pairs < inl.sum() <= len(inl)
    for (sums, rc, solved), (pairs, H, b, sum_w, sum_wr2, A_H, A_b) in zip(driver(groups), wants):
        gH, gb = _expand(sums)
        print(f"pairs {int(sums[0])}: max |dH| / A {np.max(np.abs(gH - H) / np.where(A_H > 0, A_H, 1.0)):.3e}  max |db| / A {np.max(np.abs(gb - b) / A_b):.3e}")
        assert sums[0] == pairs and rc == 0
        assert abs(sums[1] - sum_w) <= TIGHT * sum_w and abs(sums[2] - sum_wr2) <= TIGHT * sum_wr2
        assert np.all(np.abs(gH - H) <= TIGHT * A_H) and np.all(np.abs(gb - b) <= TIGHT * A_b)
        want = igr.solve("gicp", pairs, sums[2], gH, gb)
        assert solved["rank"] == want.rank
        assert np.all(np.abs(solved["eigval"] - want.eigval) <= 1e-12 * want.eigval[5])
        assert abs(solved["sigma2"] - want.sigma2) <= 1e-12 * want.sigma2
        if want.eigval[0] / want.eigval[5] >= 1e-4:        # step divides by the retained eigenvalues (tests/test_information_cpu.py)
            assert np.all(np.abs(solved["step"] - want.step) <= 1e-9 * np.linalg.norm(want.step))


def test_program_selects_rejected_rows_to_zero(driver):
    """Rows that do not contribute — not an inlier, a zero target normal, a zero source normal — with NaN and inf operands: the
    record is exact zeros, and a group of nothing else solves to rank 0."""
    nan = float("nan")
    R = gr_exp(np.array([0.1, 0.2, -0.1]))
    z, n1 = [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]
    rows = [(0.0, [nan, 1, 2], [INF, 0, 0], n1, n1),
            (1.0, [1, nan, 2], [0.1, nan, 0], z, n1),
            (1.0, [1, 2, INF], [nan, 0.1, 0], n1, z),
            (0.0, [1e300, 1e300, 1e300], [1e300, 1e300, 1e300], n1, n1)]
    on, s, e, nq, ns = (np.array(x, float) for x in zip(*rows))
    (sums, rc, solved), = driver([(R, 1e-3, 0.1, on, s, e, nq, ns)])
    assert not np.any(sums) and np.isfinite(sums).all()
    assert rc == 0 and solved["rank"] == 0 and solved["sigma2"] == 0 and not np.any(solved["step"])


# ------------------------------------------------------------------------------------------------ interface
def test_new_interface_is_declared_and_the_struct_is_unchanged(pkg, tmp_path):
    from svnicp_amd.binding import InformationStruct, INFO_POINT, INFO_PLANE, INFO_GICP
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "svnicp_hip.h"\nint main(void) {\n'
                   '  int (*f)(svnicp_ctx *, double, double, double, svnicp_information *) = svnicp_eval_information_gicp; (void)f;\n'
                   '  printf("%d %d %d %zu\\n", SVNICP_INFO_POINT, SVNICP_INFO_PLANE, SVNICP_INFO_GICP, sizeof(svnicp_information));\n  return 0;\n}\n')
    obj = tmp_path / "probe.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)])
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", str(obj), pkg.library_path(), "-Wl,-rpath," + os.path.dirname(pkg.library_path()), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [INFO_POINT, INFO_PLANE, INFO_GICP, C.sizeof(InformationStruct)] and INFO_GICP == 3
    assert C.sizeof(InformationStruct) == 1368           # as before this form existed
    assert pkg.abi_version() == 1
    assert "svnicp_eval_information_gicp" in set(pkg.declared_symbols())
    assert pkg.load_library().svnicp_eval_information_gicp.argtypes is not None


# ------------------------------------------------------------------------------------------------ pipelines
def test_pipeline_accepts_the_gicp_form_only_with_the_gicp_residual(pkg):
    pl = pkg.pipeline
    gicp = pkg.SteinICPParam(iterations=20, lr=1.0, max_dist=1.0, KNN_count=100, residual="gicp")
    cfg = pl.PipelineConfig(information="gicp", eval_dist=0.5, solver=gicp)
    assert cfg.information == "gicp" and cfg.info_huber == INF
    for residual in ("point", "plane"):
        with pytest.raises(ValueError, match='information "gicp" needs solver.residual == "gicp"'):
            pl.PipelineConfig(information="gicp", eval_dist=0.5, solver=pkg.SteinICPParam(residual=residual))
    with pytest.raises(ValueError, match="eval_dist"):
        pl.PipelineConfig(information="gicp", solver=gicp)
    with pytest.raises(ValueError, match="info_huber"):
        pl.PipelineConfig(information="gicp", eval_dist=0.5, info_huber=0.0, solver=gicp)
    for form in ("point", "plane"):                        # the other forms stay the caller's choice in GICP mode
        assert pl.PipelineConfig(information=form, eval_dist=0.5, solver=gicp).information == form


def test_cpp_pipeline_has_the_same_switch():
    """registration_pipeline.hpp compiled on the host: the constructor's checks run before anything touches a device."""
    text = open(os.path.join(ROOT, "svn-icp_amd", "host", "registration_pipeline.hpp")).read()
    assert 'information \\"gicp\\" needs solver.residual == \\"gicp\\"' in text
    shim = open(os.path.join(ROOT, "svn-icp_amd", "host", "svnicp_hip_shim.hpp")).read()
    assert "svnicp_eval_information_gicp" in shim and "information_gicp(" in shim
