"""svnicp_eval_information / svnicp_information_solve without a device: the numpy restatement (tests/information_reference.py)
against Jacobians taken by central differences in mpmath, the figures the feature was specified with, the single-plane known
answer, the host solve (csrc/information_solve.hpp) as a stand-alone program under the address and undefined-behaviour
sanitizers and through the library, row shards, the ctypes mirror of struct svnicp_information and the host layers.

Bounds of the solve cases: Jacobi's eigenvalues carry an absolute error of about 6 u |H| (7e-16 |H|), so |d lambda| and
|H v - lambda v| are held to 1e-12 |H| and |V^T V - I| to 1e-13.  step and cov divide by the retained eigenvalues: their error
is u / (lambda_min / lambda_max) relative, and every retained ratio of these cases is at least 1e-4, so 1e-9 leaves five
orders of margin."""
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
import information_reference as ir
import plane_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("point", "plane")


# ------------------------------------------------------------------------------------------------ convention
def _mp_jacobians(mp, src, tgt, T, index, normals, rows):
    """{"point": J [n, 3, 6], "plane": J [n, 1, 6]} of the contributing rows: central differences of the residuals under
    T Exp(xi), xi = [v ; omega], at 50 digits (step 1e-20: truncation 1e-40)."""
    mp.mp.dps = 50
    R = mp.matrix(T[:3, :3].tolist())
    t = mp.matrix(T[:3, 3].tolist())
    h = mp.mpf(10) ** -20

    def exp_so3(w):
        th = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
        K = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        if th == 0:
            return mp.eye(3)
        return mp.eye(3) + (mp.sin(th) / th) * K + ((1 - mp.cos(th)) / th ** 2) * (K * K)

    def residuals(xi, s, p, n):
        # T Exp(xi): rotation R Exp(omega), translation t + R V(omega) v; one of v, omega is zero in every difference, so V v = v
        v, w = mp.matrix(xi[:3]), xi[3:]
        q = R * (exp_so3(w) * s + v) + t
        e = q - p
        c = R.T * e                                   # the point residual in the frame of the linearisation point
        return [c[0], c[1], c[2]], [n[0] * e[0] + n[1] * e[1] + n[2] * e[2]]

    out = {"point": [], "plane": []}
    for b in np.flatnonzero(rows):
        s, p = mp.matrix(src[b].tolist()), mp.matrix(tgt[index[b]].tolist())
        n = mp.matrix(normals[index[b]].tolist())
        Jp, Jn = [[0.0] * 6 for _ in range(3)], [[0.0] * 6]
        for k in range(6):
            xp, xm = [mp.mpf(0)] * 6, [mp.mpf(0)] * 6
            xp[k], xm[k] = h, -h
            (cp, rp), (cm, rm) = residuals(xp, s, p, n), residuals(xm, s, p, n)
            for d in range(3):
                Jp[d][k] = float((cp[d] - cm[d]) / (2 * h))
            Jn[0][k] = float((rp[0] - rm[0]) / (2 * h))
        out["point"].append(Jp)
        out["plane"].append(Jn)
    return {k: np.array(v) for k, v in out.items()}


@pytest.fixture(scope="module")
def convention(pkg, orc):
    mp = mpmath
    src, tgt = pkg.scans.random_clouds(300, 700, seed=3)
    T = pkg.pipeline.correction_to_pose([0.05, -0.03, 0.02, 0.004, -0.003, 0.006])
    nrm, _, _ = pr.normals(orc, tgt, 16)
    ev = er.evaluate(orc, src, tgt, T, 0.3, normals=nrm)
    rows = (ev.index >= 0) & (ev.d2 < 0.09)
    assert rows.sum() > 100
    return src, tgt, T, nrm, rows, _mp_jacobians(mp, src, tgt, T, ev.index, nrm, rows)


@pytest.mark.parametrize("delta", [0.1, float("inf")])
@pytest.mark.parametrize("form", FORMS)
def test_reference_equals_the_normal_equations_of_a_differenced_jacobian(orc, convention, form, delta):
    """b = J^T W r and H = J^T W J with J from central differences under T Exp([v ; omega]) and the weights frozen: pins the
    sign of b, the order of the tangent and the frame."""
    src, tgt, T, nrm, rows, Jmp = convention
    S = ir.sums(orc, src, tgt, T, 0.3, form, delta, normals=nrm)
    on, w, _, res, _ = ir.row_terms(orc, src, tgt, T, S.eval, 0.3, form, delta, nrm)
    sel = on[rows]                                     # the plane form drops rows whose target has no normal
    J = Jmp[form][sel]
    wv, r = w[on], res[on]
    H = np.einsum("b,bdi,bdj->ij", wv, J, J)
    b = np.einsum("b,bdi,bd->i", wv, J, r)
    assert S.pairs == int(on.sum()) > 100
    # an entry whose terms are all structurally zero (the point form's I block off its diagonal) has A = 0; the R of a float64
    # pose is orthogonal to a few u only, so the differenced J holds R^T R there: such an entry is measured against its row's
    # and column's diagonal scale
    scale = np.where(S.A_H > 0, S.A_H, np.sqrt(np.outer(np.diag(S.A_H), np.diag(S.A_H))))
    print(f"{form} delta {delta}: pairs {S.pairs}  max |dH| / A {np.max(np.abs(H - S.H) / scale):.3e}  max |db| / A {np.max(np.abs(b - S.b) / S.A_b):.3e}")
    assert np.all(np.abs(H - S.H) <= 1e-9 * scale) and np.all(np.abs(b - S.b) <= 1e-9 * S.A_b)
    assert S.sum_w == S.pairs if delta == float("inf") else S.sum_w <= S.pairs


# ------------------------------------------------------------------------------------------------ specified figures
@pytest.fixture(scope="module")
def pair(pkg, orc):
    src, tgt, poses = ec.clouds(pkg, "pair")
    nrm, _, _ = pr.normals(orc, tgt, 16)
    out = {}
    for pose in ("identity", "true_pose"):
        for form in FORMS:
            out[pose, form] = ir.sums(orc, src, tgt, poses[pose], 0.3, form, 0.1, normals=nrm)
    return src, tgt, poses, nrm, out


# (pose, form): eigenvalues of H — this restatement on scans.make_pair(2048, 8192), gate 0.3 m, Huber delta 0.1,
# plane_reference.normals(kn = 16), as the feature was specified
TABLE = {
    ("identity", "plane"): (106.690, 275.771, 1113.03, 21732.9, 27591.2, 34337.0),
    ("identity", "point"): (1370.59, 1405.21, 1457.65, 78413.8, 114180.0, 185256.0),
    ("true_pose", "plane"): (107.109, 348.216, 1190.43, 29653.7, 34246.5, 40856.0),
    ("true_pose", "point"): (1417.15, 1425.91, 1491.19, 80421.6, 90856.7, 163887.0),
}


@pytest.mark.parametrize("pose,form", sorted(TABLE))
def test_specified_figures(pair, pose, form):
    S = pair[4][pose, form]
    r = ir.solve(form, S.pairs, S.sum_wr2, S.H, S.b)
    print(f"{pose} {form}: pairs {S.pairs} sum_w {S.sum_w!r} eigval {r.eigval.tolist()} eig_t {r.eig_t.tolist()} "
          f"min/max {r.eigval[0] / r.eigval[5]:.3e}")
    assert S.pairs == (S.eval.inliers if form == "point" else S.eval.plane_inliers)
    assert r.eigval == pytest.approx(TABLE[pose, form], rel=1e-3)
    assert r.rank == 6 and r.eigval[0] / r.eigval[5] > 1e-4
    if form == "point":      # H_tt = sum_w I: this form cannot show a translational degeneracy
        assert np.all(np.abs(r.eig_t - S.sum_w) <= 1e-12 * S.sum_w)
    else:
        assert np.min(np.diff(r.eig_t)) > 1e-3 * r.eig_t[2]


# ------------------------------------------------------------------------------------------------ single plane
def single_plane(seed=17):
    """(source [300, 3] at z = 0.02, target [1200, 3] in z = 0, normals (0, 0, 1)): only z, roll and pitch are constrained."""
    rng = np.random.default_rng(seed)
    tgt = np.concatenate([rng.uniform(-5, 5, (1200, 2)), np.zeros((1200, 1))], axis=1)
    src = np.concatenate([rng.uniform(-4, 4, (300, 2)), np.full((300, 1), 0.02)], axis=1)
    nrm = np.tile([0.0, 0.0, 1.0], (1200, 1))
    return src, tgt, nrm


def check_single_plane(pairs, b, rank, eigval, eigvec, eig_t, step, cov):
    top = eigval[5]
    assert pairs == 300 and rank == 3
    assert np.all(np.abs(np.sort(eig_t) - [0.0, 0.0, 300.0]) <= 1e-12 * top)
    assert abs(b[2] - 300 * 0.02) <= TIGHT * 300 * 0.02
    assert abs(step[2] + 0.02) <= 1e-9
    null = eigvec[:3]
    assert np.all(np.abs(eigval[:3]) <= 1e-12 * top)
    assert np.all(np.abs(null @ step) <= 1e-12 * np.linalg.norm(step))
    assert np.all(np.abs(null @ cov) <= 1e-12 * max(np.linalg.norm(cov), 1e-300)) and np.all(np.abs(cov @ null.T) <= 1e-12 * max(np.linalg.norm(cov), 1e-300))


def test_single_plane_has_rank_three(pkg, orc):
    src, tgt, nrm = single_plane()
    S = ir.sums(orc, src, tgt, np.eye(4), 0.5, "plane", float("inf"), normals=nrm)
    r = ir.solve("plane", S.pairs, S.sum_wr2, S.H, S.b)
    check_single_plane(S.pairs, S.b, r.rank, r.eigval, r.eigvec, r.eig_t, r.step, r.cov)
    c = pkg.information_solve("plane", S.pairs, S.sum_wr2, S.H, S.b)
    check_single_plane(c.pairs, c.b, c.rank, c.eigval, c.eigvec, c.eig_t, c.step, c.cov)


# ------------------------------------------------------------------------------------------------ the host solve
@pytest.fixture(scope="module")
def solve_cases(pkg, orc, pair):
    """name -> (form, pairs, sum_wr2, floor, H [6, 6], b [6])."""
    cases = {}
    for (pose, form), S in pair[4].items():
        cases[f"{pose}-{form}"] = (form, S.pairs, S.sum_wr2, 0.0, S.H, S.b)
    src, tgt, nrm = single_plane()
    S = ir.sums(orc, src, tgt, np.eye(4), 0.5, "plane", float("inf"), normals=nrm)
    cases["rank3"] = ("plane", S.pairs, S.sum_wr2, 0.0, S.H, S.b)
    D = np.diag([2.0, 2.0, 2.0, 5.0, 5.0, 9.0])
    cases["diag"] = ("point", 10, 3.0, 0.0, D, np.arange(1.0, 7.0))
    cases["diag-floor-half"] = ("point", 10, 3.0, 0.5, D, np.arange(1.0, 7.0))
    cases["zero"] = ("plane", 0, 0.0, 0.0, np.zeros((6, 6)), np.zeros(6))
    S = pair[4]["true_pose", "plane"]
    cases["scaled-down"] = ("plane", S.pairs, S.sum_wr2, 0.0, S.H * 1e-30, S.b * 1e-30)
    cases["scaled-up"] = ("plane", S.pairs, S.sum_wr2, 0.0, S.H * 1e30, S.b * 1e30)
    return cases


_BAD = {"nan-in-H": (0, float("nan")), "inf-in-b": (36 + 2, float("inf"))}
_OUT = (("rank", 1), ("sigma2", 1), ("eigval", 6), ("eigvec", 36), ("eig_t", 3), ("vec_t", 9), ("eig_r", 3), ("vec_r", 9), ("step", 6), ("cov", 36))


@pytest.fixture(scope="module")
def driver_results(solve_cases, tmp_path_factory):
    """The stand-alone program's output per case: a dict of fields, or the refusal code."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    d = tmp_path_factory.mktemp("information_solve")
    exe = d / "information_solve_driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "svn-icp_amd", "csrc"), os.path.join(ROOT, "tests", "information_solve_driver.cpp"), "-o", str(exe)],
                   check=True)
    names, lines = [], []
    code = {"point": 0, "plane": 1}
    for name, (form, pairs, wr2, floor, H, b) in solve_cases.items():
        names.append(name)
        lines.append(" ".join(repr(float(x)) for x in [code[form], pairs, wr2, floor, *np.ravel(H), *np.ravel(b)]))
    form, pairs, wr2, floor, H, b = solve_cases["diag"]
    for name, (pos, val) in _BAD.items():
        hb = np.concatenate([np.ravel(H), np.ravel(b)])
        hb[pos] = val
        names.append(name)
        lines.append(" ".join(repr(float(x)) for x in [code[form], pairs, wr2, floor, *hb]))
    for name, head in (("floor-one", [0, 10, 3.0, 1.0]), ("floor-negative", [0, 10, 3.0, -0.1]), ("form-unknown", [2, 10, 3.0, 0.0])):
        names.append(name)
        lines.append(" ".join(repr(float(x)) for x in [*head, *np.ravel(H), *np.ravel(b)]))
    (d / "cases.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(d / "cases.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr          # a sanitizer report goes to stderr and aborts the program
    out, it = {}, iter(r.stdout.splitlines())
    for name in names:
        head = next(it).split()
        assert head[0] == "rc"
        if int(head[1]) != 0:
            out[name] = int(head[1])
            continue
        v = [float(x) for x in next(it).split()]
        assert len(v) == sum(n for _, n in _OUT)
        fields, k = {}, 0
        for f, n in _OUT:
            fields[f] = np.array(v[k:k + n]) if n > 1 else v[k]
            k += n
        for f in ("eigvec", "cov"):
            fields[f] = fields[f].reshape(6, 6)
        for f in ("vec_t", "vec_r"):
            fields[f] = fields[f].reshape(3, 3)
        fields["rank"] = int(fields["rank"])
        out[name] = fields
    return out


def _library_result(pkg, case):
    form, pairs, wr2, floor, H, b = case
    c = pkg.information_solve(form, pairs, wr2, H, b, eig_floor_ratio=floor)
    return {f: getattr(c, f) for f, _ in _OUT}


def _check_solve(name, got, case):
    form, pairs, wr2, floor, H, b = case
    want = ir.solve(form, pairs, wr2, H, b, floor)
    S = 0.5 * H + 0.5 * H.T
    top = max(want.eigval[5], 0.0)
    for vals, vecs, ref, M in ((got["eigval"], got["eigvec"], want.eigval, S), (got["eig_t"], got["vec_t"], want.eig_t, S[:3, :3]),
                               (got["eig_r"], got["vec_r"], want.eig_r, S[3:, 3:])):
        n = len(vals)
        assert np.all(np.diff(vals) >= 0), name
        assert np.all(np.abs(vals - ref) <= 1e-12 * top), (name, vals, ref)
        for lam, v in zip(vals, vecs):
            assert np.linalg.norm(M @ v - lam * v) <= 1e-12 * top, name
            assert v[int(np.argmax(np.abs(v)))] > 0, (name, v)           # the sign rule
        assert np.max(np.abs(vecs @ vecs.T - np.eye(n))) <= 1e-13, name
    assert got["rank"] == want.rank, (name, got["rank"], want.rank)
    assert abs(got["sigma2"] - want.sigma2) <= 1e-12 * abs(want.sigma2), name
    assert np.all(np.abs(got["step"] - want.step) <= 1e-9 * np.linalg.norm(want.step)), name
    assert np.all(np.abs(got["cov"] - want.cov) <= 1e-9 * np.linalg.norm(want.cov)), name
    assert np.isfinite(np.concatenate([np.ravel(np.asarray(v, float)) for v in got.values()])).all(), name
    return want


_CASE_NAMES = ("identity-point", "identity-plane", "true_pose-point", "true_pose-plane", "rank3", "diag", "diag-floor-half", "zero",
               "scaled-down", "scaled-up")
_RANKS = {"rank3": 3, "diag": 6, "diag-floor-half": 3, "zero": 0}


@pytest.mark.parametrize("via", ["program", "library"])
@pytest.mark.parametrize("name", _CASE_NAMES)
def test_solve_against_numpy(pkg, solve_cases, driver_results, name, via):
    case = solve_cases[name]
    got = driver_results[name] if via == "program" else _library_result(pkg, case)
    want = _check_solve(name, got, case)
    if name in _RANKS:
        assert got["rank"] == _RANKS[name]
    else:
        assert got["rank"] == 6 and want.eigval[0] / want.eigval[5] >= 1e-4
    if name == "zero":
        assert got["sigma2"] == 0 and not np.any(got["step"]) and not np.any(got["cov"]) and not np.any(got["eigval"])
    if name == "diag-floor-half":        # eigenvalues 2 lie below 0.5 * 9, the fives above
        assert np.all(got["step"][:3] == 0) and np.all(got["step"][3:] != 0)


@pytest.mark.parametrize("via", ["program", "library"])
def test_solve_is_scale_invariant(pkg, solve_cases, driver_results, via):
    """H in other units: the rank and the eigenvectors do not change, the eigenvalues scale."""
    res = {n: (driver_results[n] if via == "program" else _library_result(pkg, solve_cases[n])) for n in ("true_pose-plane", "scaled-down", "scaled-up")}
    base = res["true_pose-plane"]
    for n, k in (("scaled-down", 1e-30), ("scaled-up", 1e30)):
        assert res[n]["rank"] == base["rank"] == 6
        assert np.max(np.abs(res[n]["eigvec"] - base["eigvec"])) <= 1e-12
        assert np.allclose(res[n]["eigval"], base["eigval"] * k, rtol=1e-12, atol=0)
        assert np.allclose(res[n]["step"], base["step"], rtol=1e-9, atol=0)


def test_solve_refuses_bad_input(pkg, solve_cases, driver_results):
    for name in (*_BAD, "floor-one", "floor-negative", "form-unknown"):
        assert driver_results[name] == -1, name
    form, pairs, wr2, floor, H, b = solve_cases["diag"]
    bad = H.copy(); bad[2, 3] = np.nan
    with pytest.raises(pkg.SvnIcpError):
        pkg.information_solve(form, pairs, wr2, bad, b)
    with pytest.raises(pkg.SvnIcpError):
        pkg.information_solve(form, pairs, wr2, H, np.full(6, np.inf))
    for f in (1.0, -0.1, float("nan")):
        with pytest.raises(pkg.SvnIcpError):
            pkg.information_solve(form, pairs, wr2, H, b, eig_floor_ratio=f)
    with pytest.raises(pkg.SvnIcpError):
        pkg.information_solve(2, pairs, wr2, H, b)
    o = pkg.binding.InformationStruct()                # struct_size left 0
    assert pkg.load_library().svnicp_information_solve(C.byref(o)) == -1
    assert pkg.load_library().svnicp_information_solve(None) == -1


# ------------------------------------------------------------------------------------------------ shards
@pytest.mark.parametrize("form", FORMS)
def test_row_shards_add_up(pkg, orc, pair, form):
    src, tgt, poses, nrm, whole = pair
    W = whole["true_pose", form]
    lo, hi = np.arange(len(src)) < 1000, np.arange(len(src)) >= 1000
    a, b = (ir.sums(orc, src, tgt, poses["true_pose"], 0.3, form, 0.1, normals=nrm, rows=m) for m in (lo, hi))
    assert a.pairs + b.pairs == W.pairs and min(a.pairs, b.pairs) > 0
    H, g = a.H + b.H, a.b + b.b
    assert np.all(np.abs(H - W.H) <= TIGHT * W.A_H) and np.all(np.abs(g - W.b) <= TIGHT * W.A_b)
    assert abs(a.sum_w + b.sum_w - W.sum_w) <= TIGHT * W.sum_w and abs(a.sum_wr2 + b.sum_wr2 - W.sum_wr2) <= TIGHT * W.sum_wr2
    c = pkg.information_solve(form, a.pairs + b.pairs, a.sum_wr2 + b.sum_wr2, H, g)
    _check_solve(f"shards-{form}", {f: getattr(c, f) for f, _ in _OUT}, (form, W.pairs, W.sum_wr2, 0.0, W.H, W.b))


# ------------------------------------------------------------------------------------------------ struct, symbols, host layers
_FIELDS = ("struct_size", "form", "pairs", "rank", "reserved", "huber_delta", "eig_floor_ratio", "max_corr_dist", "sum_w", "sum_wr2",
           "sigma2", "H", "b", "eigval", "eigvec", "eig_t", "vec_t", "eig_r", "vec_r", "step", "cov", "R", "t")


def test_information_struct_matches_header(pkg, tmp_path):
    from svnicp_amd.binding import InformationStruct, INFO_POINT, INFO_PLANE
    src = tmp_path / "probe.c"
    body = "".join(f'  printf("%zu\\n", offsetof(svnicp_information, {f}));\n' for f in _FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svnicp_hip.h"\nint main(void) {\n'
                   '  printf("%d\\n%d\\n%zu\\n", SVNICP_INFO_POINT, SVNICP_INFO_PLANE, sizeof(svnicp_information));\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert [name for name, _ in InformationStruct._fields_] == list(_FIELDS)
    assert got == [INFO_POINT, INFO_PLANE, C.sizeof(InformationStruct)] + [getattr(InformationStruct, f).offset for f in _FIELDS]
    assert pkg.abi_version() == 1


def test_binding_declares_the_information_symbols(pkg):
    names = ("svnicp_eval_information", "svnicp_information_solve")
    assert set(names) <= set(pkg.declared_symbols())
    L = pkg.load_library()
    for n in names:
        assert getattr(L, n).argtypes is not None, n
    assert hasattr(pkg.SVNICP, "information") and hasattr(pkg.SVGDICP, "information") and callable(pkg.information_solve)
    assert pkg.RegistrationInformation.__dataclass_fields__.keys() >= {"H", "b", "eigval", "eigvec", "eig_t", "eig_r", "rank", "step", "cov", "pairs", "pose"}


def test_pipeline_information_is_off_by_default_and_needs_an_evaluate(pkg):
    pl = pkg.pipeline
    assert pl.PipelineConfig().information == "off"
    for kw in (dict(information="plane"), dict(information="point", eval_dist=0.0), dict(information="both", eval_dist=0.5),
               dict(information="plane", eval_dist=0.5, info_huber=0.0)):
        with pytest.raises(ValueError):
            pl.PipelineConfig(**kw)
    assert pl.PipelineConfig(information="plane", eval_dist=0.5).info_huber == float("inf")
    pipe = pl.RegistrationPipeline(pl.PipelineConfig(voxel_size=0.5, map_voxel_size=0.5))
    pts = pkg.scans.lidar_scan(pkg.scans.make_scene(), np.eye(3), np.zeros(3), 4096, stream=700)
    res = pipe.process_scan(pts, 0.0)           # the first scan seeds the host map: no solver, no device
    assert res.state is None and res.information is None
