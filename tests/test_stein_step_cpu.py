"""The cases and the reference of tests/test_stein_step_gpu.py, pinned on the CPU before any GPU run.

* every case builds, i.e. reaches the regime it claims (the assertions live in tests/stein_step_cases.py);
* tests/golden/stein_step.npz is current: regenerating it with mpmath gives the same bytes for every array;
* the float64 oracle, used piecewise (oracle_step of tests/golden/make_stein_step.py: so3_exp, orc_sp_update on [P][42]
  records; solve6, so3_exp, so3_log directly; for the SVGD-ICP cases, where the oracle has no split-phase entry, the plain
  float64 step of tests/stein_step_reference.py), agrees with mpmath: the same stop decisions, non-finite patterns and median
  keys, E_oracle <= 1e-6 on every comparison and <= 1e-13 on the well-conditioned cases;
* sensitivity: a plain float64 step that is wrong in ONE detail is rejected by a named case under the bar the GPU test
  applies, 16 max(E_oracle, 2^-52), or by one of its exact comparisons — and the right float64 step is not.

Two things the issue asked for are answered differently, with the reason:
  - "Log without clamp" cannot be rejected by any input: where 0.5 (trace - 1) leaves [-1, 1], acos gives NaN, |sin NaN| >
    1e-12 is false and Log returns zeros; with the clamp, acos gives 0 or pi, |sin| <= 1e-12 and Log returns zeros as well.
    test_log_clamp_is_redundant pins that equivalence on the two cases that reach the clamp instead.
  - |phi_r| = pi - 1e-6 cannot have E_oracle <= 1e-6: the reference's Log forms 1 + cos there, 5e-13, from entries rounded
    at 1.1e-16, so sin(acos(.)) and with it the rotation vector carry 2e-4.  The case stays; only its whole pose and history
    row follow the measured E_oracle, the translation rows alone (quantity pose_t), phi, N, H and b meet the condition;
    exp_pi-1e-4 is the nearest step that meets it throughout.
"""
import importlib.util
import os

import numpy as np
import pytest

import stein_step_cases as cases
import stein_step_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_stein_step", os.path.join(HERE, "golden", "make_stein_step.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)

FACTOR, EPS = 16.0, 2.0 ** -52
CONDITION_EXCEPTIONS = {"exp_pi-1e-6_p1", "exp_pi-1e-6_p3"}   # see the module docstring


@pytest.fixture(scope="module")
def fixture():
    return mk.load()


def test_cases_build_and_claim_a_regime():
    cs = cases.all_cases()
    assert len(cs) >= 90 and all(c.regime for c in cs)
    for tag in ("lu", "exp", "median", "dir", "es", "shard", "svgd", "opt", "seq"):
        assert any(tag in c.tags for c in cs), tag
    for c in cs:
        assert c.sums.shape == (c.W, c.P, 22) and c.init.shape == (6, c.P)
        assert len(cases.shapes(c.P)) == (1 if c.P == 1 else 4 if c.P <= 128 else 2)


def test_fixture_is_current(orc, fixture):
    fresh = mk.generate(orc)
    assert sorted(fresh) == sorted(fixture)
    for k in fresh:
        a, b = np.asarray(fresh[k]), fixture[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    others = [os.path.getsize(os.path.join(HERE, "golden", f)) for f in os.listdir(os.path.join(HERE, "golden"))
              if f.endswith(".npz") and f != os.path.basename(mk.FIXTURE)]
    assert os.path.getsize(mk.FIXTURE) <= max(others), "larger than the largest other fixture under tests/golden"


@pytest.mark.parametrize("case", cases.all_cases(), ids=lambda c: c.name)
def test_oracle_agrees_with_reference(orc, fixture, case):
    r = mk.case_reference(fixture, case)
    assert r["chk"] == int(case.checksum()), "tests/golden/stein_step.npz is stale: run tests/golden/make_stein_step.py"
    o = mk.oracle_step(orc, case)
    assert o["stop"] == r["stop"] and o["iters"] == (1 if r["stop"] else mk.ITER)
    if r["stop"]:
        assert not o["hist"].any()
    if case.exact_h:
        assert ref.same_median(o["h"], r["med"], case.P), (o["h"], r["med"])
        if case.P > 1 and "sq" in case.info:
            assert np.array_equal(np.float64(case.info["lower"]), r["med"], equal_nan=True)
    got = mk.subset(o, r["idx"])
    for q in ref.QUANTITIES:
        if r.get(q) is None:
            continue
        v, w = ref.compared(got, q), ref.compared(r, q)
        e = ref.rel_err(v, w)
        assert e is not None, q + ": non-finite pattern"
        assert e.max() == r["eo"][q], q                    # the fixture's yardstick is this oracle's error
        if not (case.name in CONDITION_EXCEPTIONS and q in ("pose", "hist")):   # (pose_t, the translation rows, stays held)
            assert r["eo"][q] <= 1e-6, (q, r["eo"][q])
        if case.well:
            assert r["eo"][q] <= 1e-13, (q, r["eo"][q])


def test_oracle_pieces_against_mpmath(orc):
    """solve6 on the pivoting matrices, so3_exp and so3_log at the edge steps: the pieces orc_sp_update is made of."""
    A, F = ref.MP(), ref.F64()
    for c in cases.all_cases():
        if c.P != 1:
            continue
        red = c.reduced()[0]
        eye = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
        if "lu" in c.tags:
            H, b = ref.finalize_Hb(F, [np.float64(v) for v in red], eye)
            x = orc.solve6(np.array(H), np.array(b))
            xm = np.array([float(v) for v in A.solve([A.c(v) for v in H], [A.c(v) for v in b])])
            e = ref.rel_err(x, xm)
            assert e is not None, c.name
            kappa = cases.cond(H) if np.isfinite(xm).all() else 1.0
            assert e.max() <= 64 * EPS * max(kappa, 1.0), (c.name, e.max(), kappa)
        if "exp" in c.tags and not c.name.startswith("log_clamp"):
            pr = c.step()["phi"][0, 3:]
            R, J = orc.so3_exp(pr)
            Rm, Jm = ref.so3_exp(A, [A.c(v) for v in pr])
            eR = ref.rel_err(R.reshape(-1), np.array([float(v) for v in Rm]))
            eJ = ref.rel_err(J.reshape(-1), np.array([float(v) for v in Jm]))
            assert eR is not None and eJ is not None, c.name
            assert eR.max() <= 8 * EPS, (c.name, eR.max())
            angle = float(np.linalg.norm(pr))            # (1 - cos) / angle: 1 - cos carries an absolute 2^-53, the quotient 2^-53 / angle
            assert eJ.max() <= 8 * EPS * max(1.0, 1.0 / angle if angle >= 1e-12 else 1.0), (c.name, eJ.max())
            w = orc.so3_log(R)
            wm = ref.so3_log(A, [A.c(v) for v in R.reshape(-1)])
            ew = ref.rel_err(w, np.array([float(v) for v in wm]))
            assert ew is not None, c.name


def test_early_stop_cases_sit_inside_their_float32_interval():
    """The mean step norm in mpmath: below t in double (a float64 compare would stop every case), and at least 2^-30
    (relative) away from t (1 - 2^-25), the point below which a float32 rounds away from t."""
    A = ref.MP()
    n = 0
    for c in cases.all_cases():
        if "es" not in c.tags:
            continue
        m = mk.reference_step(A, c)["aux"]["mean"]
        t, edge = A.c(c.thr), A.c(c.thr) * (1 - A.c(2.0) ** -25)
        assert np.float32(c.thr) == c.thr and m < t * (1 - A.c(2.0) ** -30), c.name
        if "_go_" in c.name:
            assert m >= edge * (1 + A.c(2.0) ** -30), c.name
        else:
            assert m <= edge * (1 - A.c(2.0) ** -30), c.name
        n += 1
    assert n == 6


def rejected(case, r, out):
    """Why the GPU test would refuse `out` for `case` (None: it would pass)."""
    if out["stop"] != r["stop"]:
        return "stop"
    if case.exact_h and not ref.same_median(out["h"], r["med"], case.P):
        return "median key"
    got = mk.subset(out, r["idx"])
    for q in ref.QUANTITIES:
        if r.get(q) is None:
            continue
        v, w = ref.compared(got, q), ref.compared(r, q)
        e = ref.rel_err(v, w)
        if e is None:
            return q + " pattern"
        if e.max() > FACTOR * max(r["eo"][q], EPS):
            return "%s %.2e" % (q, e.max())
    if "shard" in case.tags:
        right = case.step()
        if not (np.array_equal(out["H"], right["H"]) and np.array_equal(out["b"], right["b"])):
            return "H, b bits"
    return None


REJECTED_BY = {
    "median_upper": ("med_p4",),
    "median_ij": ("med_p3", "med_p5"),
    "lu_no_exchange": ("lu_k0_sw0_p1", "lu_k0_sw0_p3d", "lu_k0_sw0_p3f"),
    "lu_pivot_ge": ("lu_tie_p1", "lu_tie_p3d", "lu_tie_p3f"),
    "no_guards": ("exp_1e-13_p1", "exp_1e-13_p3"),
    "stop_f64": ("es_go_p1", "es_go_p5"),
    "ksum_no_diag": ("dir_default_p5", "med_p3"),
    "pose_old_R": ("exp_1e-3_p1", "dir_default_p5"),
    "rank_reverse": ("shard_w3_p1", "shard_w3_p3"),
    "adam_no_bias": ("seq3_adam_p1", "seq3_adam_p5"),
}


def test_every_variant_is_listed():
    assert set(REJECTED_BY) | {"log_no_clamp"} == set(ref.VARIANTS)


@pytest.mark.parametrize("variant", sorted(REJECTED_BY))
def test_wrong_variant_is_rejected(fixture, variant):
    by_name = {c.name: c for c in cases.all_cases()}
    reasons = {}
    for name in REJECTED_BY[variant]:
        c = by_name[name]
        r = mk.case_reference(fixture, c)
        assert rejected(c, r, c.step()) is None, "the right float64 step is refused on " + name
        reasons[name] = rejected(c, r, c.step((variant,)))
    print(variant, reasons)
    assert any(reasons.values()), "no named case rejects the variant " + variant


def test_log_clamp_is_redundant(fixture):
    """The two cases reach the clamp (asserted when they are built: 0.5 (trace - 1) > 1 and < -1 in float64), and Log gives the
    same zeros with and without it — see the module docstring."""
    by_name = {c.name: c for c in cases.all_cases()}
    for name in ("log_clamp_above", "log_clamp_below"):
        c = by_name[name]
        assert abs(c.info["craw"]) > 1
        a, b = c.step(), c.step(("log_no_clamp",))
        assert (a["pose"][3:] == 0).all() and np.array_equal(a["pose"], b["pose"])
        assert rejected(c, mk.case_reference(fixture, c), a) is None
