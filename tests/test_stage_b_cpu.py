"""Stage B alone, host side: the fixture tests/golden/stage_b.npz against the case module, every case's regime, and ten
deliberately wrong float64 programs refused under the bar the GPU test uses.  Needs numpy and the fixture only.

The bar (tests/test_stage_b_gpu.py): on the particles that have mpmath sums, E = |v - v_mp| / max(sum|term|_mp, 1e-300) per
particle and sum must not exceed 16 max(E_f64, 2^-52), E_f64 being the float64 restatement's largest E of the case and sum
group; winners, masks and SVGD-ICP counts are compared exactly.  A wrong variant is refused when it changes a winner, a mask or
a count of its named case, or when its sums miss that bar there.

Pinned as an equivalence instead of a case that tells two programs apart (test_root_below_2m1000_cannot_matter): below
d2 = 2^-1000 the accumulate kernel's root (an rsq seed of d2 + 2^-1000) is wrong relatively, by up to 2^500 sqrt(d2), and
harmless absolutely — it enters the weight only, as 1 / (1 + (3 / max_dist) root)^2, which is 1.0 in float64 for every root
up to 2^-500 and every max_dist from 1e-130 up (3 2^-500 / max_dist is then below 2^-54); the residual sums take dx, dy, dz themselves.
"""
import importlib.util
import os

import numpy as np
import pytest

import stage_b_cases as cases
import stage_b_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_stage_b", os.path.join(HERE, "golden", "make_stage_b.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)

FACTOR, FLOOR = 16.0, 2.0 ** -52


@pytest.fixture(scope="module")
def fixture():
    return mk.load()


def test_fixture_is_left_out_of_the_whole_registration_vectors():
    import helpers
    assert os.path.exists(mk.FIXTURE) and "stage_b" not in helpers.golden_cases() and "stein_step" not in helpers.golden_cases()
    assert os.path.getsize(mk.FIXTURE) <= os.path.getsize(os.path.join(HERE, "golden", "svn_p64_k100.npz"))


def test_fixture_matches_the_case_module(fixture):
    """Checksums of the inputs and of the recomputed float64 sums; the float64 restatement against mpmath: its E stays
    within the a-priori bound of a left-to-right sum of B terms of at most six roundings each, (B + 6) 2^-53."""
    cs = cases.all_cases()
    assert [c.name for c in cs] == [str(n) for n in fixture["names"]], "stale fixture: run tests/golden/make_stage_b.py"
    for c in cs:
        r = mk.case_reference(fixture, c)
        assert r["chk"] == int(c.checksum()), "%s: stale fixture: run tests/golden/make_stage_b.py" % c.name
        assert r["crc_ok"], "%s: the float64 restatement gives other sums here than where the fixture was made" % c.name
        assert np.array_equal(r["idx"], c.mp_particles())
        e = np.abs(r["eps"].astype(np.float64))
        assert np.isfinite(r["v64"]).all() and e.max() <= (c.B + 6) * 2.0 ** -53, (c.name, e.max())
        for j, (g, ix) in enumerate(ref.GROUPS):
            assert r["yard"][g] == e[:, list(ix)].max()


def test_mp_particle_rule():
    assert ref.mp_particles(9).tolist() == [0, 8]
    assert ref.mp_particles(16).tolist() == [0, 15]
    assert ref.mp_particles(17).tolist() == [0, 15, 16]
    assert ref.mp_particles(130).tolist() == [0, 15, 16, 31, 32, 47, 48, 63, 64, 79, 80, 95, 96, 111, 112, 127, 128, 129]
    assert ref.mp_particles(24, (3, 20)).tolist() == [3, 15, 16, 19]
    assert ref.mp_particles(130, (64, 130)).tolist() == [64, 79, 80, 95, 96, 111, 112, 127, 128, 129]


def test_every_case_reaches_its_regime():
    """Building a case asserts its regime (stage_b_cases); here: the set is the one the tests are written for."""
    cs = {c.name: c for c in cases.all_cases()}
    for c in cs.values():
        assert 0 <= c.cand.min() and c.cand.max() < c.M <= 512 and c.B <= 300 and c.K <= 128
        lo, hi = c.particles()
        assert hi - lo > 8 and set(cases.variants(c)) == {"plain", "traced", "f64", "valu"}
    assert {c.K for c in cs.values() if "placement" in c.tags} == set(cases.PLACEMENT_K)
    for K in (97, 100, 101, 128):     # the tail tile's four slots win somewhere
        assert {96, 97, 98, 99} <= set(cs["place_K%d_P12" % K].discrete()["win"].reshape(-1).tolist()) | set(range(K, 100))
    assert {c.P for c in cs.values() if "geometry" in c.tags} >= set(cases.GEOMETRY_P)
    for P in cases.GEOMETRY_P:
        pp = cases.points_per_pass(P)
        want = {1, pp - 1, pp + 1, 4 * pp - 1, 4 * pp + 1} - {0}
        assert {c.B for c in cs.values() if c.name.startswith("geom_P%d_" % P)} == want
    assert [cases.points_per_pass(P) for P in cases.GEOMETRY_P] == [16, 16, 8, 8, 4, 4, 2, 2, 1, 1, 1]
    assert cs["shard_3_20_of_24"].shard == (3, 20) and cs["shard_64_130_of_130"].shard == (64, 130)
    assert cs["row_shard_1_of_2"].row_shard == (1, 2, 82)
    assert cs["cert_gaps_P64"].facts["wrong_below"] >= 0.1 and cs["cert_gaps_P64"].facts["above2"] > 0
    assert cs["cert_underflow_1e-25"].facts["f64_ties"] == 0.5      # the rows a metre away tie in float64, the rows at 3e-24 m do not
    q = cs["cert_underflow_1e-25"].tgt
    assert (np.abs(q).max() < 1.1e-25) and ((q.astype(np.float32).astype(np.float64) ** 2).sum(1).astype(np.float32) == 0).all(), "|c|^2 underflows"
    c = cs["cert_close_1e-9_at_10"]
    spread = np.ptp(c.tgt.reshape(c.B, c.K, 3), axis=1).max()
    assert spread < 2.1e-9 and spread < 2.0 ** -24 * 10 * 4, "closer together than 2^-24 of their distance to the point"
    assert cs["cancel_km"].facts["cancel"] <= 1e-12 and np.abs(cs["cancel_km"].src).max() > 4000
    assert not cs["mask_all_rejected"].discrete()["mask"].any() and cs["mask_all_accepted"].discrete()["mask"].all()


@pytest.mark.parametrize("num_cus", [256, 304, 64])
def test_overflow_cases_overflow(num_cus):
    full, holes = cases.overflow_cases(num_cus)
    for c in (full, holes):
        assert c.P == 64 and c.K == 16 and ("wgpcu", "1,1") in c.options and not c.mp
        assert c.B * 64 // num_cus >= 2 * cases.QUEUE_CAP
    assert full.B == 8192 or num_cus != 256
    assert full.facts["expected_ambiguous"] == full.B * 64 and holes.facts["expected_ambiguous"] == holes.B * 48


# variant -> the case that refuses it, and how ("discrete": a winner, mask or count changes; "sums": the bar)
REFUSED_BY = {
    "argmin_le": ("ties_K100_P16", "discrete"), "mask_le": ("mask_edge_at", "discrete"), "mask_squared": ("resid_band_md0.001", "discrete"),
    "reject_dropped": ("mask_all_rejected", "sums"), "weight_unsquared": ("mask_all_accepted", "sums"),
    "weight_on_rejected": ("mask_all_rejected", "sums"), "count_on_mask": ("svgd_zero_row", "discrete"),
    "transform_fused": ("place_km", "sums"), "anchor_nearest": ("place_K17_P12", "discrete"), "sum_f32": ("geom_P9_B17", "sums"),
}


def judged(case, r, variant):
    """(discrete outputs equal the reference's, largest E / bar over the sum groups) of a float64 program on the mpmath subset."""
    D0, D = case.discrete(), case.discrete(variant)
    same = all(np.array_equal(D0[k], D[k]) for k in ("win", "mask", "cnt"))
    v, _ = ref.sums_f64(case.src, D, case.max_dist, case.svgd, variant)
    idx = r["idx"]
    e = ref.error_against_mp(v[idx], r["v64"][idx], r["mag"][idx], r["eps"])
    worst = max(e[:, list(ix)].max() / (FACTOR * max(r["yard"][g], FLOOR)) for g, ix in ref.GROUPS)
    return same, worst


def test_variant_list_is_the_references():
    assert set(REFUSED_BY) == set(ref.VARIANTS) and len(ref.VARIANTS) == 10


@pytest.mark.parametrize("variant", ref.VARIANTS)
def test_wrong_variant_is_refused(fixture, variant):
    name, how = REFUSED_BY[variant]
    case = cases.by_name(name)
    r = mk.case_reference(fixture, case)
    same, worst = judged(case, r, ())
    assert same and worst <= 1.0 / FACTOR + 1e-9, "the float64 restatement itself passes, at its own E"
    same, worst = judged(case, r, (variant,))
    print("%s on %s: discrete part %s, worst E / bar %.3g" % (variant, name, "equal" if same else "differs", worst))
    if how == "discrete":
        assert not same
    else:
        assert worst > 1.0, "%s passes the bar on %s (%.3g of it)" % (variant, name, worst)


def test_root_below_2m1000_cannot_matter():
    """See the module docstring.  Every root a refinement could return for d2 < 2^-1000 lies in [0, 2^-500]."""
    roots = np.array([0.0, 2.0 ** -1074, 1e-160, 1e-155, 2.0 ** -500])
    for md in (1e-130, 1e-3, 1.0, 1e3, 1e300):
        w = md / (md + 3.0 * roots)
        assert (w * w == 1.0).all()
        c3 = 3.0 / md
        y = 1.0 / (1.0 + c3 * roots)
        assert (y * y == 1.0).all()
    c = cases.by_name("resid_tiny_md0.001")
    D = c.discrete()
    small = D["d2"] < 2.0 ** -1000
    assert small.any() and D["mask"][small].all()
    n = np.sqrt(D["d2"][small])                                  # the reference's own root of those rows
    assert n.max() <= 2.0 ** -500 and ((c.max_dist / (c.max_dist + 3.0 * n)) ** 2 == 1.0).all()
