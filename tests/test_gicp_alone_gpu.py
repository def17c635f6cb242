"""k_gicp_accumulate<PW, WP, TRACE> (+ k_plane_finalize behind it) alone on the GPU, with the mechanics of
tests/test_plane_alone_gpu.py: every case of tests/gicp_cases.py runs on a fresh context — svnicp_set_residual_gicp, the
supplied normals of both clouds, svnicp_align_begin, the candidate table and the total poses written through their taps,
svnicp_build_candidate_table, ONE svnicp_iter_accumulate(0), the record [P][42] and the statistics [P][2] read through
svnicp_plane_record_devptr / svnicp_plane_stats_devptr — with record_trace off and on (the TRACE false and true
instantiations), and once more.

Compared exactly, every case: the three runs bit for bit; the trace's winners; the accepted count; H's symmetry; every entry of
the P rows written and no row of a padded particle; an `exact` case's whole record against the float64 restatement (dyadic
inputs and epsilon = 1: every product and sum is exact, whatever the order).
Compared to plane mode's bar, every other case (the geometry cases; kilometre coordinates, a cancelling b, epsilon = 1e-6 with
near-antiparallel and near-orthogonal normals): on the particles with mpmath values in tests/golden/gicp/gicp.npz
(stage_b_reference.mp_particles) E = |v - v_mp| / mag <= 16 max(E_f64, 2^-52) per sum group; on the others |v - v_f64| / mag
within twice that bar at the case's largest yardstick.  mag = sum of cond(S_pair) |term|, taken term-wise; the factor cond(S) is
derived in tests/gicp_mp_reference.py's docstring.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import gicp_cases as cases
import gicp_mp_reference as gm
import gicp_reference as gr
import plane_mp_reference as pm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_gicp", os.path.join(HERE, "golden", "make_gicp.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)

FACTOR, FLOOR = 16.0, 2.0 ** -52
SENTINEL = -7.25e77      # fills the record before the one svnicp_iter_accumulate: no value of any case
RATIOS = {}              # (case, sum group) -> E_gpu / max(E_f64, 2^-52)


@pytest.fixture(scope="module")
def fixture():
    return mk.load()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for (name, g), (r, e, y) in sorted(RATIOS.items()):
        print("record, %-28s %-3s E_gpu %.3e E_f64 %.3e ratio %.3g" % (name, g, e, y, r))


def guarded(hip, what, fn):
    """fn(); an error of the HIP runtime ends the session: nothing more is started on a device that has faulted."""
    try:
        return fn()
    except hip.SvnIcpError as e:
        pytest.exit("HIP error in %s: %s" % (what, e), returncode=3)


def run_case(hip, case, trace):
    """One svnicp_iter_accumulate of `case` on a fresh context: dict(Hb [P][42], stats [P][2], corr [P][B] or None, pad)."""
    import torch
    from svnicp_amd.sharded import _DevView
    L = hip.load_library()
    P, B, K = case.P, case.B, case.K
    init = np.zeros((6, P))
    prm = hip.SteinICPParam(iterations=1, lr=1.0, max_dist=case.max_dist, KNN_count=K, record_trace=trace)
    s = hip.SVNICP(prm, init)
    s.set_residual("gicp", case.delta, 16, case.eps)
    s.add_cloud(case.src, case.tgt, init)
    s.set_target_normals(case.nt_supplied)
    s.set_source_normals(case.ns_supplied)
    for k, v in case.options():
        s.set_option(k, v)
    s._check(L.svnicp_align_begin(s.handle), "svnicp_align_begin")
    grid = (C.c_int * 4)()
    s._check(L.svnicp_get_stage_b_grid(s.handle, grid), "svnicp_get_stage_b_grid")
    assert int(grid[3]) == case.padded_particles(), "the plan pads the particles as registration_plan.hpp's shape says"
    s.synchronize()

    def view(fn, shape, dt):
        ptr = getattr(L, fn)(s.handle)
        assert ptr, fn
        return torch.as_tensor(_DevView(ptr, shape, dt), device="cuda")
    view("svnicp_candidates_devptr", (B, K), "<i4").copy_(torch.from_numpy(case.cand))
    view("svnicp_total_pose_devptr", (P, 12), "<f8").copy_(torch.from_numpy(case.poses))
    rows = max(P, int(grid[3]))            # the record is allocated for the padded particles too; no kernel may write their rows
    view("svnicp_plane_record_devptr", (rows, 42), "<f8").fill_(SENTINEL)
    view("svnicp_plane_stats_devptr", (rows, 2), "<f8").fill_(SENTINEL)
    torch.cuda.synchronize()
    s._check(L.svnicp_build_candidate_table(s.handle), "svnicp_build_candidate_table")
    s._check(L.svnicp_iter_accumulate(s.handle, 0), "svnicp_iter_accumulate")
    s.synchronize()
    Hb = view("svnicp_plane_record_devptr", (rows, 42), "<f8").cpu().numpy().copy()
    stats = view("svnicp_plane_stats_devptr", (rows, 2), "<f8").cpu().numpy().copy()
    pad = np.concatenate([Hb[P:], stats[P:]], 1)
    kept_t, kept_s = s.get_target_normals(), s.get_source_normals()
    s._check(L.svnicp_finish(s.handle), "svnicp_finish")
    s.synchronize()
    corr = s.get_trace()["corr"][0].astype(np.int64) if trace else None
    s.close()
    return dict(Hb=Hb[:P], stats=stats[:P], corr=corr, pad=pad, kept_t=kept_t, kept_s=kept_s, grid=tuple(int(x) for x in grid))


def check_exact(case, variant, out):
    D = case.discrete()
    Hb, stats = out["Hb"], out["stats"]
    assert np.isfinite(Hb).all() and np.isfinite(stats).all(), "%s: a value is not finite" % variant
    assert not (Hb == SENTINEL).any() and not (stats == SENTINEL).any(), "%s: an entry of a particle's record or statistics was not written" % variant
    assert out["pad"].shape[0] == case.padded_particles() - case.P and (out["pad"] == SENTINEL).all(), "%s: a row beyond P was written" % variant
    for kept, want in ((out["kept_t"], case.nt), (out["kept_s"], case.ns)):
        assert np.array_equal(kept != 0.0, want != 0.0) and np.abs(kept - want).max() <= 2 * 2.0 ** -53, "%s: the kept normals" % variant
    if out["corr"] is not None:
        assert np.array_equal(out["corr"], D["win"]), "%s: winners differ from the reference" % variant
    H = Hb[:, :36].reshape(-1, 6, 6)
    assert np.array_equal(H, H.transpose(0, 2, 1)), "%s: H is not symmetric bit for bit" % variant
    assert np.array_equal(stats[:, 0], D["ok"].sum(1).astype(np.float64)), "%s: the accepted count" % variant
    if "all_rejected" in case.tags:
        assert not D["ok"].any()
        assert np.array_equal(H, np.broadcast_to(gr.DAMPING * np.eye(6), H.shape)) and not Hb[:, 36:].any() and not stats.any(), \
            "%s: an all-rejected case gives H = 1e-6 I, b = 0, statistics 0" % variant
    if "gate_rejects_row0" in case.tags:
        assert not D["ok"][0, 0] and D["ok"][0, 1] and D["d2"][0, 0] == case.max_dist
    if "gate_accepts_row0" in case.tags:
        assert D["ok"][0, 0] and D["d2"][0, 0] == np.nextafter(case.max_dist, 0.0)
    if "huber_w1" in case.tags:
        assert stats[0, 1] == 0.25 and Hb[0, 0] == 1.0 + gr.DAMPING and Hb[0, 36] == 0.5, "rho = delta: weight 1"
    if "huber_below1" in case.tags:
        w = case.delta / 0.5
        assert w < 1.0 and stats[0, 1] == w * 0.25 and Hb[0, 0] == w + gr.DAMPING and Hb[0, 36] == w * 0.5 and Hb[0, 3 * 6 + 3] == 4.0 * w + gr.DAMPING
    if "exact" in case.tags:
        v64, _ = gm.sums_f64(case)
        got = pm.vec29(Hb, stats)
        bad = np.argwhere(got != v64)
        assert bad.size == 0, "%s: %d values differ from the exact record, first (particle, value) %s: %r for %r" % (
            variant, len(bad), bad[0].tolist(), got[tuple(bad[0])], v64[tuple(bad[0])])


def check_bar(case, variant, out, r):
    """On the particles with mpmath values E = |v - v_mp| / mag <= 16 max(E_f64, 2^-52) per sum group; on the others
    |v - v_f64| / mag within twice that bar at the case's largest yardstick (tests/test_plane_alone_gpu.py's check_bar)."""
    v = pm.vec29(out["Hb"], out["stats"])
    idx = r["idx"]
    assert np.array_equal(v[:, 27], r["v64"][:, 27]), "the accepted count"
    e = pm.error_against_mp(v[idx], r["v64"][idx], r["mag"][idx], r["eps"])
    for g, ix in gm.GROUPS:
        eg, ey = float(e[:, list(ix)].max()), r["yard"][g]
        ratio = eg / max(ey, FLOOR)
        RATIOS[(case.name + "/" + variant, g)] = (ratio, eg, ey)
        assert ratio <= FACTOR, "%s %s %s: E_gpu %.3e is %.3g x max(E_f64 %.3e, 2^-52), the bar is %g" % (case.name, variant, g, eg, ratio, ey, FACTOR)
    rest = np.setdiff1d(np.arange(case.P), idx)
    if rest.size:
        bar = 2 * FACTOR * max(max(r["yard"].values()), FLOOR)
        with np.errstate(all="ignore"):
            e2 = np.abs(v[rest] - r["v64"][rest]) / r["mag"][rest]
        assert e2.max() <= bar, "%s: a particle without mpmath values is %.3e from the float64 restatement (bar %.3e)" % (variant, e2.max(), bar)


@pytest.mark.parametrize("case", cases.all_cases(), ids=lambda c: c.name)
def test_record_alone(hip, fixture, case):
    r = None
    if "exact" not in case.tags:
        r = mk.case_reference(fixture, case)
        assert r["chk"] == int(case.checksum()) and r["crc_ok"], "tests/golden/gicp/gicp.npz is stale: run tests/golden/make_gicp.py"
    outs = {}
    for name, trace in (("plain", False), ("traced", True), ("again", False)):
        outs[name] = guarded(hip, "case %s, variant %s" % (case.name, name), lambda: run_case(hip, case, trace))
    for name, out in outs.items():
        check_exact(case, name, out)
    for k in ("Hb", "stats"):
        assert np.array_equal(outs["plain"][k], outs["again"][k]), "the same case run twice differs in %s" % k
        assert np.array_equal(outs["plain"][k], outs["traced"][k]), "TRACE false and true differ in %s" % k
    if r is not None:
        for name in ("plain", "traced"):
            check_bar(case, name, outs[name], r)
