"""The plane residual's kernels one by one on the GPU (k_target_normals, k_pack_normals, k_plane_accumulate<PW, WP, TRACE>,
k_plane_finalize), against exact rationals and the mpmath values of tests/golden/plane.npz.  Needs numpy, torch and the fixture.

Normals: every case of plane_cases.normal_cases runs svnicp_align_begin with residual = plane and no supplied normals; the
result is read with svnicp_get_target_normals.  Every row of every cluster is judged, none left out: validity exactly as the
fixture has it; an exact kind's normal a signed unit axis vector bit for bit; | |n| - 1 | <= 4 * 2^-53; eigen-residual and
Rayleigh excess against the cluster's exact scatter matrix (plane_mp_reference.criterion) within 16 max(E_ref, kn 2^-52),
E_ref being numpy's eigh on the float64 restatement's matrix.  Where (l1 - l0) / l2 >= 1e-3 the angle follows from the
residual (sin theta <= residual / gap); no second number is needed.

Record: every case of plane_cases.all_cases runs on a fresh context — svnicp_set_residual(plane, delta, 16),
svnicp_set_target_normals, svnicp_align_begin, the stage-B grid read back through svnicp_get_stage_b_grid and compared with
the one the case was built for, the candidate table and the total poses written through their taps,
svnicp_build_candidate_table, ONE svnicp_iter_accumulate(0), the record and the statistics read through
svnicp_plane_record_devptr / svnicp_plane_stats_devptr — with record_trace off and on (the TRACE false and true
instantiations), and once more.  Compared exactly: the three runs bit for bit; the trace's winners against the reference's;
the accepted count; H's symmetry; that every entry of the P rows was written and no row of a padded particle; an exact case's whole record against the float64 restatement (which the CPU test shows to
be the correctly rounded exact value there).  Compared to stage B's bar: on the particles with mpmath values
E = |v - v_mp| / max(sum|term|_mp, 1e-300) <= 16 max(E_f64, 2^-52) per sum group; on the others |v - v_f64| / sum|term|
within twice that bar at the case's largest yardstick.  The only skip: a grid the device has too few CUs for.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import plane_cases as cases
import plane_mp_reference as pm
import plane_reference as pr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_plane", os.path.join(HERE, "golden", "make_plane.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)

FACTOR, FLOOR = 16.0, 2.0 ** -52
NORM_BAR = 4 * 2.0 ** -53
SENTINEL = -7.25e77      # fills the record before the one svnicp_iter_accumulate: no value of any case
NORMAL_RATIOS = {}   # cluster kind -> largest figure / bar
RECORD_RATIOS = {}   # (variant, sum group) -> largest E_gpu / max(E_f64, 2^-52)


@pytest.fixture(scope="module")
def fixture():
    return mk.load()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for kind, r in sorted(NORMAL_RATIOS.items()):
        print("normals, largest figure / bar: %-18s %.3g" % (kind, r))
    for (variant, g), r in sorted(RECORD_RATIOS.items()):
        print("record, largest E_gpu / max(E_f64, 2^-52): variant %-6s %-3s %.3g" % (variant, g, r))


def guarded(hip, what, fn):
    """fn(); an error of the HIP runtime ends the session: nothing more is started on a device that has faulted."""
    try:
        return fn()
    except hip.SvnIcpError as e:
        pytest.exit("HIP error in %s: %s" % (what, e), returncode=3)


# ------------------------------------------------------------------------------------------------ normals
def device_normals(hip, case):
    prm = hip.SteinICPParam(iterations=1, lr=1.0, max_dist=1.0, KNN_count=4)
    init = np.zeros((6, 1))
    s = hip.SVNICP(prm, init)
    s.set_residual("plane", 0.1, case.kn)
    s.add_cloud(case.src, case.tgt, init)
    s._check(s._L.svnicp_align_begin(s.handle), "svnicp_align_begin")
    n = s.get_target_normals()
    assert s.get_plane_stats(with_sums=False)[1] == 1
    s.close()
    return n


@pytest.mark.parametrize("case", cases.normal_cases(), ids=lambda c: c.name)
def test_normals_alone(hip, fixture, case):
    r = mk.normal_reference(fixture, case)
    assert r["chk"] == int(case.checksum()), "tests/golden/plane.npz is stale: run tests/golden/make_plane.py"
    n = guarded(hip, case.name, lambda: device_normals(hip, case))
    assert n.shape == (case.M, 3) and np.isfinite(n).all()
    wrong, fig, axes = pm.judge_clusters(case, r["lam"], r["valid"], n)
    assert not wrong, "%d rows have a normal where there is none, or none where there is one; first (kind, placement, row): %s" % (len(wrong), wrong[:4])
    assert not axes, "an exactly diagonal scatter matrix must give a signed unit axis vector bit for bit: %s" % (axes[:4],)
    bar = FACTOR * max(max(r["eref"]), case.kn * FLOOR)
    worst = {}
    for kind, (nm, res, ray) in sorted(fig.items()):
        worst[kind] = max(nm / NORM_BAR, res / bar, abs(ray) / bar)
        NORMAL_RATIOS[kind] = max(NORMAL_RATIOS.get(kind, 0.0), worst[kind])
        print("%s %-18s | |n| - 1 | %.2e (bar %.2e), residual %.2e, rayleigh %.2e (bar %.2e, E_ref %.2e)" % (case.name, kind, nm, NORM_BAR, res, ray, bar, max(r["eref"])))
    assert set(fig) == {c.kind for c, v in zip(case.clusters, r["valid"]) if v}, "every valid kind was judged"
    for kind, w in worst.items():
        assert w <= 1.0, "%s %s: %.3g of the bar" % (case.name, kind, w)


def test_supplied_normals_table(hip):
    """k_pack_normals on one crafted table: unit rows within 2 ulp, 'no normal' rows exactly 0 — a zero, NaN or inf row, a row at
    a non-finite point, and the finite rows whose squared norm overflows (1e160) or underflows (1e-170, subnormal) in float64."""
    tgt, nrm, want, notes = cases.pack_table()
    init = np.zeros((6, 1))

    def run():
        s = hip.SVNICP(hip.SteinICPParam(iterations=1, lr=1.0, max_dist=1.0, KNN_count=4), init)
        s.set_residual("plane", 0.1, 8)
        s.add_cloud(np.zeros((4, 3)), tgt, init)
        s.set_target_normals(nrm)
        got = s.get_target_normals()
        s.close()
        return got
    got = guarded(hip, "supplied normals", run)
    kept = pr.normalise_supplied(nrm, tgt)
    assert np.array_equal(got, kept), "n / |n| with |n| = sqrt((x x + y y) + z z) in float64, bit for bit: what the kernel does today"
    for g, w, note in zip(got, want, notes):
        if w.any():
            assert np.abs(g - w).max() <= 2 * 2.0 ** -53, (note, g, w)
        else:
            assert np.array_equal(g, np.zeros(3)), (note, g)


# ------------------------------------------------------------------------------------------------ accumulate and finalize
def run_case(hip, case, options, trace):
    """One svnicp_iter_accumulate of `case` on a fresh context: dict(Hb [P][42], stats [P][2], corr [P][B] or None, grid)."""
    import torch
    from svnicp_amd.sharded import _DevView
    L = hip.load_library()
    P, B, K = case.P, case.B, case.K
    init = np.zeros((6, P))
    prm = hip.SteinICPParam(iterations=1, lr=1.0, max_dist=case.max_dist, KNN_count=K, record_trace=trace)
    s = hip.SVNICP(prm, init)
    s.set_residual("plane", case.delta, 16)
    s.add_cloud(case.src, case.tgt, init)
    s.set_target_normals(case.nrm_supplied)
    for k, v in options:
        s.set_option(k, v)
    s._check(L.svnicp_align_begin(s.handle), "svnicp_align_begin")
    grid = (C.c_int * 4)()
    s._check(L.svnicp_get_stage_b_grid(s.handle, grid), "svnicp_get_stage_b_grid")
    grid = tuple(int(x) for x in grid)
    if grid != case.expected_grid():       # the case was built for another grid: nothing is launched
        s.close()
        return dict(grid=grid)
    s.synchronize()

    def view(fn, shape, dt):
        ptr = getattr(L, fn)(s.handle)
        assert ptr, fn
        return torch.as_tensor(_DevView(ptr, shape, dt), device="cuda")
    view("svnicp_candidates_devptr", (B, K), "<i4").copy_(torch.from_numpy(case.cand))
    view("svnicp_total_pose_devptr", (P, 12), "<f8").copy_(torch.from_numpy(case.poses))
    rows = max(P, grid[3])                 # the record is allocated for the padded particles too; no kernel may write their rows
    view("svnicp_plane_record_devptr", (rows, 42), "<f8").fill_(SENTINEL)
    view("svnicp_plane_stats_devptr", (rows, 2), "<f8").fill_(SENTINEL)
    torch.cuda.synchronize()
    s._check(L.svnicp_build_candidate_table(s.handle), "svnicp_build_candidate_table")
    s._check(L.svnicp_iter_accumulate(s.handle, 0), "svnicp_iter_accumulate")
    s.synchronize()
    Hb = view("svnicp_plane_record_devptr", (rows, 42), "<f8").cpu().numpy().copy()
    stats = view("svnicp_plane_stats_devptr", (rows, 2), "<f8").cpu().numpy().copy()
    pad = np.concatenate([Hb[P:], stats[P:]], 1)
    Hb, stats = Hb[:P], stats[:P]
    kept = s.get_target_normals()
    s._check(L.svnicp_finish(s.handle), "svnicp_finish")
    s.synchronize()
    corr = s.get_trace()["corr"][0].astype(np.int64) if trace else None
    s.close()
    return dict(grid=grid, Hb=Hb, stats=stats, corr=corr, kept=kept, pad=pad)


def check_exact(case, variant, out):
    D = case.discrete()
    Hb, stats = out["Hb"], out["stats"]
    assert np.isfinite(Hb).all() and np.isfinite(stats).all(), "%s: a value is not finite" % variant
    assert not (Hb == SENTINEL).any() and not (stats == SENTINEL).any(), "%s: an entry of a particle's record or statistics was not written" % variant
    assert out["pad"].shape[0] == case.geometry()[4] - case.P and (out["pad"] == SENTINEL).all(), "%s: a row beyond P was written" % variant
    assert np.array_equal(out["kept"] != 0.0, case.nrm != 0.0) and np.abs(out["kept"] - case.nrm).max() <= 2 * 2.0 ** -53, \
        "%s: the kept normals are not the restatement's n / |n| within 2 ulp" % variant
    if "exact" in case.tags:
        assert np.array_equal(out["kept"], case.nrm)
    if out["corr"] is not None:
        bad = np.argwhere(out["corr"] != D["win"])
        assert bad.size == 0, "%s: %d of %d winners differ from the reference, first (particle, row) %s" % (variant, len(bad), case.P * case.B, bad[:1].tolist())
    H = Hb[:, :36].reshape(-1, 6, 6)
    assert np.array_equal(H, H.transpose(0, 2, 1)), "%s: H is not symmetric bit for bit" % variant
    assert np.array_equal(stats[:, 0], D["ok"].sum(1).astype(np.float64)), "%s: the accepted count" % variant
    if "all_rejected" in case.tags:
        assert np.array_equal(H, np.broadcast_to(pr.DAMPING * np.eye(6), H.shape)) and not Hb[:, 36:].any() and not stats.any(), \
            "%s: an all-rejected case gives H = 1e-6 I, b = 0, statistics 0" % variant
    if "exact" in case.tags:
        v64, _ = case.f64()
        got = pm.vec29(Hb, stats)
        bad = np.argwhere(got != v64)
        assert bad.size == 0, "%s: %d values differ from the exact record, first (particle, value) %s: %r for %r" % (
            variant, len(bad), bad[0].tolist(), got[tuple(bad[0])], v64[tuple(bad[0])])


def check_bar(case, variant, out, r):
    v = pm.vec29(out["Hb"], out["stats"])
    idx = r["idx"]
    e = pm.error_against_mp(v[idx], r["v64"][idx], r["mag"][idx], r["eps"])
    worst = {}
    for g, ix in pm.GROUPS:
        ratio = float(e[:, list(ix)].max()) / max(r["yard"][g], FLOOR)
        worst[g] = ratio
        RECORD_RATIOS[(variant, g)] = max(RECORD_RATIOS.get((variant, g), 0.0), ratio)
        print("%s %s %s: E_gpu %.3e, E_f64 %.3e, ratio %.3g" % (case.name, variant, g, e[:, list(ix)].max(), r["yard"][g], ratio))
    for g, _ in pm.GROUPS:
        assert worst[g] <= FACTOR, "%s %s: E_gpu is %.3g x max(E_f64, 2^-52), the bar is %g" % (variant, g, worst[g], FACTOR)
    rest = np.setdiff1d(np.arange(case.P), idx)
    if rest.size:
        bar = 2 * FACTOR * max(max(r["yard"].values()), FLOOR)
        with np.errstate(all="ignore"):
            e2 = np.abs(v[rest] - r["v64"][rest]) / r["mag"][rest]
        assert e2.max() <= bar, "%s: a particle without mpmath values is %.3e from the float64 restatement (bar %.3e)" % (variant, e2.max(), bar)


@pytest.mark.parametrize("case", cases.all_cases(), ids=lambda c: c.name)
def test_record_alone(hip, fixture, case):
    import torch
    r = mk.case_reference(fixture, case)
    assert r["chk"] == int(case.checksum()) and r["crc_ok"], "tests/golden/plane.npz is stale: run tests/golden/make_plane.py"
    V = cases.variants(case)
    outs = {}
    for name in ("plain", "traced", "again"):
        options, trace = V["plain" if name == "again" else name]
        outs[name] = guarded(hip, "case %s, variant %s" % (case.name, name), lambda: run_case(hip, case, options, trace))
        if outs[name]["grid"] != case.expected_grid():
            want, got = case.expected_grid(), outs[name]["grid"]
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            if got[0] < want[0] and want[0] * want[1] > cus:
                pytest.skip("%s needs a grid of %d x %d workgroups in one resident round; this device has %d CUs and plans %s" % (case.name, want[0], want[1], cus, got))
            assert got == want, "%s was built for the stage-B grid %s {grid_x, grid_y, pts_per_block, Ppad}, the registration plans %s" % (case.name, want, got)
    for name, out in outs.items():
        check_exact(case, name, out)
    for k in ("Hb", "stats"):
        assert np.array_equal(outs["plain"][k], outs["again"][k]), "the same case run twice differs in %s" % k
        assert np.array_equal(outs["plain"][k], outs["traced"][k]), "TRACE false and true differ in %s" % k
    for name in ("plain", "traced"):
        check_bar(case, name, outs[name], r)
