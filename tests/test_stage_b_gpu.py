"""Stage B alone on the GPU (k_stein_search_bf16, k_stein_accumulate_w, k_reduce_partials and the two one-kernel variants),
against the discrete reference and the mpmath sums of tests/golden/stage_b.npz.

Every case of tests/stage_b_cases.py runs on a fresh context through every variant that admits it (stage_b_cases.variants):
svnicp_align_begin, the case's candidate table written into svnicp_candidates_devptr and its total poses into
svnicp_total_pose_devptr, svnicp_build_candidate_table, ONE svnicp_iter_accumulate(0), the sums read from svnicp_sums_devptr
(svnicp_rank_sums_devptr for the row shard).  Stage A never runs.  Needs numpy, torch and the fixture only.

Compared exactly: the trace's winner slot of every pair against the reference's (variants traced, f64, valu); that every sum
is finite; sum w = B and 21 zeros of an all-rejected case; SVGD-ICP's count; the row shard's slot and the zeros of the other
slot; the same case run twice, bit for bit; and plain (k_stein_accumulate_w<.., true>, reading kidx) against traced (<.., false>,
reading the slot byte), bit for bit: both gather tgt[cand[b][slot]] and run the same accumulate body in the same row order.
Compared to the bar: on the particles with mpmath sums, E = |v - v_mp| / max(sum|term|_mp, 1e-300) <= 16 max(E_f64, 2^-52)
per sum group; on the other particles |v - v_f64| / sum|term| within twice that bar at the case's largest yardstick.  The
queue-overflow cases have no mpmath sums: there the bar is the a-priori distance of two float64 sums of the same B terms,
(2 B + 20) 2^-53 (each is within (B + 6) 2^-53 of the exact sum of its terms, and the device's weight is good to a few 2^-53).
"""
import importlib.util
import os

import numpy as np
import pytest

import stage_b_cases as cases
import stage_b_reference as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_stage_b", os.path.join(HERE, "golden", "make_stage_b.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)

FACTOR, FLOOR = 16.0, 2.0 ** -52
RATIOS = {}          # (variant, sum group) -> largest E_gpu / max(E_f64, 2^-52), printed at the end of the module


@pytest.fixture(scope="module")
def fixture():
    return mk.load()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for (variant, g), r in sorted(RATIOS.items()):
        print("largest E_gpu / max(E_f64, 2^-52): variant %-6s %-3s %.3g" % (variant, g, r))


def run_case(hip, case, options, trace):
    """One svnicp_iter_accumulate of `case` on a fresh context: dict(sums [P][22], corr [P][B] or None, ambiguous pairs,
    other: the row shard's other slot)."""
    import torch
    from svnicp_amd.sharded import _DevView
    L = hip.load_library()
    P, B, K = case.P, case.B, case.K
    init = np.zeros((6, P))
    prm = hip.SteinICPParam(iterations=1, lr=1.0, max_dist=case.max_dist, KNN_count=K, record_trace=trace)
    if case.svgd:
        prm.optimizer = "Adam"
    s = (hip.SVGDICP if case.svgd else hip.SVNICP)(prm, init)
    s.add_cloud(case.src, case.tgt, init)
    for k, v in options:
        s.set_option(k, v)
    if case.shard is not None:
        s._check(L.svnicp_set_shard(s.handle, case.shard[0], case.shard[1]), "svnicp_set_shard")
    if case.row_shard is not None:
        s._check(L.svnicp_set_row_shard(s.handle, *case.row_shard), "svnicp_set_row_shard")
    s._check(L.svnicp_align_begin(s.handle), "svnicp_align_begin")
    s.synchronize()

    def view(fn, shape, dt):
        ptr = getattr(L, fn)(s.handle)
        assert ptr, fn
        return torch.as_tensor(_DevView(ptr, shape, dt), device="cuda")
    view("svnicp_candidates_devptr", (B, K), "<i4").copy_(torch.from_numpy(case.cand))
    view("svnicp_total_pose_devptr", (P, 12), "<f8").copy_(torch.from_numpy(case.poses))
    torch.cuda.synchronize()
    s._check(L.svnicp_build_candidate_table(s.handle), "svnicp_build_candidate_table")
    s._check(L.svnicp_iter_accumulate(s.handle, 0), "svnicp_iter_accumulate")
    s._check(L.svnicp_finish(s.handle), "svnicp_finish")
    s.synchronize()
    other = None
    if case.row_shard is not None:
        rank, world, _ = case.row_shard
        rec = view("svnicp_rank_sums_devptr", (world, P, 22), "<f8").cpu().numpy()
        sums, other = rec[rank], np.delete(rec, rank, 0)
    else:
        sums = view("svnicp_sums_devptr", (P, 22), "<f8").cpu().numpy()
    out = dict(sums=sums.copy(), corr=s.get_trace()["corr"][0].astype(np.int64) if trace else None, ambiguous=s.get_ambiguous_pairs(), other=other)
    s.close()
    return out


def run_guarded(hip, case, variant):
    """run_case; an error of the HIP runtime ends the session: nothing more is started on a device that has faulted."""
    options, trace = cases.variants(case)[variant]
    try:
        return run_case(hip, case, options, trace)
    except hip.SvnIcpError as e:
        pytest.exit("HIP error in case %s, variant %s: %s" % (case.name, variant, e), returncode=3)


def check_discrete(case, variant, out):
    D = case.discrete()
    lo, hi = case.particles()
    sums = out["sums"][lo:hi]
    assert np.isfinite(sums).all(), "%s: a sum is not finite" % variant
    if out["corr"] is not None:
        bad = np.argwhere(out["corr"][lo:hi] != D["win"][lo:hi])
        assert bad.size == 0, "%s: %d of %d winners differ from the reference, first (particle, row) %s: slot %d for %d" % (
            variant, len(bad), (hi - lo) * case.B, (bad[0] + (lo, 0)).tolist(), out["corr"][lo:hi][tuple(bad[0])], D["win"][lo:hi][tuple(bad[0])])
        assert (out["corr"][:lo] == -1).all() and (out["corr"][hi:] == -1).all(), "winners outside the shard were written"
    if "all_rejected" in case.tags:
        assert (sums[:, 0] == case.B).all() and not sums[:, 1:].any(), "%s: an all-rejected case gives sum w = B and 21 zeros" % variant
    if case.svgd:
        assert np.array_equal(sums[:, 4], D["cnt"][lo:hi].sum(1).astype(np.float64)), "%s: SVGD-ICP's count" % variant
    if out["other"] is not None:
        assert not out["other"].any(), "%s: the other rank's slot was written" % variant


def check_sums(case, variant, out, r):
    lo, hi = case.particles()
    v = out["sums"]
    idx = r["idx"]
    e = ref.error_against_mp(v[idx], r["v64"][idx], r["mag"][idx], r["eps"])
    worst = {}
    for g, ix in ref.GROUPS:
        ratio = float(e[:, list(ix)].max()) / max(r["yard"][g], FLOOR)
        worst[g] = ratio
        RATIOS[(variant, g)] = max(RATIOS.get((variant, g), 0.0), ratio)
        print("%s %s %s: E_gpu %.3e, E_f64 %.3e, ratio %.3g" % (case.name, variant, g, e[:, list(ix)].max(), r["yard"][g], ratio))
    for g, _ in ref.GROUPS:
        assert worst[g] <= FACTOR, "%s %s: E_gpu is %.3g x max(E_f64, 2^-52), the bar is %g" % (variant, g, worst[g], FACTOR)
    rest = np.setdiff1d(np.arange(lo, hi), idx)
    if rest.size:
        bar = 2 * FACTOR * max(max(r["yard"].values()), FLOOR)
        with np.errstate(all="ignore"):
            e2 = np.abs(v[rest] - r["v64"][rest]) / r["mag"][rest]
        assert e2.max() <= bar, "%s: a particle without mpmath sums is %.3e from the float64 restatement (bar %.3e)" % (variant, e2.max(), bar)


@pytest.mark.parametrize("case", cases.all_cases(), ids=lambda c: c.name)
def test_stage_b_alone(hip, fixture, case):
    r = mk.case_reference(fixture, case)
    assert r["chk"] == int(case.checksum()) and r["crc_ok"], "tests/golden/stage_b.npz is stale: run tests/golden/make_stage_b.py"
    outs = {v: run_guarded(hip, case, v) for v in cases.variants(case)}
    again = run_guarded(hip, case, "plain")
    lo, hi = case.particles()
    for v, out in outs.items():
        check_discrete(case, v, out)
    assert np.array_equal(outs["plain"]["sums"][lo:hi], again["sums"][lo:hi]), "the same case run twice differs"
    assert np.array_equal(outs["plain"]["sums"][lo:hi], outs["traced"]["sums"][lo:hi]), "plain and traced split differ"
    assert outs["plain"]["ambiguous"] == outs["traced"]["ambiguous"] == again["ambiguous"] >= 0 and outs["f64"]["ambiguous"] == -1
    if "ties" in case.tags:
        assert outs["plain"]["ambiguous"] >= int(case.discrete()["tie"][lo:hi].sum()), "a tied pair was decided in float32"
    for v, out in outs.items():
        check_sums(case, v, out, r)


def test_queue_overflow(hip):
    """More undecided pairs than a search workgroup's queue holds: `full` ties every pair, `holes` 48 lanes of each 64, so that a
    step straddles the end of the queue.  Reference: the discrete part and the float64 sums."""
    import torch
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    for case in cases.overflow_cases(num_cus):
        assert case.B * case.P // num_cus >= 2 * cases.QUEUE_CAP
        D = case.discrete()
        v64, mag = mk.f64_sums(case)
        bar = (2 * case.B + 20) * 2.0 ** -53
        outs = {v: run_guarded(hip, case, v) for v in ("plain", "traced", "f64", "valu")}
        for v, out in outs.items():
            check_discrete(case, v, out)
            with np.errstate(all="ignore"):
                e = np.abs(out["sums"] - v64) / np.maximum(mag, mk.TINY)
            print("%s %s: largest |v - v_f64| / sum|term| %.3e (bar %.3e), ambiguous pairs %d" % (case.name, v, e.max(), bar, out["ambiguous"]))
            assert e.max() <= bar, (case.name, v, e.max())
        assert np.array_equal(outs["plain"]["sums"], outs["traced"]["sums"])
        for v in ("plain", "traced"):
            assert outs[v]["ambiguous"] == case.facts["expected_ambiguous"], (case.name, v, outs[v]["ambiguous"])
