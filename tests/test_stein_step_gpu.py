"""The Stein step alone on the GPU, against the mpmath reference of tests/golden/stein_step.npz.

Every case of tests/stein_step_cases.py runs through every launch shape that admits it (stein_step_cases.shapes): a fresh
context with record_trace, tiny clouds that are never searched, svnicp_align_begin, the case's sums written straight into
svnicp_sums_devptr (svnicp_rank_sums_devptr for a row shard), ONE svnicp_iter_update (three for the SVGD-ICP optimizer
sequences; mode SVGD reaches k_particle_update_svgd and the chain with svgd = 1 through the same options), svnicp_finish.  Stage A and stage B
never run, so a case takes milliseconds.  Needs numpy, torch and the fixture only.

Which shape ran is known indirectly: the options were accepted, and which launches they select is the pure function
plan_step of registration_plan.hpp that tests/test_registration_plan_cpu.py pins; P = 1 reports h = NaN (no pair statistics).
finish_iter is read as svnicp_get_iterations_run (the device's control word): svnicp_get_runtime needs the stage-A event that
a registration without stage A never records.

Compared exactly: the non-finite pattern of every quantity, the stop decision, iterations run, the zero history row after a
stop, the median's key (h log(P + 1) gives it back to 2 ulp, for the cases on a binary grid), H and b of a row shard bit for bit.
Compared to the bar: E = max |v - v_mp| / max(max |v_mp|, 1e-300) per particle and quantity must not exceed
16 max(E_oracle, 2^-52), E_oracle being the float64 oracle's E on the same case out of the fixture; two shapes of one case
differ by no more than twice that.
"""
import importlib.util
import os

import numpy as np
import pytest

import stein_step_cases as cases
import stein_step_reference as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_stein_step", os.path.join(HERE, "golden", "make_stein_step.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)

FACTOR, EPS = 16.0, 2.0 ** -52
B = M = 256
K, I = 8, mk.ITER    # more iterations allocated than run: iterations_run is 1 after a stop and I without
assert B == cases.N_SRC
RATIOS = {}          # (shape, quantity) -> largest E_gpu / max(E_oracle, 2^-52), printed at the end of the module


@pytest.fixture(scope="module")
def fixture():
    return mk.load()


@pytest.fixture(scope="module")
def clouds():
    g = np.arange(B, dtype=np.float64)
    src = np.stack([g % 8, (g // 8) % 8, g // 64], 1) * 0.5
    return src, src + 0.01


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for (shape, q), r in sorted(RATIOS.items()):
        print("largest E_gpu / max(E_oracle, 2^-52): shape %-7s %-5s %.3g" % (shape, q, r))


def run_step(hip, clouds, case, options):
    """One svnicp_iter_update of `case` on a fresh context; the outputs in the layout of stein_step_reference.svn_step."""
    import torch
    from svnicp_amd.sharded import _DevView
    L = hip.load_library()
    P, W = case.P, case.W
    prm = hip.SteinICPParam(iterations=I, lr=case.lr, max_dist=1.0, KNN_count=K, SVN_full_grad=case.full, check_early_stop=case.es,
                            convergence_threshold=case.thr, record_trace=True)
    if case.mode == "svgd":
        prm.optimizer = case.optimizer
    s = (hip.SVGDICP if case.mode == "svgd" else hip.SVNICP)(prm, case.init)
    s.add_cloud(clouds[0], clouds[1], case.init)
    for k, v in options:
        s.set_option(k, v)
    if W > 1:
        s._check(L.svnicp_set_row_shard(s.handle, 0, W, B * W), "svnicp_set_row_shard")
    s._check(L.svnicp_align_begin(s.handle), "svnicp_align_begin")
    s.synchronize()
    if W > 1:
        dst = torch.as_tensor(_DevView(L.svnicp_rank_sums_devptr(s.handle), (W, P, 22), "<f8"), device="cuda")
        dst.copy_(torch.from_numpy(np.ascontiguousarray(case.sums)))
    else:
        dst = torch.as_tensor(_DevView(L.svnicp_sums_devptr(s.handle), (P, 22), "<f8"), device="cuda")
        dst.copy_(torch.from_numpy(np.ascontiguousarray(case.sums[0])))
    torch.cuda.synchronize()
    for it in range(case.steps):   # (the sums stay where they are: every update of a sequence reads the same record)
        s._check(L.svnicp_iter_update(s.handle, it), "svnicp_iter_update")
    s._check(L.svnicp_finish(s.handle), "svnicp_finish")
    s.synchronize()
    tr = s.get_trace(with_corr=False)
    hist = s.get_particle_history()
    last = case.steps - 1
    out = dict(H=tr["H"][last].reshape(P, 36), b=tr["b"][last], N=tr["newton"][last], phi=tr["phi"][last], h=np.float64(tr["h"][last]),
               pose=s.get_particles().reshape(6, P), hist=hist[last], hist_rest=hist[last + 1:], stop=bool(L.svnicp_stopped(s.handle)),
               iters=s.get_iterations_run())
    s.close()
    return out


def run_guarded(hip, clouds, case, options):
    """run_step; an error of the HIP runtime ends the session: nothing more is started on a device that has faulted."""
    try:
        return run_step(hip, clouds, case, options)
    except hip.SvnIcpError as e:
        pytest.exit("HIP error in case %s with options %r: %s" % (case.name, options, e), returncode=3)


def check_against_reference(case, shape, out, r):
    idx = r["idx"]
    got = mk.subset(out, idx)
    assert out["stop"] == r["stop"], "stop decision"
    assert out["iters"] == (1 if r["stop"] else I), "iterations run / finish_iter"
    assert not out["hist_rest"].any(), "history rows of iterations that never ran"
    if r["stop"]:
        assert not out["hist"].any(), "the stopping epoch's history row must stay zero"
    if case.exact_h:
        assert ref.same_median(out["h"], r["med"], case.P), "h %r does not give the median %r back" % (out["h"], r["med"])
    quantities = [q for q in ref.QUANTITIES if r.get(q) is not None]
    worst = {}
    for q in quantities:
        v, w = ref.compared(got, q), ref.compared(r, q)
        e = ref.rel_err(v, w)
        assert e is not None, "%s: non-finite pattern differs from the reference\n%r\n%r" % (q, v, w)
        ratio = float(e.max()) / max(r["eo"][q], EPS)
        worst[q] = ratio
        RATIOS[(shape, q)] = max(RATIOS.get((shape, q), 0.0), ratio)
        print("%s %s %s: E_gpu %.3e, E_oracle %.3e, ratio %.3g" % (case.name, shape, q, e.max(), r["eo"][q], ratio))
    for q in quantities:
        assert worst[q] <= FACTOR, "%s: E_gpu is %.3g x max(E_oracle, 2^-52), the bar is %g" % (q, worst[q], FACTOR)


@pytest.mark.parametrize("case", cases.all_cases(), ids=lambda c: c.name)
def test_stein_step_alone(hip, fixture, clouds, case):
    r = mk.case_reference(fixture, case)
    assert r["chk"] == int(case.checksum()), "tests/golden/stein_step.npz is stale: run tests/golden/make_stein_step.py"
    outs = {}
    for shape, options in cases.shapes(case.P).items():
        outs[shape] = run_guarded(hip, clouds, case, options)
    for shape, out in outs.items():
        assert case.P > 1 or np.isnan(out["h"]), "one particle has no bandwidth"
        check_against_reference(case, shape, out, r)
    # the shapes against each other, every particle: within twice the bar
    names = list(outs)
    for q in ("N", "phi", "pose"):
        bar = 2 * FACTOR * max(r["eo"][q], EPS)
        for n in names[1:]:
            a, b = (outs[names[0]][q], outs[n][q]) if q != "pose" else (outs[names[0]][q].T, outs[n][q].T)
            e = ref.rel_err(b, a)
            assert e is not None, "%s: shapes %s and %s differ in their non-finite pattern" % (q, names[0], n)
            assert e.max() <= bar, "%s: shapes %s and %s differ by %.3e (bar %.3e)" % (q, names[0], n, e.max(), bar)


@pytest.mark.parametrize("case", [c for c in cases.all_cases() if "shard" in c.tags], ids=lambda c: c.name)
def test_row_shard_records_added_in_rank_order(hip, clouds, case):
    """H and b of the trace equal, bit for bit, the finalisation of the numpy left-to-right sum of the W records (the order
    svnicp_hip.h promises), and not that of another order."""
    F = ref.F64()
    eye = [np.float64(v) for v in (1, 0, 0, 0, 1, 0, 0, 0, 1)]

    def finalised(red):
        Hs, bs = [], []
        for p in range(case.P):
            H, b = ref.finalize_Hb(F, [np.float64(v) for v in red[p]], eye)
            Hs.append(H); bs.append(b)
        return np.array(Hs, np.float64), np.array(bs, np.float64)
    H, b = finalised(ref.reduce_sums(case.sums))
    Hrev, brev = finalised(ref.reduce_sums(case.sums, reverse=True))
    assert not (np.array_equal(H, Hrev) and np.array_equal(b, brev))
    for shape, options in cases.shapes(case.P).items():
        out = run_guarded(hip, clouds, case, options)
        assert np.array_equal(out["H"], H) and np.array_equal(out["b"], b), shape
