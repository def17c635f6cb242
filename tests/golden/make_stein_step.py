"""tests/golden/make_stein_step.py — regenerates tests/golden/stein_step.npz.

For every case of tests/stein_step_cases.py: the mpmath (60 digits) restatement of the Stein step
(tests/stein_step_reference.py) rounded to double, and the float64 oracle's own error against it — the yardstick of
tests/test_stein_step_gpu.py, which reads this file and needs no mpmath.  The inputs are not stored: the cases module
rebuilds them (numpy only); a checksum of them is.  Beyond 16 particles only the particles of
stein_step_cases.compared_particles are kept, and of them what is compared (phi, the new pose; the history row is the
pose rounded to float32, or zero after a stop).

Run from the repo root:  python tests/golden/make_stein_step.py
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import stein_step_cases as cases  # noqa: E402
import stein_step_reference as ref  # noqa: E402

FIXTURE = os.path.join(HERE, "stein_step.npz")
SMALL = 16   # particle count up to which H, b and N are kept too
ITER = 4     # iterations a context is made for: one is run (three by the seq3 cases), iterations_run tells a stop apart


def oracle_step(orc, case):
    """The float64 oracle used piecewise: so3_exp for the initial rotation, H and b finalised in numpy from the reduced sums,
    then orc_sp_update (solve6, inv6, the median by qsort, so3_exp, so3_log) on the [P][42] records."""
    if case.mode == "svgd":   # the oracle has no split-phase SVGD entry: the plain float64 step is the yardstick there
        return dict(case.step(), iters=ITER)
    L = orc.lib()
    P = case.P
    F = ref.F64()
    s = orc.Solver(case.init, iterations=ITER, lr=case.lr, check_early_stop=case.es, convergence_threshold=case.thr, knn_count=8,
                   svn_full_grad=case.full)
    L.orc_sp_begin(s.h)
    bufs = dict(H=np.zeros((ITER, P, 36)), b=np.zeros((ITER, P, 6)), newton=np.zeros((ITER, P, 6)), phi=np.zeros((ITER, P, 6)),
                h=np.zeros(ITER))
    t = orc.Trace(None, None, *[bufs[k].ctypes.data for k in ("H", "b", "newton", "phi", "h")], None)
    L.orc_set_trace(s.h, C.byref(t))
    red = case.reduced()
    rec = np.zeros((P, 42))
    with np.errstate(all="ignore"):
        for p in range(P):
            R, _ = orc.so3_exp(case.init[3:, p])
            H, b = ref.finalize_Hb(F, [np.float64(v) for v in red[p]], [np.float64(v) for v in R.reshape(9)])
            rec[p, :36], rec[p, 36:] = H, b
    stop = bool(L.orc_sp_update(s.h, 0, rec.ctypes.data_as(C.POINTER(C.c_double))))
    L.orc_sp_finish(s.h)
    return dict(H=bufs["H"][0], b=bufs["b"][0], N=bufs["newton"][0], phi=bufs["phi"][0], h=np.float64(bufs["h"][0]),
                pose=s.get_particles().reshape(6, P), hist=s.get_particle_history()[0], stop=stop, iters=s.iterations_run())


def subset(out, idx):
    """The compared particles of a step's outputs."""
    P = out["pose"].shape[1]
    o = dict(out)
    for q in ("H", "b", "N", "phi"):
        o[q] = out[q][idx]
    o["pose"] = out["pose"][:, idx]
    o["hist"] = np.asarray(out["hist"]).reshape(6, P)[:, idx].reshape(-1)
    return o


def reference_step(A, case):
    if case.mode == "svgd":
        return ref.svgd_steps(A, case.init, case.reduced(), case.lr, case.optimizer, cases.N_SRC, case.steps)
    return ref.svn_step(A, case.init, case.reduced(), case.full, case.lr, case.es, case.thr)


def generate(orc, only=None):
    """{array name: array} of the fixture."""
    A = ref.MP()
    d = {}
    for c in cases.all_cases():
        if only and c.name not in only:
            continue
        idx = cases.compared_particles(c.P)
        r = reference_step(A, c)
        o = oracle_step(orc, c)
        assert o["stop"] == r["stop"], c.name
        e = ref.errors(subset(o, idx), subset(r, idx))
        assert None not in e.values(), (c.name, e)
        rs = subset(r, idx)
        parts = [[c.checksum(), r["stop"], r["h"], r["med"]], [e[q] for q in ref.QUANTITIES], [len(idx)], idx, rs["phi"], rs["pose"]]
        if c.P <= SMALL:
            parts += [rs["H"], rs["b"], rs["N"]]
        d[c.name] = np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in parts])   # one record per case
    return d


def load(path=FIXTURE):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def case_reference(fix, case):
    """A case's reference outputs out of the fixture, in the layout of subset(); r["chk"] is the checksum of its inputs."""
    v = fix[case.name]
    nq = len(ref.QUANTITIES)
    n = int(v[4 + nq])
    r = dict(chk=int(v[0]), stop=bool(v[1]), h=np.float64(v[2]), med=np.float64(v[3]), eo=dict(zip(ref.QUANTITIES, v[4:4 + nq])))
    at = 5 + nq
    r["idx"] = v[at:at + n].astype(np.int64); at += n
    r["phi"] = v[at:at + 6 * n].reshape(n, 6); at += 6 * n
    r["pose"] = v[at:at + 6 * n].reshape(6, n); at += 6 * n
    r["H"] = r["b"] = r["N"] = None
    if case.P <= SMALL:
        r["H"] = v[at:at + 36 * n].reshape(n, 36); at += 36 * n
        r["b"] = v[at:at + 6 * n].reshape(n, 6); at += 6 * n
        r["N"] = v[at:at + 6 * n].reshape(n, 6); at += 6 * n
    assert at == v.size, case.name
    if case.mode == "svgd":   # no Hessian in SVGD-ICP: the traces of H and b are not written
        r["H"] = r["b"] = None
    r["pose_t"] = r["pose"][:3].T
    r["hist"] = np.zeros(r["pose"].size, np.float32) if r["stop"] else r["pose"].reshape(-1).astype(np.float32)
    return r


def main():
    import __graft_entry__ as graft
    orc = graft.load_oracle()
    orc.build()
    d = generate(orc)
    np.savez_compressed(FIXTURE, **d)
    print("%s: %d cases, %d bytes" % (FIXTURE, len(cases.all_cases()), os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    main()
