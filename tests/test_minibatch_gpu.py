"""Mini-batch Stein ICP on the device (SteinICPParam.use_minibatch / batch_size; include/svnicp_hip.h "mini-batch").

The oracle has no mini-batch switch and needs none: iteration i of a mini-batch run is ONE full-batch iteration on the cloud
src[idx[i]] started from the particles iteration i-1 left (tests/test_minibatch_cpu.py pins that identity on the oracle
alone), and a constant table is one ordinary run on src[L].  Correspondences are held to equality; H, b, phi and h to
|a - b| <= TIGHT + TIGHT * |b| (sums over the batch are far larger than 1, so the bound has a relative part; TIGHT = 1e-9 from
tests/helpers.py), poses and statistics to TIGHT absolute."""
import os
import subprocess

import numpy as np
import pytest

from helpers import TIGHT

pytestmark = pytest.mark.gpu

R0 = None


def _near(a, b):
    return np.allclose(a, b, rtol=TIGHT, atol=TIGHT)


def _prm(pkg, mode_cfg, trace=True, **over):
    c = dict(mode_cfg, **over)
    return pkg.SteinICPParam(iterations=c["iterations"], lr=c["lr"], max_dist=c["max_dist"],
                             check_early_stop=c.get("check_early_stop", False),
                             convergence_threshold=c.get("convergence_threshold", 1e-5), KNN_count=c["knn_count"],
                             SVN_full_grad=c.get("svn_full_grad", False), optimizer=c.get("optimizer", "Adam"), record_trace=trace)


def _table(B, I, batch, seed):
    t = np.random.default_rng(seed).integers(0, B, size=(I, batch)).astype(np.int32)
    if batch > 1:
        t[:, 1] = t[:, 0]          # a row drawn twice counts twice
    return t


def _phi_norm(phi):
    return float(np.mean(np.sqrt((phi.reshape(-1, 6) ** 2).sum(1))))


def _chain(orc, mode, cfg, src, tgt, idx, init, lr=None, stop_thr=None):
    """The chained oracle: one full-batch iteration per table row.  Returns (per-iteration traces, the last step's solver,
    iterations run)."""
    p = np.array(init, np.float64)
    traces, o = [], None
    for i in range(idx.shape[0]):
        c = dict(cfg, iterations=1)
        if lr is not None:
            c["lr"] = lr
        o = orc.Solver(p, mode=mode, **c)
        o.add_cloud(src[idx[i]], tgt, p)
        tr = o.enable_trace()
        o.stein_align()
        traces.append({k: v[0].copy() for k, v in tr.items()})
        if stop_thr is not None and np.float32(_phi_norm(tr["phi"][0])) < np.float32(stop_thr):
            return traces, o, i + 1
        p = o.get_particles().reshape(6, -1)
    return traces, o, idx.shape[0]


# ------------------------------------------------------------------ 1. the generated table
def test_generated_table_matches_python_mirror(hip):
    P, B, M, K, I, batch, seed = 4, 3000, 6000, 8, 5, 700, 12345
    src, tgt = hip.scans.random_clouds(B, M, seed=2)
    init = hip.scans.make_particles(P, seed=2) * 0.2
    s = hip.SVNICP(hip.SteinICPParam(iterations=I, lr=1.0, KNN_count=K, SVN_full_grad=False, use_minibatch=True, batch_size=batch,
                                     minibatch_seed=seed), init)
    for n in range(3):
        s.add_cloud(src, tgt, init)
        s.stein_align()
        got = s.get_minibatch_indices()
        assert got.shape == (I, batch)
        assert np.array_equal(got, hip.minibatch_indices(seed, n, I, batch, B)), f"registration {n}"
        U, nq = s.get_minibatch_rows()
        assert U == len(np.unique(got)) and U <= nq <= min(B, I * batch)


# ------------------------------------------------------------------ 2. candidates of the drawn rows
@pytest.mark.parametrize("knn", ["brute", "tiles", None])
@pytest.mark.parametrize("case", ["few", "all", "wide"])
def test_minibatch_candidates_exact(hip, orc, knn, case):
    K, P = 16, 4
    B, M, I, batch = {"few": (4000, 20000, 3, 50), "all": (300, 20000, 4, 450), "wide": (500, 9000, 2, 1200)}[case]
    src, tgt = hip.scans.random_clouds(B, M, seed=B + K, extent=40.0)
    init = hip.scans.make_particles(P, seed=1) * 0.1
    R0, t0 = hip.scans.rot_zyx(0.001, 0.002, -0.001), np.array([0.01, -0.02, 0.005])
    idx = _table(B, I, batch, seed=B)
    if case == "all":
        idx[0, :B] = np.random.default_rng(1).permutation(B)      # every row is drawn
    s = hip.SVNICP(hip.SteinICPParam(iterations=I, lr=1.0, KNN_count=K, SVN_full_grad=False, record_trace=True), init)
    if knn:
        s.set_option("knn", knn)
    s.set_minibatch_indices(idx)
    s.add_cloud(src, tgt, init); s.set_initial_mean((R0, t0))
    s.stein_align()
    want = orc.knn_topk(orc.transform(src, R0, t0), tgt, K)[0][idx]
    assert np.array_equal(s.get_minibatch_indices(), idx)
    assert np.array_equal(s.get_minibatch_candidates().astype(np.int64), want)
    U, nq = s.get_minibatch_rows()
    assert U == len(np.unique(idx)) and U <= nq <= min(B, I * batch)
    if case == "all":
        assert U == B
    with pytest.raises(hip.SvnIcpError, match="svnicp_get_minibatch_candidates"):
        s.get_candidates()
    assert s.get_trace()["corr"].shape == (I, P, batch)


# ------------------------------------------------------------------ 3. identity table == full batch
def test_identity_table_equals_full_batch(hip, orc):
    P, B, M, K, I = 16, 1500, 6000, 32, 6
    src, tgt = hip.scans.random_clouds(B, M, seed=9)
    init = hip.scans.make_particles(P, seed=9) * 0.3
    cfg = dict(iterations=I, lr=1.0, max_dist=1.0, knn_count=K, svn_full_grad=False)
    full = hip.SVNICP(_prm(hip, cfg), init); full.add_cloud(src, tgt, init); full.stein_align()
    s = hip.SVNICP(_prm(hip, cfg), init)
    s.set_minibatch_indices(np.tile(np.arange(B, dtype=np.int32), (I, 1)))
    s.add_cloud(src, tgt, init); s.stein_align()
    o = orc.Solver(init, **cfg); o.add_cloud(src, tgt, init); o.stein_align()
    assert np.array_equal(s.get_trace()["corr"], full.get_trace()["corr"])
    for ref in (full, o):
        assert np.allclose(s.get_particles(), ref.get_particles(), rtol=0, atol=TIGHT)
        assert np.allclose(s.get_transformation(), ref.get_transformation(), rtol=0, atol=TIGHT)
        assert np.allclose(s.get_cov_matrix(), ref.get_cov_matrix(), rtol=0, atol=TIGHT)
        assert np.allclose(s.get_distribution(), ref.get_distribution(), rtol=0, atol=TIGHT)
        assert np.allclose(s.get_particle_history(), ref.get_particle_history(), rtol=0, atol=TIGHT)


# ------------------------------------------------------------------ 4. chain identity, SVN, every stage-B plan
CHAIN = [
    # P, B, M, K, I, batch, full, options
    (1, 1000, 4000, 16, 6, 300, False, {}),                       # k_icp_single
    (4, 1000, 4000, 16, 6, 300, True, {}),                        # <= 8-particle kernels
    (30, 2000, 8000, 32, 6, 500, False, {}),                      # small chain
    (128, 4096, 10000, 100, 5, 2048, False, {}),                  # small chain, batch * P = 2^18
    (128, 8192, 16000, 100, 4, 6000, False, {}),                  # general chain (batch * P > 2^19)
    (200, 2000, 6000, 24, 4, 700, True, {}),                      # pair statistics on the second stream
    (16, 3000, 9000, 150, 4, 800, False, {}),                     # K > 128: LDS-tile search
    (30, 2000, 8000, 32, 5, 500, False, {"accum": "f64"}),
    (30, 2000, 8000, 32, 5, 500, True, {"accum": "valu"}),
    (30, 2000, 8000, 32, 5, 500, False, {"chain": "general"}),
]


@pytest.mark.parametrize("P,B,M,K,I,batch,full,opts", CHAIN)
def test_chain_identity_svn(hip, orc, P, B, M, K, I, batch, full, opts):
    src, tgt = hip.scans.random_clouds(B, M, seed=P + B)
    init = hip.scans.make_particles(P, seed=P) * 0.3
    cfg = dict(iterations=I, lr=0.5 if full else 1.0, max_dist=1.0, knn_count=K, svn_full_grad=full)
    idx = _table(B, I, batch, seed=P + batch)
    s = hip.SVNICP(_prm(hip, cfg), init)
    for k, v in opts.items():
        s.set_option(k, v)
    s.set_minibatch_indices(idx)
    s.add_cloud(src, tgt, init)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    traces, o, n = _chain(orc, orc.MODE_SVN, cfg, src, tgt, idx, init)
    tr = s.get_trace()
    assert s.get_iterations_run() == n == I
    for it in range(I):
        assert np.array_equal(tr["corr"][it], traces[it]["corr"]), f"correspondences of iteration {it}"
        for k in ("H", "b", "phi"):
            assert _near(tr[k][it], traces[it][k]), f"{k} of iteration {it}: {np.abs(tr[k][it] - traces[it][k]).max():.3e}"
        if P > 1:
            assert _near(tr["h"][it], traces[it]["h"]), f"h of iteration {it}"
    assert np.allclose(s.get_particles(), o.get_particles(), rtol=0, atol=TIGHT)
    assert np.allclose(s.get_transformation(), o.get_transformation(), rtol=0, atol=TIGHT)
    assert np.allclose(s.get_cov_matrix(), o.get_cov_matrix(), rtol=0, atol=TIGHT)
    assert np.allclose(s.get_distribution(), o.get_distribution(), rtol=0, atol=TIGHT)


# ------------------------------------------------------------------ 5. early stop inside the chain
@pytest.mark.parametrize("entry", ["align", "async"])
def test_chain_early_stop(hip, orc, entry):
    P, B, M, K, I, batch = 8, 512, 2048, 32, 14, 400
    src, tgt = hip.scans.random_clouds(B, M, seed=P + B)
    init = hip.scans.make_particles(P, seed=P) * 0.3
    cfg = dict(iterations=I, lr=1.0, max_dist=1.0, knn_count=K, svn_full_grad=True)
    idx = _table(B, I, batch, seed=77)
    traces, _, _ = _chain(orc, orc.MODE_SVN, cfg, src, tgt, idx, init)
    m = [_phi_norm(t["phi"]) for t in traces]
    print("mean |phi| per iteration:", ["%.3e" % x for x in m])
    stop = next((j for j in range(3, I - 2) if m[j] < min(m[:j])), None)
    assert stop is not None, "no running minimum strictly inside (2, I-2): pick other clouds"
    thr = 0.5 * (m[stop] + min(m[:stop]))
    cfg_es = dict(cfg, check_early_stop=True, convergence_threshold=thr)
    _, o, n = _chain(orc, orc.MODE_SVN, cfg_es, src, tgt, idx, init, stop_thr=thr)
    assert n == stop + 1
    s = hip.SVNICP(_prm(hip, cfg_es, trace=False), init)
    s.set_minibatch_indices(idx)
    s.add_cloud(src, tgt, init)
    if entry == "align":
        s.stein_align()
    else:
        s.stein_align_async(); s.synchronize()
    assert s.get_iterations_run() == n
    assert np.allclose(s.get_particles(), o.get_particles(), rtol=0, atol=TIGHT)


# ------------------------------------------------------------------ 6. constant table == one oracle run on src[L]
def _same_outputs(s, o):
    assert np.allclose(s.get_particles(), o.get_particles(), rtol=0, atol=TIGHT)
    assert np.allclose(s.get_transformation(), o.get_transformation(), rtol=0, atol=TIGHT)
    assert np.allclose(s.get_cov_matrix(), o.get_cov_matrix(), rtol=0, atol=TIGHT)
    assert np.allclose(s.get_distribution(), o.get_distribution(), rtol=0, atol=TIGHT)
    assert np.allclose(s.get_particle_history(), o.get_particle_history(), rtol=0, atol=TIGHT)
    assert int(s.get_runtime()[2]) == o.finish_iter() and s.get_iterations_run() == o.iterations_run()


def test_constant_table_svn(hip, orc):
    P, B, M, K, I, batch = 12, 1000, 4000, 16, 7, 300
    src, tgt = hip.scans.random_clouds(B, M, seed=21)
    init = hip.scans.make_particles(P, seed=21) * 0.3
    cfg = dict(iterations=I, lr=1.0, max_dist=1.0, knn_count=K, svn_full_grad=False)
    L = _table(B, 1, batch, seed=5)[0]
    s = hip.SVNICP(_prm(hip, cfg), init)
    s.set_minibatch_indices(np.tile(L, (I, 1)))
    s.add_cloud(src, tgt, init); s.stein_align()
    o = orc.Solver(init, **cfg); o.add_cloud(src[L], tgt, init); o.stein_align()
    _same_outputs(s, o)


@pytest.mark.parametrize("opt,lr,es", [("Adam", 0.01, False), ("RMSprop", 0.01, False), ("SGD", None, False), ("Adagrad", 0.01, False),
                                       ("Adam", 0.01, True)])
def test_constant_table_svgd(hip, orc, opt, lr, es):
    P, B, M, K, I = 12, 600, 3000, 16, 8
    src, tgt = hip.scans.random_clouds(B, M, seed=41)
    init = hip.scans.make_particles(P, seed=41) * 0.3
    cfg = dict(iterations=I, lr=lr if lr else 1e-3 / B, max_dist=1.0, check_early_stop=es, convergence_threshold=0.05 if es else 1e-9,
               knn_count=K, optimizer=opt)
    L = _table(B, 1, B, seed=6)[0]          # len(L) == B: the scaling factor is what the oracle uses for a cloud of that size
    s = hip.SVGDICP(_prm(hip, cfg), init)
    s.set_minibatch_indices(np.tile(L, (I, 1)))
    s.add_cloud(src, tgt, init); s.stein_align()
    o = orc.Solver(init, mode=orc.MODE_SVGD, svn_full_grad=False, **{k: v for k, v in cfg.items() if k != "svn_full_grad"})
    o.add_cloud(src[L], tgt, init); o.stein_align()
    if es:
        assert o.iterations_run() < I, "the early stop must fire for this case to mean anything"
    _same_outputs(s, o)


# ------------------------------------------------------------------ 7. SVGD, per-iteration tables, batch < B
def test_chain_identity_svgd_sgd_one_particle(hip, orc):
    B, M, K, I, batch = 800, 3000, 16, 8, 200
    src, tgt = hip.scans.random_clouds(B, M, seed=33)
    init = np.zeros((6, 1))
    cfg = dict(iterations=I, lr=1e-3 / B, max_dist=1.0, knn_count=K, optimizer="SGD")
    idx = _table(B, I, batch, seed=8)
    s = hip.SVGDICP(_prm(hip, cfg), init)
    s.set_minibatch_indices(idx)
    s.add_cloud(src, tgt, init); s.stein_align()
    # gradient_scaling_factor_ stays the WHOLE cloud's size B; the chained oracle step scales by its cloud's size `batch`
    traces, o, _ = _chain(orc, orc.MODE_SVGD, cfg, src, tgt, idx, init, lr=cfg["lr"] * B / batch)
    tr = s.get_trace()
    for it in range(I):
        assert np.array_equal(tr["corr"][it], traces[it]["corr"]), f"correspondences of iteration {it}"
    assert np.abs(o.get_particles()).max() > 1e-6
    assert np.allclose(s.get_particles(), o.get_particles(), rtol=0, atol=TIGHT)


# ------------------------------------------------------------------ 8. one context: full batch -> mini-batch -> other size -> off
def test_context_reuse(hip):
    P, B, M, K, I = 16, 1200, 5000, 16, 5
    src, tgt = hip.scans.random_clouds(B, M, seed=3)
    init = hip.scans.make_particles(P, seed=3) * 0.3
    prm = hip.SteinICPParam(iterations=I, lr=1.0, KNN_count=K, SVN_full_grad=False)
    fresh = hip.SVNICP(prm, init); fresh.add_cloud(src, tgt, init); fresh.stein_align()
    want = fresh.get_particles()
    s = hip.SVNICP(prm, init)
    s.add_cloud(src, tgt, init); s.stein_align()
    assert np.array_equal(s.get_particles(), want)
    s.set_minibatch(300, 1); s.add_cloud(src, tgt, init); s.stein_align()
    a = s.get_particles()
    assert s.get_minibatch_indices().shape == (I, 300) and not np.array_equal(a, want)
    s.set_minibatch(2000, 1); s.add_cloud(src, tgt, init); s.stein_align()
    assert s.get_minibatch_indices().shape == (I, 2000) and s.get_minibatch_rows()[1] == B
    s.set_minibatch(0); s.add_cloud(src, tgt, init); s.stein_align()
    assert np.array_equal(s.get_particles(), want)
    assert s.get_candidates().shape == (B, K)
    with pytest.raises(hip.SvnIcpError):
        s.get_minibatch_rows()


# ------------------------------------------------------------------ 9. refusals
def test_refusals(hip):
    P, B, M, K, I = 6, 400, 2000, 8, 4
    src, tgt = hip.scans.random_clouds(B, M, seed=4)
    init = hip.scans.make_particles(P, seed=4) * 0.2
    prm = hip.SteinICPParam(iterations=I, lr=1.0, KNN_count=K, SVN_full_grad=False)
    L = hip.load_library()

    def refused(s, what):
        rc = L.svnicp_align_begin(s.handle)
        assert rc == -1, f"{what}: svnicp_align_begin returned {rc}"
        assert L.svnicp_last_error(s.handle), what
        with pytest.raises(hip.SvnIcpError):
            s.stein_align()

    def usable(s):
        s.set_minibatch(0); s.add_cloud(src, tgt, init)
        assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS

    def solver(batch=100):
        s = hip.SVNICP(prm, init); s.add_cloud(src, tgt, init); s.set_minibatch(batch, 0)
        return s

    s = solver(); assert L.svnicp_set_shard(s.handle, 0, 3) == 0; refused(s, "partial particle shard")
    assert L.svnicp_set_shard(s.handle, 0, P) == 0; usable(s)
    s = solver(); assert L.svnicp_set_row_shard(s.handle, 0, 2, 2 * B) == 0; refused(s, "row shard")
    assert L.svnicp_set_row_shard(s.handle, 0, 1, B) == 0; usable(s)
    s = solver(); s.set_option("correspondence", "full"); refused(s, "correspondence=full")
    s.set_option("correspondence", "fast"); usable(s)
    s = solver(); s.set_option("chain", "persistent"); refused(s, "chain=persistent")
    s.set_option("chain", "auto"); usable(s)
    s = solver(-5); refused(s, "negative batch size"); usable(s)
    s = solver((1 << 22) // I + 1); refused(s, "too many table rows"); usable(s)
    s = solver(); s.set_minibatch_indices(np.zeros((I + 1, 10), np.int32)); refused(s, "table shape"); usable(s)
    # split phase: only the whole row range
    s = solver()
    assert L.svnicp_align_begin(s.handle) == 0
    assert L.svnicp_stage_candidates(s.handle, 0, B // 2) == -1 and L.svnicp_last_error(s.handle)
    assert L.svnicp_stage_candidates(s.handle, 0, B) == 0
    usable(s)
    # bad values: host table (checked on the host), device table (checked by the kernel that reads it)
    import torch
    for bad in (B, -1):
        t = np.zeros((I, 50), np.int32); t[2, 7] = bad
        s = hip.SVNICP(prm, init); s.add_cloud(src, tgt, init); s.set_minibatch_indices(t)
        with pytest.raises(hip.SvnIcpError):
            s.stein_align()
        usable(s)
        s = hip.SVNICP(prm, init); s.add_cloud(src, tgt, init); s.set_minibatch_indices(torch.from_numpy(t).cuda())
        with pytest.raises(hip.SvnIcpError):
            s.stein_align()
        usable(s)
        s = hip.SVNICP(prm, init); s.add_cloud(src, tgt, init); s.set_minibatch_indices(torch.from_numpy(t).cuda())
        s.stein_align_async()
        with pytest.raises(hip.SvnIcpError):
            s.synchronize()
        usable(s)


def test_split_phase_one_shard_equals_align(hip):
    """svnicp_align_begin ... svnicp_finish with ONE shard is the code of svnicp_align, and advances the registration counter."""
    P, B, M, K, I, batch = 16, 900, 4000, 16, 5, 250
    src, tgt = hip.scans.random_clouds(B, M, seed=8)
    init = hip.scans.make_particles(P, seed=8) * 0.3
    prm = hip.SteinICPParam(iterations=I, lr=1.0, KNN_count=K, SVN_full_grad=False, use_minibatch=True, batch_size=batch, minibatch_seed=9)
    a = hip.SVNICP(prm, init)
    b = hip.SVNICP(prm, init)
    L = hip.load_library()
    for n in range(2):
        a.add_cloud(src, tgt, init); a.stein_align()
        b.add_cloud(src, tgt, init)
        assert L.svnicp_align_begin(b.handle) == 0 and L.svnicp_stage_candidates(b.handle, 0, B) == 0
        assert L.svnicp_build_candidate_table(b.handle) == 0
        for it in range(I):
            assert L.svnicp_iter_accumulate(b.handle, it) == 0 and L.svnicp_iter_update(b.handle, it) == 0
        assert L.svnicp_finish(b.handle) == 0
        b.synchronize()
        assert np.array_equal(b.get_minibatch_indices(), hip.minibatch_indices(9, n, I, batch, B))
        assert np.array_equal(a.get_particles(), b.get_particles())


# ------------------------------------------------------------------ 10. the C++ shim
def test_cpp_shim_minibatch(hip, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "minibatch_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-I",
                           os.path.join(root, "svn-icp_amd", "host"), os.path.join(root, "tests", "minibatch_driver.cpp"), "-L",
                           os.path.join(root, "svn-icp_amd"), "-lsvnicp_hip", "-Wl,-rpath," + os.path.join(root, "svn-icp_amd"),
                           "-o", exe])
    P, B, M, K, I, batch, seed = 8, 700, 3000, 16, 5, 200, 4242
    src, tgt = hip.scans.random_clouds(B, M, seed=10)
    init = hip.scans.make_particles(P, seed=10) * 0.2
    f = tmp_path / "in.bin"
    with open(f, "wb") as fh:
        np.array([P, B, M, K, I, batch], np.int64).tofile(fh)
        np.array([seed], np.uint64).tofile(fh)
        init.astype(np.float64).tofile(fh); src.tofile(fh); tgt.tofile(fh)
    r = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = next(l for l in r.stdout.splitlines() if l.startswith("RESULT"))
    vals = line.split()
    s = hip.SVNICP(hip.SteinICPParam(iterations=I, lr=1.0, max_dist=1.0, KNN_count=K, SVN_full_grad=False, use_minibatch=True,
                                     batch_size=batch, minibatch_seed=seed), init)
    s.add_cloud(src, tgt, init); s.stein_align()
    idx = s.get_minibatch_indices().astype(np.uint64).ravel()
    checksum = int((idx * (np.arange(idx.size, dtype=np.uint64) + np.uint64(1))).sum() & np.uint64((1 << 64) - 1))
    assert int(vals[1]) == checksum
    assert np.array_equal(np.array([float.fromhex(v) for v in vals[2:8]]), s.get_transformation())
