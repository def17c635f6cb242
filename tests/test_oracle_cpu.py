"""CPU tests of the oracle itself: pinned against the reference's own knn_cpu.cpp (its outputs stored under
tests/golden/knn_ref, and live through oracle/_ref where that is built), cross-checked against the op-for-op libtorch
restatement, and against the committed golden vectors."""
import os
import sys

import numpy as np
import pytest

from helpers import golden_cases, load_golden, oracle_from_golden, TIGHT
from conftest import so3_exp_np


# ---------------------------------------------------------------- KNN stage: pinned by the reference
KNN_REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_ref", "knn_cpu_ref.npz")


def _reference_knn(orc, case):
    """Inputs and outputs of the reference's float32 KNearestNeighborIdxCpu (unmodified, oracle/_ref) for one case, as
    stored by tests/golden/make_knn_ref.py.  Where oracle/_ref is built, the live call must reproduce them bit for bit."""
    g = np.load(KNN_REF, allow_pickle=False)
    q, t, K = g[case + "_q"], g[case + "_t"], int(g[case + "_k"])
    ri, rd = g[case + "_idx"], g[case + "_d2"]
    if orc.ref_available():
        li, ld = orc.ref_knn_cpu_f32(q, t, K)
        assert np.array_equal(li, ri) and np.array_equal(ld, rd), "oracle/_ref no longer gives the stored outputs"
    return q, t, K, ri, rd


@pytest.mark.parametrize("B,M,K", [(40, 300, 1), (64, 500, 7), (33, 257, 32), (16, 150, 100), (5, 3, 4)])
def test_knn_oracle_vs_reference_knn_cpu_with_ties(orc, B, M, K):
    """Integer-grid clouds: every distance is exact in float32 AND float64 and massively tied, so the
    reference's float32 KNearestNeighborIdxCpu (unmodified, oracle/_ref) must give bit-identical
    indices and distances to both the f32 twin and the f64 oracle loop: this pins selection,
    strict-'<' tie breaking (lowest index wins), ascending order and zero padding for M < K."""
    q, t, k, ri, rd = _reference_knn(orc, f"ties_{B}_{M}_{K}")
    assert q.shape == (B, 3) and t.shape == (M, 3) and k == K
    fi, fd = orc.knn_topk_f32(q, t, K)
    di, dd = orc.knn_topk(q, t, K)
    assert np.array_equal(ri, fi) and np.array_equal(rd, fd)
    assert np.array_equal(ri, di) and np.array_equal(rd.astype(np.float64), dd)
    if M >= K:  # ascending by (dist, idx)
        assert np.all(np.diff(dd, axis=1) >= 0)
        same = np.diff(dd, axis=1) == 0
        assert np.all(np.diff(di, axis=1)[same] > 0)
    else:
        assert np.all(di[:, M:] == 0) and np.all(dd[:, M:] == 0)


def test_knn_f32_twin_vs_reference_on_random_float_data(orc):
    q, t, K, ri, rd = _reference_knn(orc, "random")
    assert q.dtype == np.float32 and q.shape == (50, 3) and t.shape == (700, 3) and K == 20
    fi, fd = orc.knn_topk_f32(q, t, K)
    assert np.array_equal(ri, fi) and np.array_equal(rd, fd)


def test_knn_oracle_matches_definition(orc):
    rng = np.random.default_rng(5)
    q, t = rng.normal(size=(30, 3)), rng.normal(size=(400, 3))
    idx, d2 = orc.knn_topk(q, t, 9)
    dx = q[:, None, 0] - t[None, :, 0]; dy = q[:, None, 1] - t[None, :, 1]; dz = q[:, None, 2] - t[None, :, 2]
    d = (dx * dx + dy * dy) + dz * dz
    order = np.argsort(d, axis=1, kind="stable")[:, :9]
    assert np.array_equal(idx, order)
    assert np.array_equal(d2, np.take_along_axis(d, order, 1))


# ---------------------------------------------------------------- small dense pieces
def test_so3_exp_log_roundtrip_and_left_jacobian(orc):
    rng = np.random.default_rng(0)
    for _ in range(20):
        w = rng.normal(size=3) * rng.choice([1e-3, 0.1, 1.0])
        R, Jl = orc.so3_exp(w)
        assert np.allclose(R, so3_exp_np(w), atol=1e-14)
        assert np.allclose(orc.so3_log(R), w, atol=1e-9)
        # J_l(w) = d/de Exp(w + e) Exp(w)^-1 ; check J_l w = w and numerical derivative
        assert np.allclose(Jl @ w, w, atol=1e-12)
    R, Jl = orc.so3_exp(np.zeros(3))
    assert np.array_equal(R, np.eye(3)) and np.all(np.isnan(Jl[np.eye(3, dtype=bool)]))  # 0/0 as in SVNICP.cpp:188
    assert np.array_equal(orc.so3_log(np.eye(3)), np.zeros(3))


def test_solve6_inv6(orc):
    rng = np.random.default_rng(1)
    A = rng.normal(size=(6, 6)); A = A @ A.T + 0.1 * np.eye(6); b = rng.normal(size=6)
    assert np.allclose(orc.solve6(A, b), np.linalg.solve(A, b), rtol=1e-11)
    assert np.allclose(orc.inv6(A), np.linalg.inv(A), rtol=1e-10)
    P = np.eye(6)[[3, 0, 5, 1, 2, 4]]  # forces pivoting
    assert np.allclose(orc.solve6(P, b), np.linalg.solve(P, b))


# ---------------------------------------------------------------- golden vectors
@pytest.mark.parametrize("name", golden_cases())
def test_oracle_reproduces_golden(orc, name):
    g = load_golden(name)
    s = oracle_from_golden(orc, g)
    tr = s.enable_trace()
    assert s.stein_align() == int(g["state"])
    n = int(g["iters_run"])
    assert np.array_equal(s.candidates(), g["cand_idx"].astype(np.int64))
    # R0 != I: the golden's query transform went through a BLAS gemm (possibly fused), the oracle's
    # through scalar mul/add: distances agree to the last bits, index sets are identical
    assert np.allclose(s.candidate_dist2(), g["cand_d2"], rtol=1e-12, atol=1e-18)
    # correspondences: the golden transform went through a BLAS bmm, the oracle through scalar
    # code; equal except on (never observed) last-bit near-ties
    assert (tr["corr"][:n] != g["corr"]).mean() <= 1e-4
    assert np.array_equal(tr["mask"][:n][tr["corr"][:n] == g["corr"]], g["mask"][tr["corr"][:n] == g["corr"]])
    assert np.allclose(tr["phi"][:n], g["phi"], rtol=0, atol=TIGHT)
    if g["mode"] == "svn":
        assert np.allclose(tr["H"][:n], g["H"], rtol=1e-11, atol=1e-9)
        assert np.allclose(tr["b"][:n], g["b"], rtol=1e-9, atol=1e-9)
    if g["init"].shape[1] > 1:
        assert np.allclose(tr["h"][:n], g["h"], rtol=1e-10)
    assert np.allclose(s.get_transformation(), g["mean"], atol=TIGHT)
    assert np.allclose(s.get_distribution(), g["var"], atol=TIGHT)
    assert np.allclose(s.get_cov_matrix(), g["cov"], atol=TIGHT)
    assert np.allclose(s.get_particles(), g["particles"], atol=TIGHT)
    assert np.allclose(s.get_particle_weight(), g["weights"], atol=0)
    assert np.allclose(s.get_particle_history(), g["history"], atol=1e-6)
    # rows after an early stop stay zero (break before the history write, SVNICP.cpp:95-107)
    if n < g["cfg"]["iterations"] or g["cfg"]["check_early_stop"]:
        run = s.iterations_run()
        assert np.all(s.get_particle_history()[run - 1 if g["cfg"]["check_early_stop"] and run <= n else run:] == 0)


# ---------------------------------------------------------------- live cross-check against libtorch
@pytest.mark.parametrize("P,full", [(1, False), (5, False), (5, True)])
def test_oracle_vs_torch_restatement_live(orc, pkg, P, full):
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import torch_restatement as tr
    src, tgt = pkg.scans.random_clouds(150, 500, seed=21)
    init = pkg.scans.make_particles(P, seed=21) * 0.3
    o = orc.Solver(init, iterations=5, lr=1.0, max_dist=1.0, knn_count=12, svn_full_grad=full)
    o.add_cloud(src, tgt, init); o.stein_align()
    s = tr.SVNICP(tr.SteinICPParam(iterations=5, lr=1.0, max_dist=1.0, KNN_count=12, SVN_full_grad=full), torch.tensor(init))
    s.add_cloud(torch.tensor(src), torch.tensor(tgt), torch.tensor(init)); s.stein_align()
    assert np.allclose(o.get_transformation(), s.get_transformation().numpy(), atol=TIGHT)
    assert np.allclose(o.get_cov_matrix(), s.get_cov_matrix().numpy(), atol=TIGHT)


def test_oracle_full_correspondence_is_a_k1_search_over_the_whole_target(orc, pkg):
    """orc_set_correspondence_full restates SVGDICP::get_correspondence (SVGDICP.cpp:274-298): with K = 1 the index the
    reference's KNearestNeighborIdx returns is the argmin of the squared distances in target order (knn_cpu.cpp:35-67,
    pinned above).  First iteration, numpy brute force on the same transformed points."""
    src, tgt = pkg.scans.random_clouds(120, 400, seed=31)
    P = 4
    init = pkg.scans.make_particles(P, seed=31) * 0.3
    o = orc.Solver(init, iterations=2, lr=1.0, max_dist=1.0, knn_count=6, svn_full_grad=False)
    o.set_correspondence_full(True)
    o.add_cloud(src, tgt, init)
    tro = o.enable_trace(); o.stein_align()
    for p in range(P):
        R = so3_exp_np(init[3:, p])
        T = (src[:, 0:1] * R[:, 0] + src[:, 1:2] * R[:, 1] + src[:, 2:3] * R[:, 2]) + init[:3, p]     # SVNICP.cpp:62-64, R0 = I, t0 = 0
        d = T[:, None, :] - tgt[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        assert np.array_equal(tro["corr"][0, p], np.argmin(d2, axis=1))
    # the fast routine restricts the same search to the K candidates of the initial pose: where it disagrees, its winner is farther
    o2 = orc.Solver(init, iterations=2, lr=1.0, max_dist=1.0, knn_count=6, svn_full_grad=False)
    o2.add_cloud(src, tgt, init)
    tr2 = o2.enable_trace(); o2.stein_align()
    fast_idx = np.take_along_axis(o2.candidates()[None, :, :].repeat(P, 0), tr2["corr"][0][..., None].astype(np.int64), axis=2)[..., 0]
    assert (fast_idx == tro["corr"][0]).mean() > 0.5


def test_oracle_recovers_planted_transform(orc, pkg):
    off = (0.05, -0.03, 0.02, 0.004, -0.003, 0.006)
    src, tgt = pkg.scans.random_clouds(2000, 6000, seed=4, offset=off)
    init = pkg.scans.make_particles(16, seed=4) * 0.2
    o = orc.Solver(init, iterations=15, lr=1.0, max_dist=1.0, knn_count=20, svn_full_grad=False)
    o.add_cloud(src, tgt, init); o.stein_align()
    m = o.get_transformation()
    assert np.abs(m[:3] - off[:3]).max() < 5e-3 and np.abs(m[3:] - off[3:]).max() < 2e-3
    assert np.all(np.linalg.eigvalsh(o.get_cov_matrix().reshape(6, 6)) > -1e-15)


def test_oracle_thread_count_does_not_change_results(orc, pkg):
    src, tgt = pkg.scans.random_clouds(5000, 3000, seed=8)
    init = pkg.scans.make_particles(3, seed=8) * 0.2
    res = []
    for nt in (1, 4):
        orc.set_threads(nt)
        o = orc.Solver(init, iterations=3, lr=1.0, max_dist=1.0, knn_count=8, svn_full_grad=True)
        o.add_cloud(src, tgt, init); o.stein_align(); res.append(o.get_particles())
    orc.set_threads(0)
    assert np.array_equal(res[0], res[1])
