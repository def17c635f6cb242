"""Mini-batch Stein ICP (SteinICPParam.use_minibatch / batch_size), the parts that need no GPU: the Python mirror of the
generated index table, the exported symbols, and the chain identity of the oracle that the GPU tests lean on — iteration i
of a mini-batch run is ONE full-batch iteration on the cloud src[idx[i]] started from the particles iteration i-1 left."""
import os
import subprocess

import numpy as np
import pytest

M64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _exact_table(seed, n, I, batch, B):
    base = _splitmix64((seed * 1000003 + n) & M64)
    return np.array([(_splitmix64((base + j) & M64) * B) >> 64 for j in range(I * batch)], np.int64).reshape(I, batch)


@pytest.mark.parametrize("B", [1, 4096, 1113, (1 << 31) - 1])
def test_minibatch_indices_exact_arithmetic(pkg, B):
    t = pkg.minibatch_indices(7, 3, 5, 300, B)
    assert t.shape == (5, 300) and t.dtype == np.int32
    assert t.min() >= 0 and t.max() < B
    assert np.array_equal(t, pkg.minibatch_indices(7, 3, 5, 300, B))
    assert np.array_equal(t.astype(np.int64), _exact_table(7, 3, 5, 300, B))
    assert np.array_equal(pkg.minibatch_indices(2 ** 63 + 11, 2 ** 40, 2, 50, B).astype(np.int64), _exact_table(2 ** 63 + 11, 2 ** 40, 2, 50, B))
    if B > 1:
        other = pkg.minibatch_indices(7, 4, 5, 300, B)
        assert (other == t).mean() < 0.05, "two registrations must draw different tables"
        assert (pkg.minibatch_indices(8, 3, 5, 300, B) == t).mean() < 0.05


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_minibatch_indices_uniform(pkg, seed):
    """A condition, not a tolerance on a measurement: every bin of 10^6 draws over B = 1000 within 6 sigma of n / B."""
    B, n = 1000, 1_000_000
    t = pkg.minibatch_indices(seed, 0, 1000, 1000, B)
    counts = np.bincount(t.ravel(), minlength=B)
    p = 1.0 / B
    sigma = np.sqrt(n * p * (1 - p))
    worst = np.abs(counts - n * p).max() / sigma
    print(f"seed {seed}: worst bin {worst:.2f} sigma")
    assert worst <= 6.0


def test_minibatch_symbols_and_plain_c_header(pkg, tmp_path):
    L = pkg.load_library()
    for name in ("svnicp_set_minibatch", "svnicp_set_minibatch_indices", "svnicp_get_minibatch_indices",
                 "svnicp_get_minibatch_candidates", "svnicp_get_minibatch_rows"):
        assert name in pkg.declared_symbols(), name
        assert hasattr(L, name), name
    assert pkg.abi_version() == 1
    src = tmp_path / "t.c"
    root = os.path.dirname(os.path.dirname(pkg.library_path()))
    src.write_text('#include "svnicp_hip.h"\nint main(void){int (*f)(svnicp_ctx*, int, uint64_t) = svnicp_set_minibatch; '
                   'int (*g)(svnicp_ctx*, int64_t*) = svnicp_get_minibatch_rows; return f == 0 || g == 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-c", str(src), "-o",
                           str(tmp_path / "t.o")])


def test_param_mirror_has_the_fields(pkg):
    p = pkg.SteinICPParam()
    assert p.use_minibatch is False and p.batch_size == 50 and p.minibatch_seed == 0


def _chain(orc, mode, cfg, src, tgt, idx, init, lr=None):
    p = np.array(init, np.float64)
    for i in range(idx.shape[0]):
        c = dict(cfg, iterations=1)
        if lr is not None:
            c["lr"] = lr
        o = orc.Solver(p, mode=mode, **c)
        o.add_cloud(src[idx[i]], tgt, p)
        o.stein_align()
        p = o.get_particles().reshape(6, -1)
    return p


@pytest.mark.parametrize("full", [False, True])
def test_oracle_chain_identity_svn(pkg, orc, full):
    """Chained one-iteration oracle runs against one continuous run, identity table: the yardstick of the GPU tests."""
    P, B, M, K, I = 8, 600, 2500, 16, 10
    src, tgt = pkg.scans.random_clouds(B, M, seed=5)
    init = pkg.scans.make_particles(P, seed=5) * 0.3
    cfg = dict(iterations=I, lr=1.0 if not full else 0.5, max_dist=1.0, check_early_stop=False, convergence_threshold=1e-5,
               knn_count=K, svn_full_grad=full)
    o = orc.Solver(init, **cfg); o.add_cloud(src, tgt, init); o.stein_align()
    idx = np.tile(np.arange(B), (I, 1))
    p = _chain(orc, orc.MODE_SVN, cfg, src, tgt, idx, init)
    err = np.abs(p.ravel() - o.get_particles()).max()
    print(f"SVN full_grad={full}: chained vs continuous {err:.3e}")
    assert err <= 1e-10


def test_oracle_chain_identity_svgd_sgd_one_particle(pkg, orc):
    P, B, M, K, I = 1, 600, 2500, 16, 10
    src, tgt = pkg.scans.random_clouds(B, M, seed=6)
    init = np.zeros((6, 1))
    cfg = dict(iterations=I, lr=1e-3 / B, max_dist=1.0, check_early_stop=False, convergence_threshold=1e-5, knn_count=K,
               svn_full_grad=False, optimizer="SGD")
    o = orc.Solver(init, mode=orc.MODE_SVGD, **cfg); o.add_cloud(src, tgt, init); o.stein_align()
    idx = np.tile(np.arange(B), (I, 1))
    p = _chain(orc, orc.MODE_SVGD, cfg, src, tgt, idx, init)
    assert np.abs(o.get_particles()).max() > 0
    assert np.array_equal(p.ravel(), o.get_particles())
