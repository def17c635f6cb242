"""bring-up timing helper (not a pytest file): mini-batch registrations against full batch, in ONE process.
  python tests/gpu_time_minibatch.py            C3 shapes and the scan-to-map size, every variant, accuracy over seeds
  python tests/gpu_time_minibatch.py --full-only  only the full-batch time of both sizes (A/B of two library builds:
                                                  SVNICP_TEST_LIB names the library, the caller alternates the processes)
Every shape is warmed up, the variants alternate, >= 20 registrations each; wall time around a synchronise, the GPU span
(get_gpu_ms) and the kernel classes (get_kernel_ms, one extra profiled registration)."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
if os.environ.get("SVNICP_TEST_LIB"):   # A/B builds of the library (bring-up only)
    pkg.binding._LIB_PATH = os.path.abspath(os.environ["SVNICP_TEST_LIB"])
import torch
from svnicp_amd.pipeline import downsample_uniform, crop_pointcloud

FULL_ONLY = "--full-only" in sys.argv
N = 20


def so3_exp(w):
    a = np.linalg.norm(w)
    if a < 1e-12:
        return np.eye(3)
    k = w / a
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(a) * np.eye(3) + (1 - np.cos(a)) * np.outer(k, k) + np.sin(a) * Kx


def pose_distance(a, b):
    R = so3_exp(a[3:]).T @ so3_exp(b[3:])
    return float(np.linalg.norm(a[:3] - b[:3])), float(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))


def run(tag, prm_kw, src, tgt, init, batches, seeds=5):
    B = src.shape[0]
    sd, td = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    solvers = {}
    for b in batches:
        s = pkg.SVNICP(pkg.SteinICPParam(**prm_kw), init)
        if b and not FULL_ONLY:
            s.set_minibatch(b, 1)
        solvers[b] = s

    def step(s):
        s.add_cloud(sd, td, init); s.set_initial_mean(np.eye(4)); s.stein_align(); return s.get_transformation()

    for s in solvers.values():
        for _ in range(3):
            step(s)
    wall = {b: 0.0 for b in batches}
    span = {b: [] for b in batches}
    for _ in range(N):                      # alternating
        for b, s in solvers.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            step(s)
            torch.cuda.synchronize(); wall[b] += time.perf_counter() - t0
            span[b].append(s.get_gpu_ms())
    full_mean = None
    for b, s in solvers.items():
        sp = np.array(span[b])
        s.set_profile(True); mean = step(s); km = {k: round(v[0], 3) for k, v in s.get_kernel_ms().items()}; s.set_profile(False)
        line = f"{tag} B {B} M {tgt.shape[0]} batch {b or 'full'}: {1e3 * wall[b] / N:.3f} ms wall per registration; GPU span stage A + table {sp[:, 0].mean():.3f} ms, iterations {sp[:, 1].mean():.3f} ms (min total {sp[:, 2].min():.3f}, max {sp[:, 2].max():.3f}); kernel classes (ms) {km}; iterations run {s.get_iterations_run()}"
        if b and not FULL_ONLY:
            U, nq = s.get_minibatch_rows()
            d = []
            for seed in range(seeds):
                s.set_minibatch(b, 100 + seed)
                d.append(pose_distance(step(s), full_mean))
            d = np.array(d)
            line += f"; U {U} n_q {nq}; mean pose vs full batch over {seeds} seeds: translation {d[:, 0].mean():.4f} m (max {d[:, 0].max():.4f}), rotation {d[:, 1].mean():.5f} rad (max {d[:, 1].max():.5f})"
        elif not b:
            full_mean = mean
        print(line, flush=True)


# C3: 128 particles, 131 072 x 262 144, K = 100, 20 iterations
pair = pkg.scans.make_pair(131072, 262144); init = pkg.scans.make_particles(128)
c3 = dict(iterations=20, lr=1.0, max_dist=1.0, KNN_count=100, SVN_full_grad=False)
run("C3", c3, pair.source, pair.target, init, [0] if FULL_ONLY else [0, 16384, 4096, 1024])

# the scan-to-map size with the reference's shipped solver settings (tests/gpu_time_small.py, SHIPPED)
pair = pkg.scans.make_pair(65536, 50000); init = pkg.scans.make_particles(10)
srcc, _ = crop_pointcloud(pair.source, 1.0, 100.0)
src_ds = downsample_uniform(downsample_uniform(srcc, 0.5), 1.5)
shipped = dict(iterations=100, lr=1.0, max_dist=3.0, KNN_count=100, SVN_full_grad=False, check_early_stop=True, convergence_threshold=5e-4)
run("scan-to-map (shipped settings)", shipped, src_ds, pair.target, init, [0] if FULL_ONLY else [0, 1000, 200])
