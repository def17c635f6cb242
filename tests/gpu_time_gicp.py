"""bring-up timing helper (not a pytest file): the generalized-ICP residual against plane and point mode, in ONE process.
  python tests/gpu_time_gicp.py
C3 size (128 particles, 131 072 x 262 144, K = 100, 20 iterations) and the scan-to-map size (30 particles, ~1 100 x 50 000).
After warm-up the three modes alternate; every round gives each mode a NEW svnicp_set_source and svnicp_set_target and two
registrations of them (the second after svnicp_set_particles alone), under a host clock around svnicp_synchronize:
  normal passes          = first registration of new clouds - second of the same clouds: the target's pass in plane mode, the
                           target's and the source's in generalized-ICP mode (point mode's difference is the target layout
                           alone and is printed beside them)
  per-iteration kernels  = svnicp_get_kernel_ms of one more, profiled registration: k_gicp_accumulate + k_plane_finalize
                           against k_plane_accumulate + k_plane_finalize and k_stein_accumulate_w + k_reduce_partials"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g

pkg = g.load_package()
import torch
from svnicp_amd.pipeline import downsample_uniform, crop_pointcloud

N = 8


def run(tag, prm_kw, src, tgt, init):
    sd, td = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    P = init.shape[1]
    solvers = {}
    for mode in ("point", "plane", "gicp"):
        solvers[mode] = pkg.SVNICP(pkg.SteinICPParam(residual=mode, **prm_kw), init)
    dp = C.POINTER(C.c_double)
    initc = np.ascontiguousarray(init)

    def timed(s):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        s.stein_align_async(); s.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def pair_of_registrations(s):
        s.add_cloud(sd, td, init); s.set_initial_mean(np.eye(4)); s.synchronize()     # a new svnicp_set_source and svnicp_set_target
        first = timed(s)
        s._check(s._L.svnicp_set_particles(s.handle, initc.ctypes.data_as(dp), P), "svnicp_set_particles"); s.synchronize()
        second = timed(s)
        return first, second

    for s in solvers.values():
        for _ in range(2):
            pair_of_registrations(s)
    t = {m: [] for m in solvers}
    for _ in range(N):                      # alternating
        for m, s in solvers.items():
            t[m].append(pair_of_registrations(s))
    for m, s in solvers.items():
        a = np.array(t[m])
        d = a[:, 0] - a[:, 1]
        s.set_profile(True)
        s._check(s._L.svnicp_set_particles(s.handle, initc.ctypes.data_as(dp), P), "svnicp_set_particles")
        s.stein_align()
        km = {k: (round(v[0], 3), v[1]) for k, v in s.get_kernel_ms().items()}
        s.set_profile(False)
        I = max(1, s.get_iterations_run())
        per_it = (km["k_stein_accumulate"][0] + km["k_reduce_partials"][0]) / I
        line = (f"{tag} B {src.shape[0]} M {tgt.shape[0]} P {P} {m}: first registration of new clouds {a[:, 0].mean():.3f} ms "
                f"(min {a[:, 0].min():.3f}), second {a[:, 1].mean():.3f} ms (min {a[:, 1].min():.3f}), first - second "
                f"{d.mean():.3f} ms (min {d.min():.3f}, max {d.max():.3f}); accumulate + {'reduce' if m == 'point' else 'finalize'} "
                f"{1e3 * per_it:.1f} us per iteration; kernel classes (ms, launches) {km}; pose {np.round(s.get_transformation(), 5).tolist()}")
        if m == "plane":
            stats, passes = s.get_plane_stats()
            line += f"; accepted pairs per particle {stats[:, 0].min():.0f}..{stats[:, 0].max():.0f}, normal passes {passes}"
        if m == "gicp":
            stats, passes = s.get_gicp_stats()
            valid = (s.get_source_normals() != 0).any(axis=1).mean()
            line += (f"; accepted pairs per particle {stats[:, 0].min():.0f}..{stats[:, 0].max():.0f}, normal passes (target, source) {passes}, "
                     f"source rows with a normal {valid:.4f}")
        print(line, flush=True)


cfg = dict(iterations=20, lr=1.0, max_dist=1.0, KNN_count=100, SVN_full_grad=False)
c3 = pkg.scans.CONFIGS["C3"]
pair = pkg.scans.make_pair(c3["B"], c3["M"])
run("C3", cfg, pair.source, pair.target, pkg.scans.make_particles(c3["P"]))

pair = pkg.scans.make_pair(65536, 50000)
srcc, _ = crop_pointcloud(pair.source, 1.0, 100.0)
small = downsample_uniform(downsample_uniform(srcc, 0.5), 1.5)
run("scan-to-map size", cfg, small, pair.target, pkg.scans.make_particles(30))
