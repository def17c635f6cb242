"""bring-up timing helper (not a pytest file): what the Gaussian pose prior costs a registration.
  python tests/gpu_time_pose_prior.py
Scan-to-map size: 1 113 source points (make_pair(65536, 50000)'s source after the crop and the two samplings at voxel 1.0)
against 50 000 target points, K = 100, 20 iterations, no early stop, P = 1, 30 and 128.  In ONE process, after warm-up,
alternating rounds of three contexts per particle count:
  (a) no prior, the default plan            (P = 1: the fused one-particle iteration; P = 30, 128: the small chain)
  (b) no prior, the plan a prior runs under (options single=split / chain=general)
  (c) the prior on                          (Lambda = diag(400, 400, 400, 1e4, 1e4, 1e4), mean 0)
(c) - (b) is the prior's own launch per iteration; (b) - (a) is what losing the fused iteration / the small chain costs."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g

pkg = g.load_package()
import torch
from svnicp_amd.pipeline import crop_pointcloud, downsample_uniform

ROUNDS, ITERS = 30, 20
pair = pkg.scans.make_pair(65536, 50000)
srcc, _ = crop_pointcloud(pair.source, 1.0, 100.0)
src_h = np.ascontiguousarray(downsample_uniform(downsample_uniform(srcc, 0.5), 1.5))
src, tgt = torch.from_numpy(src_h).cuda(), torch.from_numpy(pair.target).cuda()
LAM = np.diag([400.0, 400.0, 400.0, 1e4, 1e4, 1e4])
print(f"source {src_h.shape[0]} points, target {pair.target.shape[0]} points, K 100, {ITERS} iterations, {ROUNDS} alternating rounds", flush=True)

for P in (1, 30, 128):
    init = pkg.scans.make_particles(P)
    prm = pkg.SteinICPParam(iterations=ITERS, lr=1.0, max_dist=1.0, KNN_count=100, SVN_full_grad=False)
    ctx = {}
    for tag in "abc":
        s = pkg.SVNICP(prm, init)
        if tag != "a":
            s.set_option("single", "split"); s.set_option("chain", "general")
        if tag == "c":
            s.set_pose_prior(np.zeros(6), LAM)
        ctx[tag] = s

    def timed(s):
        s.add_cloud(src, tgt, init); s.set_initial_mean(np.eye(4)); s.synchronize()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        s.stein_align_async(); s.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for _ in range(5):
        for tag in "abc":
            timed(ctx[tag])
    t = {tag: [] for tag in "abc"}
    for _ in range(ROUNDS):                  # alternating
        for tag in "abc":
            t[tag].append(timed(ctx[tag]))
    m = {tag: float(np.median(v)) for tag, v in t.items()}
    sp = {tag: (float(np.min(v)), float(np.max(v))) for tag, v in t.items()}
    print(f"P {P}: per registration, median of {ROUNDS} (min .. max) ms:  "
          + "  ".join(f"({tag}) {m[tag]:.3f} ({sp[tag][0]:.3f} .. {sp[tag][1]:.3f})" for tag in "abc"), flush=True)
    print(f"P {P}: prior's launch (c) - (b) = {1e3 * (m['c'] - m['b']):.1f} us per registration, {1e3 * (m['c'] - m['b']) / ITERS:.2f} us per iteration;  "
          f"plan (b) - (a) = {1e3 * (m['b'] - m['a']):.1f} us per registration, {1e3 * (m['b'] - m['a']) / ITERS:.2f} us per iteration;  "
          f"prior on against the default (c) - (a) = {1e3 * (m['c'] - m['a']):.1f} us ({100 * (m['c'] / m['a'] - 1):.1f} %)", flush=True)
    for s in ctx.values():
        s.close()
