"""bring-up timing helper (not a pytest file): svnicp_evaluate + svnicp_eval_information_gicp next to svnicp_evaluate +
svnicp_eval_information (plane form), after the pattern of tests/gpu_time_information.py.
  python tests/gpu_time_information_gicp.py scan-to-map|C3
One size per process (a job gives each its own time limit):
  scan-to-map  make_pair(65536, 50000)'s target, the source cropped and sampled as the pipeline does (about 1 100 points),
               30 particles, K = 100, 20 iterations
  C3           128 particles x 131 072 source x 262 144 target points, K = 100, 20 iterations (bench.py's headline clouds)
After warm-up, 20 rounds that ALTERNATE the three measurements (a host clock around the blocking calls), supplied normals
(0, 0, 1) on every row of both clouds (zero-free: every inlier is a plane inlier and has a source normal, so both forms sum the
same rows), gate 0.3 m, Huber delta 0.1, epsilon 1e-3:
  evaluate               transform, K = 1 search, pair kernel, finalize, one synchronise
  evaluate + plane form  ... then k_information_pairs<plane>, k_information_finalize, one copy, one synchronise, the 6x6 solve
  evaluate + GICP form   ... the same with k_information_pairs<gicp>: one more coalesced 24-byte read per row, the 3x3 inverse
and, inside the same rounds, the information call alone.  Printed: median, min and max of each, the medians' difference to
evaluate alone, and the ratio of the two information calls' medians."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g

pkg = g.load_package()
import torch
from svnicp_amd.pipeline import crop_pointcloud, downsample_uniform

N = 20
sc = pkg.scans


def run(tag, src, tgt, P, K=100, I=20):
    init = sc.make_particles(P)
    prm = pkg.SteinICPParam(iterations=I, lr=1.0, max_dist=1.0, KNN_count=K, SVN_full_grad=False)
    s = pkg.SVNICP(prm, init, pkg.ParticleWeightOpt())
    src_d, tgt_d = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    for _ in range(2):
        s.add_cloud(src_d, tgt_d, init); s.set_initial_mean(np.eye(4)); s.stein_align()
    n = np.zeros_like(tgt); n[:, 2] = 1.0
    s.set_target_normals(n)
    n = np.zeros_like(src); n[:, 2] = 1.0
    s.set_source_normals(n)
    T = np.eye(4)

    def timed(form):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        s.evaluate(0.3, T)
        t1 = time.perf_counter()
        info = s.information(form, 0.1, gicp_epsilon=1e-3) if form else None
        t2 = time.perf_counter()
        return 1e3 * (t2 - t0), 1e3 * (t2 - t1), info

    kinds = (None, "plane", "gicp")
    for k in kinds * 3:
        timed(k)
    both = {k: [] for k in kinds}
    alone = {k: [] for k in kinds}
    last = {}
    for _ in range(N):
        for k in kinds:
            a, b, last[k] = timed(k)
            both[k].append(a); alone[k].append(b)
    base = np.median(both[None])
    for k in kinds:
        t, u = np.array(both[k]), np.array(alone[k])
        name = "evaluate" if k is None else f"evaluate + information({k})"
        extra = "" if k is None else (f" | the information call alone median {np.median(u):.3f} ms (min {u.min():.3f}, max {u.max():.3f}) | "
                                      f"medians' difference {np.median(t) - base:+.3f} ms")
        print(f"{tag}: B {src.shape[0]} M {tgt.shape[0]} | {name} median {np.median(t):.3f} ms (min {t.min():.3f}, max {t.max():.3f}){extra}", flush=True)
    print(f"{tag}: information(gicp) alone / information(plane) alone, medians: {np.median(alone['gicp']) / np.median(alone['plane']):.3f}", flush=True)
    for k in ("plane", "gicp"):
        print(f"{tag}: {k} pairs {last[k].pairs} rank {last[k].rank} eigval {last[k].eigval.tolist()}", flush=True)
    s.close()


which = sys.argv[1] if len(sys.argv) > 1 else "scan-to-map"
if which == "scan-to-map":
    pair = sc.make_pair(65536, 50000)
    srcc, _ = crop_pointcloud(pair.source, 1.0, 100.0)
    src = np.ascontiguousarray(downsample_uniform(downsample_uniform(srcc, 0.5), 1.5))
    run("scan-to-map", src, np.ascontiguousarray(pair.target), 30)
elif which == "C3":
    c3 = sc.CONFIGS["C3"]
    pair = sc.make_pair(c3["B"], c3["M"])
    run("C3", pair.source, pair.target, c3["P"])
else:
    sys.exit(f"unknown size {which!r}: scan-to-map or C3")
