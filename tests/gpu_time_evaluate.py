"""bring-up timing helper (not a pytest file): svnicp_evaluate beside the registration's own stage A.
  python tests/gpu_time_evaluate.py
Two sizes, each in ONE process state after warm-up:
  scan-to-map  make_pair(65536, 50000)'s target, the source cropped and sampled as the pipeline does (about 1 100 points),
               30 particles, K = 100, 20 iterations
  C3           128 particles x 131 072 source x 262 144 target points, K = 100, 20 iterations (bench.py's headline clouds)
Per size: the registration's stage A by hipEvents (svnicp_get_gpu_ms()[0]: K-neighbour search + candidate table) and the
median of 20 warm svnicp_evaluate calls (a host clock around the blocking call: transform, K = 1 search, pair kernel,
finalize, one synchronise), without normals and with supplied ones (zero rows: the gather reads the 48-byte records)."""
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
    stage_a = []
    for _ in range(4):
        s.add_cloud(src_d, tgt_d, init); s.set_initial_mean(np.eye(4)); s.stein_align()
        stage_a.append(s.get_gpu_ms()[0])
    T = np.eye(4)

    def timed():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        e = s.evaluate(0.3, T)
        return 1e3 * (time.perf_counter() - t0), e

    for normals in (False, True):
        if normals:
            n = np.zeros_like(tgt); n[:, 2] = 1.0
            s.set_target_normals(n)
        for _ in range(3):
            timed()
        t = []
        for _ in range(N):
            ms, e = timed()
            t.append(ms)
        t = np.array(t)
        print(f"{tag}: B {src.shape[0]} M {tgt.shape[0]} P {P} K {K} | stage A of the registration {np.median(stage_a[1:]):.3f} ms | "
              f"svnicp_evaluate{' with normals' if normals else ''} median {np.median(t):.3f} ms (min {t.min():.3f}, max {t.max():.3f}) | "
              f"fitness {e.fitness:.4f} inlier rmse {e.inlier_rmse:.4f} plane rmse {e.plane_rmse:.4f}", flush=True)
    s.close()


pair = sc.make_pair(65536, 50000)
srcc, _ = crop_pointcloud(pair.source, 1.0, 100.0)
src = np.ascontiguousarray(downsample_uniform(downsample_uniform(srcc, 0.5), 1.5))
run("scan-to-map", src, np.ascontiguousarray(pair.target), 30)
c3 = sc.CONFIGS["C3"]
pair = sc.make_pair(c3["B"], c3["M"])
run("C3", pair.source, pair.target, c3["P"])
