"""bring-up timing helper (not a pytest file): one scoring of the particles beside one iteration of the same registration.
  python tests/gpu_time_particle_score.py
Two sizes, each in ONE process state after warm-up:
  scan-to-map  make_pair(65536, 50000)'s target, the source cropped and sampled as the pipeline does (about 1 100 points),
               30 particles, K = 100, 20 iterations
  C3           128 particles x 131 072 source x 262 144 target points, K = 100, 20 iterations (bench.py's headline clouds)
Per size: one iteration of the registration by hipEvents (svnicp_get_kernel_ms with every class bracketed: search +
accumulate + reduce + update, divided by the iterations run), the median of 20 warm svnicp_score_particles calls (a host
clock around the blocking call: score kernel, finalize, the copy of the poses, two downloads), without normals and with
supplied ones (the tile then holds the 48-byte records), and the whole registration with and without weighting
(svnicp_get_gpu_ms()[2] does not cover what svnicp_finish enqueues, so this one is a host clock around the blocking call)."""
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

    def align():
        s.add_cloud(src_d, tgt_d, init); s.set_initial_mean(np.eye(4))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        s.stein_align()
        return 1e3 * (time.perf_counter() - t0)

    s.set_profile(True)
    for _ in range(3):
        align()
    per_iter = sum(ms for k, (ms, n) in s.get_kernel_ms().items() if k not in ("stage_a_knn", "k_build_table")) / I
    s.set_profile(False)
    whole = {}
    for name in ("uniform", "softmin"):
        s.set_particle_weighting(name, 0.3, 1e-3)
        for _ in range(3):
            align()
        whole[name] = np.median([align() for _ in range(N)])
    s.set_particle_weighting("uniform")
    align()

    def timed():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = s.score_particles(0.3)
        return 1e3 * (time.perf_counter() - t0), r

    for normals in (False, True):
        if normals:
            n = np.zeros_like(tgt); n[:, 2] = 1.0
            s.set_target_normals(n)
        for _ in range(3):
            timed()
        t = []
        for _ in range(N):
            ms, r = timed()
            t.append(ms)
        t = np.array(t)
        print(f"{tag}: B {src.shape[0]} M {tgt.shape[0]} P {P} K {K} | one iteration of the registration {per_iter:.3f} ms | "
              f"svnicp_score_particles{' with normals' if normals else ''} median {np.median(t):.3f} ms (min {t.min():.3f}, max {t.max():.3f}) "
              f"= {1e-6 * src.shape[0] * P * K / np.median(t):.1f} G pair distances / s | registration, host clock: uniform "
              f"{whole['uniform']:.3f} ms, weighted {whole['softmin']:.3f} ms | inliers {r.inliers.min()}..{r.inliers.max()} cost {r.cost.min():.5f}..{r.cost.max():.5f}",
              flush=True)
    s.close()


pair = sc.make_pair(65536, 50000)
srcc, _ = crop_pointcloud(pair.source, 1.0, 100.0)
src = np.ascontiguousarray(downsample_uniform(downsample_uniform(srcc, 0.5), 1.5))
run("scan-to-map", src, np.ascontiguousarray(pair.target), 30)
c3 = sc.CONFIGS["C3"]
pair = sc.make_pair(c3["B"], c3["M"])
run("C3", pair.source, pair.target, c3["P"])
