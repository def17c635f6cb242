"""bring-up timing helper (not a pytest file): one scoring of the particles in each of the three forms — the point cost, the
Huber-weighted plane residual, the generalized-ICP residual.
  python tests/gpu_time_particle_score_objective.py [--point-only] [--root DIR]
The two sizes of tests/gpu_time_particle_score.py, each in ONE process state after warm-up: the scan-to-map size (about 1 100
source points, 30 particles, K = 100) and C3 (128 particles x 131 072 x 262 144 points, K = 100).  A point-mode registration,
then supplied normals for both clouds (the forms are the caller's choice), then per form the median of 20 warm blocking calls
with a host clock around each (score kernel, finalize, the copy of the poses, two downloads).  All forms stage the 48-byte
records, so the point form here is gpu_time_particle_score.py's "with normals" figure.
--root DIR loads the package of another checkout (the parent commit's build, for the comparison in the same job);
--point-only times svnicp_score_particles alone, which is all such a checkout has."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINT_ONLY = "--point-only" in sys.argv
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
import __graft_entry__ as g

pkg = g.load_package()
import torch
from svnicp_amd.pipeline import crop_pointcloud, downsample_uniform

N = 20
GATE, DELTA, EPS = 0.3, 0.1, 1e-3
sc = pkg.scans


def run(tag, src, tgt, P, K=100, I=20):
    init = sc.make_particles(P)
    prm = pkg.SteinICPParam(iterations=I, lr=1.0, max_dist=1.0, KNN_count=K, SVN_full_grad=False)
    s = pkg.SVNICP(prm, init, pkg.ParticleWeightOpt())
    s.add_cloud(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), init)
    s.set_initial_mean(np.eye(4))
    s.stein_align()
    n = np.zeros_like(tgt); n[:, 2] = 1.0
    s.set_target_normals(n)
    forms = [("point", lambda: s.score_particles(GATE))]
    if not POINT_ONLY:
        n = np.zeros_like(src); n[:, 1] = np.sqrt(0.5); n[:, 2] = np.sqrt(0.5)
        s.set_source_normals(n)
        forms += [("plane", lambda: s.score_particles(GATE, form="plane", huber_delta=DELTA)),
                  ("gicp", lambda: s.score_particles(GATE, form="gicp", huber_delta=DELTA, gicp_epsilon=EPS))]
    for name, call in forms:
        def timed():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            r = call()
            return 1e3 * (time.perf_counter() - t0), r
        for _ in range(3):
            timed()
        t = []
        for _ in range(N):
            ms, r = timed()
            t.append(ms)
        t = np.array(t)
        print(f"{tag} [{os.path.relpath(ROOT)}]: B {src.shape[0]} M {tgt.shape[0]} P {P} K {K} | form {name}: median {np.median(t):.3f} ms "
              f"(min {t.min():.3f}, max {t.max():.3f}) | inliers {r.inliers.min()}..{r.inliers.max()} accepted {r.plane_inliers.min()}..{r.plane_inliers.max()} "
              f"cost {r.cost.min():.5f}..{r.cost.max():.5f}", flush=True)
    s.close()


pair = sc.make_pair(65536, 50000)
srcc, _ = crop_pointcloud(pair.source, 1.0, 100.0)
src = np.ascontiguousarray(downsample_uniform(downsample_uniform(srcc, 0.5), 1.5))
run("scan-to-map", src, np.ascontiguousarray(pair.target), 30)
c3 = sc.CONFIGS["C3"]
pair = sc.make_pair(c3["B"], c3["M"])
run("C3", pair.source, pair.target, c3["P"])
