"""bring-up timing helper (not a pytest file): svnicp_particle_modes on a finished registration.
  python tests/gpu_time_modes.py
P = 16, 128, 512 and 1030 particles on one small registration each (make_pair(2048, 4096), K = 16, 3 iterations: the call
reads the particles alone, the clouds do not matter), all in ONE process after warm-up.  Per P, the median of 30 warm calls by a
host clock around the blocking call (synchronise, one kernel, one copy of the result block and the labels) at three links:
  wide    one mode of P
  prior   links the size of the particle spread: a handful of modes
  zero    every particle its own mode (the ranking's worst case)
and a chain of P shuffled particles through the caller-supplied form (the labelling's worst case; one more upload)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as g

pkg = g.load_package()
import torch
import particle_modes_cases as pc

N = 30
sc = pkg.scans
pair = sc.make_pair(2048, 4096)


def timed(f):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = f()
    return 1e3 * (time.perf_counter() - t0), r


def median(f):
    for _ in range(3):
        f()
    t = np.array([timed(f)[0] for _ in range(N)])
    return np.median(t), t.min(), t.max()


for P in (16, 128, 512, 1030):
    init = sc.make_particles(P)
    s = pkg.SVNICP(pkg.SteinICPParam(iterations=3, lr=1.0, max_dist=1.0, KNN_count=16, SVN_full_grad=False), init, pkg.ParticleWeightOpt())
    s.add_cloud(pair.source, pair.target, init)
    s.stein_align()
    out = []
    for name, link in (("wide", (10.0, 10.0)), ("prior", (0.1, 0.004)), ("zero", (0.0, 0.0))):
        med, lo, hi = median(lambda: s.particle_modes(link[0], link[1], 32))
        out.append(f"{name} links: {s.particle_modes(link[0], link[1], 32).n_modes} modes, median {med:.3f} ms (min {lo:.3f}, max {hi:.3f})")
    x = pc.chain(P)
    med, lo, hi = median(lambda: s.particle_modes(pc.LINK_T, pc.LINK_R, 32, particles=x))
    out.append(f"shuffled chain (caller's set): median {med:.3f} ms (min {lo:.3f}, max {hi:.3f})")
    print(f"P {P}: " + " | ".join(out), flush=True)
    s.close()
