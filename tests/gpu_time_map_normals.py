"""bring-up timing helper (not a pytest file): normals from the voxel map's own cells against the solver's normal pass.
  python tests/gpu_time_map_normals.py
Scan-to-map size: make_pair(65536, 50000)'s target in a device map (voxel 1.0, 20 points per voxel: the cap keeps 18 574 of
the 50 000 points — a map of 50 000 points needs scans from several places and is still to be timed), 1 100 source points, 30 particles, K = 100, 20 iterations.  In ONE process, after warm-up, alternating:
  (a) svnicp_map_query_normals on the last whole-map query — a host clock around the call, which ends in its own synchronise
  (b) the solver's estimated-normals pass on the same target, the way tests/gpu_time_plane.py times it: the first plane-mode
      registration against a new svnicp_set_target minus the second against the same target
Then the per-scan wall time of the Python pipeline (device map + device pre-processing, 12 scans of 65 536 points, voxel 1.0)
in point mode, in plane mode with the solver's pass, and in plane mode with the map's normals."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g

pkg = g.load_package()
import torch
from svnicp_amd.pipeline import (DeviceVoxelHashMap, PipelineConfig, RegistrationPipeline, crop_pointcloud, downsample_uniform)

N = 12
sc = pkg.scans

pair = sc.make_pair(65536, 50000)
srcc, _ = crop_pointcloud(pair.source, 1.0, 100.0)
src = np.ascontiguousarray(downsample_uniform(downsample_uniform(srcc, 0.5), 1.5))
dm = DeviceVoxelHashMap(1.0, 1e9, 20, device=0)
dm.add_pointcloud(pair.target.astype(np.float32), np.eye(4))
ptr, M = dm.get_map()
init = sc.make_particles(30)
initc = np.ascontiguousarray(init)
dp = C.POINTER(C.c_double)
print(f"map: {len(dm)} voxels, {M} points ({M / len(dm):.2f} per voxel); source {src.shape[0]} points", flush=True)

for kn in (8, 16):
    prm = pkg.SteinICPParam(iterations=20, lr=1.0, max_dist=1.0, KNN_count=100, SVN_full_grad=False, residual="plane", normal_k=kn)
    s = pkg.SVNICP(prm, init)

    def timed():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        s.stein_align_async(); s.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def solver_pass():
        s.add_cloud_device_target(src, ptr, M, init); s.set_initial_mean(np.eye(4)); s.synchronize()      # a new svnicp_set_target
        first = timed()
        s._check(s._L.svnicp_set_particles(s.handle, initc.ctypes.data_as(dp), 30), "svnicp_set_particles"); s.synchronize()
        return first - timed()

    def map_pass():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        _, w = dm.get_map_normals(kn)
        return 1e3 * (time.perf_counter() - t0), w

    for _ in range(3):
        solver_pass(); map_pass()
    a, b = [], []
    for _ in range(N):                       # alternating
        t, with_normal = map_pass()
        a.append(t)
        b.append(solver_pass())
    a, b = np.array(a), np.array(b)
    passes = s.get_plane_stats(with_sums=False)[1]
    print(f"normal_k {kn}: (a) svnicp_map_query_normals {a.mean():.3f} ms (min {a.min():.3f}, max {a.max():.3f}), {with_normal} of {M} rows "
          f"with a normal | (b) solver's normal pass {b.mean():.3f} ms (min {b.min():.3f}, max {b.max():.3f}), {passes} passes run "
          f"| (b) / (a) = {b.mean() / a.mean():.1f}", flush=True)
    # the registration itself with the map's normals, for scale
    s.add_cloud_device_target(src, ptr, M, init); s.set_target_normals_device(dm.get_map_normals(kn)[0], M)
    s.set_initial_mean(np.eye(4)); s.synchronize()
    r = [timed()]
    for _ in range(N):
        s._check(s._L.svnicp_set_particles(s.handle, initc.ctypes.data_as(dp), 30), "svnicp_set_particles"); s.synchronize()
        r.append(timed())
    print(f"normal_k {kn}: plane registration with supplied normals {np.mean(r[1:]):.3f} ms (min {np.min(r[1:]):.3f})", flush=True)
    s.close()

# ---- the pipeline, per scan ------------------------------------------------------------------------------------------
scene = sc.make_scene()
scans = []
for k in range(12):
    t = np.array([0.0, 0.0, 0.05 * k]); R = sc.rot_zyx(0.0, 0.0, np.radians(0.3 * k))
    scans.append(sc.lidar_scan(scene, R, t, 65536, stream=1300 + k).astype(np.float32))
for tag, residual, map_normals in (("point mode", "point", False), ("plane, solver's pass", "plane", False),
                                   ("plane, map normals", "plane", True)):
    times = []
    for rep in range(2):                     # the first drive warms every shape up
        cfg = PipelineConfig(min_range=1.0, max_range=80.0, voxel_size=1.0, map_voxel_size=1.0, map_voxel_max_points=20,
                             map_range=100.0, particle_count=30, gpu_map=True, gpu_prep=True, map_normals=map_normals,
                             solver=pkg.SteinICPParam(iterations=20, lr=1.0, max_dist=1.0, KNN_count=100, SVN_full_grad=False,
                                                      residual=residual, normal_k=16))
        pipe = RegistrationPipeline(cfg, device=0)
        times = []
        for k, pts in enumerate(scans):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            res = pipe.process_scan(pts, stamp=0.1 * k)
            torch.cuda.synchronize()
            if k:
                times.append(1e3 * (time.perf_counter() - t0))
    passes = pipe._solver.get_plane_stats(with_sums=False)[1]
    z = res.pose[2, 3]
    print(f"pipeline, {tag}: {np.mean(times):.3f} ms per registered scan (min {np.min(times):.3f}, max {np.max(times):.3f}) over "
          f"{len(times)} scans, {len(pipe.map)} voxels at the end, normal passes {passes}, last z {z:.4f} (true {0.05 * 11:.2f}), "
          f"with_normal {res.with_normal}", flush=True)
