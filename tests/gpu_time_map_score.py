"""bring-up timing helper (not a pytest file): svnicp_map_score_poses at the scan-to-map size and at a raw scan's size.
  python tests/gpu_time_map_score.py
Map: the drive of tests/map_normals_cases.py (voxel 0.5 m, 20 points per voxel), fed the 0.25 m samplings of its scans until it
holds about 50 000 points.  Rows: scan 4's solver cloud cut to 1 100 rows, and a cropped raw scan of 131 072 points.  Poses: the
729-node grid of the tests (+-2 m / 0.5 m in x and y, +-10 deg / 2.5 deg in yaw) around a centre displaced from the true pose,
the same extents at half the step (17^3 = 4 913 nodes), 32 768 random corrections inside them, and the true pose alone.
Rows and poses live in device memory and outCx4 is NULL: nothing crosses PCIe inside a timed call.  One process; 5 warm-up
calls, then 30 timed ones per configuration; a pair of events on an otherwise idle stream brackets the blocking call (the call
runs on the map's own stream and ends in its synchronise, so the figure includes two launches and that synchronise), and the
host clock is printed next to it.  Median and range.  Output: profiles/map_score_timing.log."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g

pkg = g.load_package()
import torch
import map_normals_cases as mn
import map_score_cases as ms

pl, sc = pkg.pipeline, pkg.scans
WARM, REPS, GATE = 5, 30, 0.5
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


dm = pl.DeviceVoxelHashMap(mn.DRIVE_VOXEL, 100.0, mn.DRIVE_MAX_POINTS, device=0)
k, M = 0, 0
while M < 50000 and k < 40:
    to_map, _, T = mn._drive_scan(k)
    dm.add_pointcloud(to_map.astype(np.float32), T)
    M = dm.get_map()[1]
    k += 1
say(f"map: {k} scans, {len(dm)} voxels, {M} points ({M / len(dm):.2f} per voxel), voxel {mn.DRIVE_VOXEL} m, gate {GATE} m")

T4 = ms.drive_scan(4)[1]
small = np.ascontiguousarray(ms.drive_scan(4)[0][:1100])
raw = sc.lidar_scan(sc.make_scene(), T4[:3, :3], T4[:3, 3], 131072, stream=304).astype(np.float32)
big = np.ascontiguousarray(pl.crop_pointcloud(raw, 1.0, 80.0)[0], np.float32)
centre = T4 @ np.linalg.inv(pl.correction_to_pose(ms.JUMP))
rng = np.random.default_rng(0)
fine, _ = pl.correction_grid(ms.GRID_EXTENT, tuple(0.5 * v for v in ms.GRID_STEP))
pose_sets = {1: pl.pose_rows(T4[None]), 729: ms.grid_search()[3], 4913: pl.correction_poses(centre, fine),
             32768: pl.correction_poses(centre, rng.uniform(-1, 1, size=(32768, 6)) * np.array(ms.GRID_EXTENT)),
             128: pl.correction_poses(centre, rng.uniform(-1, 1, size=(128, 6)) * np.array(ms.GRID_EXTENT))}
assert fine.shape[0] == 4913


def measure(rows, Cn):
    d_rows = torch.from_numpy(rows).to("cuda:0").contiguous()
    d_poses = torch.from_numpy(np.ascontiguousarray(pose_sets[Cn])).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    first = dm.score_poses_device(d_rows.data_ptr(), rows.shape[0], d_poses, GATE)          # also checks the call, once
    ev, host = [], []
    for r in range(WARM + REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        rc = dm._L.svnicp_map_score_poses(dm._h, C.c_void_p(d_rows.data_ptr()), rows.shape[0], 1, C.c_void_p(d_poses.data_ptr()), Cn, 1,
                                          GATE, None)
        e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        assert rc == 0
        if r >= WARM:
            ev.append(e0.elapsed_time(e1)); host.append(1e3 * (t1 - t0))
    best = int(np.lexsort((np.arange(Cn), first[:, 3]))[0])
    pairs = rows.shape[0] * Cn
    say(f"rows {rows.shape[0]:6d} x poses {Cn:5d}: events median {np.median(ev):.3f} ms (min {min(ev):.3f}, max {max(ev):.3f}) | host clock "
        f"median {np.median(host):.3f} ms (min {min(host):.3f}, max {max(host):.3f}) | {pairs / np.median(ev) * 1e-6:.1f} M (pose, row) pairs per ms"
        f" | best pose {best}: located {int(first[best, 0])}, inliers {int(first[best, 1])}, cost {first[best, 3]:.4f}")


for Cn in (1, 729, 4913, 32768):
    measure(small, Cn)
for Cn in (1, 128):
    measure(big, Cn)
dm.close()

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "map_score_timing.log"), "w") as f:
    f.write("\n".join(lines) + "\n")
