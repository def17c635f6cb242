"""bring-up timing helper (not a pytest file): the coarse-to-fine pose search (svnicp_map_search_poses) against the flat grids it
replaces, at the scan-to-map size.
  python tests/gpu_time_map_search.py [output log]
Map and rows as tests/gpu_time_map_score.py: the drive of tests/map_normals_cases.py fed until it holds about 50 000 points, scan
4's solver cloud cut to 1 100 rows, in device memory.  The grid is the tests' (+-2 m / 0.5 m in x and y, +-10 deg / 2.5 deg in
yaw) around a centre displaced from the true pose by (4, -2, 0, 0, 0, 5) thirds of a step.  Configurations:
  (a) today's path for 729 nodes: correction_poses on the host + score_poses_device + seed_from_scores
  (b) search_poses_device, levels=1, the same grid
  (c) levels=2, keep=8 (945 nodes)
  (d) levels=1 at a third of the step over the same window (25^3 = 15 625 nodes): the flat grid (c) replaces
  (e) levels=3, keep=8 (1 161 nodes)
One process; 5 warm-up rounds, then 30 timed ones, every round running (a)..(e) in turn.  A pair of events on an otherwise idle
stream brackets each blocking call, and the host clock is printed next to it: for (a) the host clock is the figure that counts,
its poses are made and its records sorted on the host.  Median and range.  Output: profiles/map_search_timing.log."""
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
import map_search_cases as sc

pl = pkg.pipeline
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

rows = np.ascontiguousarray(ms.drive_scan(4)[0][:1100])
d_rows = torch.from_numpy(rows).to("cuda:0").contiguous()
torch.cuda.synchronize()
ptr, n = d_rows.data_ptr(), rows.shape[0]
centre = sc.centre(sc.TRUTHS[0])
nodes, _ = pl.correction_grid(ms.GRID_EXTENT, ms.GRID_STEP)
third = tuple(v / 3.0 for v in ms.GRID_STEP)


def flat_today():
    poses = pl.correction_poses(centre, nodes)
    scores = dm.score_poses_device(ptr, n, poses, GATE)
    best, _, order = pl.seed_from_scores(scores, nodes, 8)
    return {"best_correction": best, "best_record": scores[order[0]], "nodes_scored": nodes.shape[0]}


def search(step, levels):
    return lambda: dm.search_poses_device(ptr, n, centre, ms.GRID_EXTENT, step, levels, 8, GATE)


configs = [("(a) host poses + score + host sort, 729 nodes", flat_today), ("(b) search levels=1, 729 nodes", search(ms.GRID_STEP, 1)),
           ("(c) search levels=2 keep=8", search(ms.GRID_STEP, 2)), ("(d) search levels=1 at step/3", search(third, 1)),
           ("(e) search levels=3 keep=8", search(ms.GRID_STEP, 3))]
ev = {name: [] for name, _ in configs}
host = {name: [] for name, _ in configs}
last = {}
for r in range(WARM + REPS):
    for name, fn in configs:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        last[name] = fn()
        e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        if r >= WARM:
            ev[name].append(e0.elapsed_time(e1)); host[name].append(1e3 * (t1 - t0))
truth = sc.truth_correction(sc.TRUTHS[0])
for name, _ in configs:
    e, h, res = ev[name], host[name], last[name]
    off = res["best_correction"] - truth
    say(f"{name:48s}: events median {np.median(e):.3f} ms (min {min(e):.3f}, max {max(e):.3f}) | host clock median {np.median(h):.3f} ms "
        f"(min {min(h):.3f}, max {max(h):.3f}) | nodes {res['nodes_scored']:6d} | best cost {res['best_record'][3]:.5f}, "
        f"{np.hypot(off[0], off[1]):.3f} m {abs(off[5]):.4f} rad from the truth")
dm.close()

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "map_search_timing.log")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
