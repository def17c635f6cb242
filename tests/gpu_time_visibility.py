"""bring-up timing helper (not a pytest file): svnicp_map_clear_seen_through beside the map's own insert and query.
Two maps: (a) the OS1-64 moving-box drive of tests/map_visibility_cases.py (7 scans inserted, the 8th clears), (b)
gpu_time_map.py's configuration (20 scans of 131 072 points, voxel 0.5 m, 20 points per voxel; sensor HDL-64E).  One process;
the clouds live in device memory (nothing is uploaded inside a timed call); warm-up, then 12 rounds that alternate clear /
insert / query; host clock around calls that end in a synchronise.  A repeated clear removes nothing further but tests the
same points against the same image; a repeated insert finds its voxels full.  Output: profiles/visibility_timing.log."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g
pkg = g.load_package()
import torch
import map_visibility_cases as mv
pl, sc = pkg.pipeline, pkg.scans
ROUNDS, WARM = 12, 3
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    return t


def measure(tag, m, sensor, T, scan, cloud, query_r, window=(1, 1)):
    d_scan, d_cloud = dev(scan), dev(cloud)
    first = m.clear_seen_through_device(d_scan.data_ptr(), d_scan.shape[0], T, sensor, window=window)
    _, M = m.get_map()
    say(f"{tag}: {len(m)} voxels, {M} map points, scan {d_scan.shape[0]} points, image {sensor.n_scan} x {sensor.horizon_scan}, "
        f"window {window}; first call {first}")
    tc, ta, tq = [], [], []
    for r in range(WARM + ROUNDS):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        st = m.clear_seen_through_device(d_scan.data_ptr(), d_scan.shape[0], T, sensor, window=window)
        t1 = time.perf_counter()
        m.add_pointcloud_device(d_cloud.data_ptr(), d_cloud.shape[0], T)
        t2 = time.perf_counter()
        _, Mq = m.get_map(T, query_r)
        t3 = time.perf_counter()
        if r >= WARM:
            tc.append(t1 - t0); ta.append(t2 - t1); tq.append(t3 - t2)
    ms = lambda v: "median %.3f ms (min %.3f, max %.3f)" % (1e3 * np.median(v), 1e3 * min(v), 1e3 * max(v))
    say(f"  clear_seen_through : {ms(tc)}   last call {st}")
    say(f"  add_cloud          : {ms(ta)}   {d_cloud.shape[0]} points")
    say(f"  query              : {ms(tq)}   {Mq} points")


# (a) the OS1-64 drive's map
sensor = pl.SEG_PRESETS["OS1-64"]
scans = mv.drive_scans(sc, sensor, 8, True)
m = pl.DeviceVoxelHashMap(1.0, 100.0, 20)
for T, scan in scans[:7]:
    m.add_pointcloud(pl.downsample_uniform(pl.crop_pointcloud(scan, 1.0, 100.0)[0], 0.5), T)
T, scan = scans[7]
cropped = np.asarray(pl.crop_pointcloud(scan, 1.0, 100.0)[0], np.float32)
measure("OS1-64 drive", m, sensor, T, cropped, pl.downsample_uniform(cropped, 0.5), 110.0)
m.close()

# (b) gpu_time_map.py's configuration
scene = sc.make_scene(sc.SEED)
sensor = pl.SEG_PRESETS["HDL-64E"]
m = pl.DeviceVoxelHashMap(0.5, 100.0, 20)
for i in range(20):
    t = np.array([0.5 * i, 0.0, 0.0])
    pts = sc.lidar_scan(scene, np.eye(3), t, 131072, stream=100 + i).astype(np.float32)
    T = np.eye(4); T[:3, 3] = t
    if i < 19:
        m.add_pointcloud(pts, T)
measure("131072-point scans", m, sensor, T, pts, pts, 110.0)
measure("131072-point scans, single pixel", m, sensor, T, pts, pts, 110.0, window=(0, 0))
m.close()

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "visibility_timing.log"), "w") as f:
    f.write("\n".join(lines) + "\n")
