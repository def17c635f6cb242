"""bring-up timing helper (not a pytest file): svnicp_prep_scan against svnicp_prep_scan_deskew on one 131 072-point scan
(64 beams x 2 048 columns, a sweep skewed by 3 deg of yaw and 0.8 m of travel), float64 stamps, voxel 0.5 m.  Both calls upload
the raw scan (+ 1 MB of stamps) and end in their own stream synchronisation; wall time around each call after a device
synchronise, alternating the two, after a warm-up of every size.  Also the deskew alone with the scan already in HBM
(SVNICP_MEM_DEVICE inputs)."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
import torch
from svnicp_amd.pipeline import DevicePreprocessor
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
sc = pkg.scans
delta = np.array([0.004, -0.006, 0.05, 0.8, 0.1, -0.03])
sw = sc.lidar_sweep(sc.make_scene(sc.SEED), np.eye(4), delta, 131072, stream=17)
pts = sw.points.astype(np.float32)
st = sw.stamps
tp, ts = torch.from_numpy(pts).cuda(), torch.from_numpy(st).cuda()
prep = DevicePreprocessor(0)
runs = {
    "prep_scan (host xyz)": lambda: prep.scan(pts, 1.0, 80.0, 0.5, 0.0),
    "prep_scan_deskew (host xyz + f64 stamps)": lambda: prep.scan(pts, 1.0, 80.0, 0.5, 0.0, stamps=st, delta=delta),
    "prep_scan (device xyz)": lambda: prep.scan(tp, 1.0, 80.0, 0.5, 0.0),
    "prep_scan_deskew (device xyz + stamps)": lambda: prep.scan(tp, 1.0, 80.0, 0.5, 0.0, stamps=ts, delta=delta),
    "prep_scan_deskew KITTI (device xyz)": lambda: prep.scan(tp, 1.0, 80.0, 0.5, 0.0, delta=delta, kitti=True),
}
for f in runs.values():   # warm-up: code objects, rocprim temporaries, buffer sizes
    for _ in range(5):
        f()
torch.cuda.synchronize()
times = {k: [] for k in runs}
for _ in range(reps):
    for k, f in runs.items():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        f()
        torch.cuda.synchronize(); times[k].append(time.perf_counter() - t0)
print(f"131072 points, voxel 0.5 m, {reps} alternating repetitions each; counts after the last call: cropped {prep.n_cropped}, "
      f"map {prep.n_map}, source {prep.n_source}")
for k, v in times.items():
    v = np.array(v) * 1e3
    print(f"{k:44s} median {np.median(v):.3f} ms  p10 {np.percentile(v, 10):.3f}  p90 {np.percentile(v, 90):.3f}")
