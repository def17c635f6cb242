"""bring-up timing helper (not a pytest file): range-image segmentation (svnicp_prep_segment) of one 131 072-point HDL-64E scan
(the first 2 048 of the 2 250 columns of scans.lidar_grid_scan: ground, walls and boxes), against the C++ host restatement
(registration_pipeline.hpp: segment_scan, tests/segment_driver.cpp, -O2); and the scan-to-map cycle with and without
PipelineConfig.segmentation under gpu_map + gpu_prep.  Device times: hipEvents around the call (which ends in its own stream
synchronisation) and wall time, after a warm-up, host scan and device-resident scan."""
import os, struct, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g
pkg = g.load_package()
import torch
from svnicp_amd import pipeline as pl
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
sc = pkg.scans
prm = pl.SEG_PRESETS["HDL-64E"]
pts = sc.lidar_grid_scan(sc.make_scene(), sc.rot_zyx(0, 0, 0.3), np.array([1.0, -2.0, 0.0]), prm, 5)[:131072].astype(np.float32)
tp = torch.from_numpy(pts).cuda()
prep = pl.DevicePreprocessor(0)
runs = {"prep_segment (host xyz)": lambda: prep.segment(pts, prm), "prep_segment (device xyz)": lambda: prep.segment(tp, prm)}
for f in runs.values():
    for _ in range(10):
        f()
torch.cuda.synchronize()
ev = {k: [] for k in runs}
wall = {k: [] for k in runs}
for _ in range(reps):
    for k, f in runs.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); t0 = time.perf_counter(); a.record()
        f()
        b.record(); torch.cuda.synchronize(); wall[k].append(time.perf_counter() - t0); ev[k].append(a.elapsed_time(b))
print(f"131072 points (HDL-64E grid scan), {reps} alternating repetitions; segmented {prep.n_segmented} points")
for k in runs:
    e, w = np.array(ev[k]), np.array(wall[k]) * 1e3
    print(f"{k:28s} events median {np.median(e):.3f} ms (p10 {np.percentile(e, 10):.3f}, p90 {np.percentile(e, 90):.3f})   "
          f"wall median {np.median(w):.3f} ms")
# the C++ host restatement on the same scan
with tempfile.TemporaryDirectory() as d:
    exe = os.path.join(d, "segment_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "svn-icp_amd", "host"), os.path.join(ROOT, "tests", "segment_driver.cpp"), "-o", exe])
    with open(os.path.join(d, "in.bin"), "wb") as f:
        f.write(bytes(pl.seg_params_struct(prm))); f.write(struct.pack("<i", pts.shape[0])); f.write(pts.tobytes())
    r = subprocess.run([exe, os.path.join(d, "in.bin"), os.path.join(d, "out.bin"), "21"], capture_output=True, text=True, timeout=600)
    print(next(l for l in r.stdout.splitlines() if l.startswith("host segment_scan")))
# the scan-to-map cycle, 144 000-point grid scans of a slow drive
scene = sc.make_scene()
scans = [sc.lidar_grid_scan(scene, sc.rot_zyx(0, 0, np.radians(0.4 * k)), np.array([0.08 * k, 0, 0]), prm, 900 + k).astype(np.float32)
         for k in range(24)]
for seg in (False, True):
    cfg = pl.PipelineConfig(min_range=1.0, max_range=80.0, voxel_size=0.5, map_voxel_size=0.5, particle_count=32, gpu_map=True,
                            gpu_prep=True, segmentation=seg,
                            solver=pkg.SteinICPParam(iterations=20, lr=1.0, max_dist=1.0, KNN_count=32, SVN_full_grad=False))
    pipe = pl.RegistrationPipeline(cfg, device=0)
    t = []
    for k, p in enumerate(scans):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = pipe.process_scan(p, 0.1 * k)
        torch.cuda.synchronize(); t.append(time.perf_counter() - t0)
    pre = res.preprocessing_s * 1e3
    print(f"pipeline cycle, gpu_prep, segmentation={seg!s:5s}: median {np.median(np.array(t[4:]) * 1e3):.3f} ms per scan "
          f"(scans 4..23; last scan pre-processing {pre:.3f} ms, source {pipe._prep.n_source} points)")
