"""Normals from the voxel map's own cells (svnicp_map_query_normals) without a GPU: the interface is
declared, exported and mirrored; tests/map_normals_reference.py — the numpy restatement the GPU tests hold the kernel to —
returns the normal of a known plane, covers the drive's map, and feeds a plane-mode scan-to-map step on the CPU oracle that
ends well inside point mode's error; the pipeline's switch refuses the configurations it cannot serve."""
import ctypes as C

import numpy as np
import pytest

import map_normals_cases as mc
import map_normals_reference as mr
import plane_reference as pr

NEW_EXPORTS = ("svnicp_map_query_normals", "svnicp_map_normals_devptr", "svnicp_map_download_normals")


def test_map_normals_interface_is_declared_exported_and_mirrored(pkg):
    declared = pkg.binding.declared_symbols()
    for name in NEW_EXPORTS:
        assert name in declared, f"include/svnicp_hip.h does not declare {name}"
    L = C.CDLL(pkg.binding.library_path())
    for name in NEW_EXPORTS:
        assert hasattr(L, name), f"libsvnicp_hip.so does not export {name}"
    L = pkg.load_library()
    assert L.svnicp_map_query_normals.argtypes[1:] == [C.c_int, C.POINTER(C.c_int64)]
    assert L.svnicp_map_normals_devptr.restype is C.c_void_p
    for m in ("get_map_normals", "download_normals"):
        assert callable(getattr(pkg.pipeline.DeviceVoxelHashMap, m))
    assert callable(pkg.SVNICP.set_target_normals_device)
    assert pkg.pipeline.PipelineConfig().map_normals is False
    assert pkg.binding.abi_version() == 1


def test_restatement_returns_the_normal_of_a_known_plane(pkg):
    """A tilted plane with 2 mm noise, 6 000 points over 12 m x 12 m, voxel 1.0: every valid normal is within 3 degrees of
    the plane's (sigma / extent of a 16-neighbourhood, about 0.002 / 0.3, is 0.4 degrees; 3 degrees leaves room for the
    tails of 6 000 draws), and the neighbour lists start with the point itself."""
    rng = np.random.default_rng(5)
    n_true = np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])
    xy = rng.uniform(-6, 6, size=(6000, 2))
    z = -(n_true[0] * xy[:, 0] + n_true[1] * xy[:, 1]) / n_true[2] + rng.normal(0, 0.002, 6000)
    hm = pkg.pipeline.VoxelHashMap(1.0, 1e9, 20)
    hm.add_pointcloud(np.column_stack([xy, z]).astype(np.float32), np.eye(4))
    ref = mr.map_normals(hm._vox, 16)
    assert ref.valid.mean() > 0.9
    cosang = np.abs(ref.normals[ref.valid] @ n_true)
    print(f"known plane: valid {ref.valid.mean():.3f}, worst angle {np.degrees(np.arccos(cosang.min())):.3f} deg")
    assert cosang.min() >= np.cos(np.radians(3.0))
    assert np.array_equal(ref.nbr[ref.valid][:, 0], np.flatnonzero(ref.valid))     # d2 = 0 first: the point itself
    assert np.array_equal(ref.normals[~ref.valid], np.zeros_like(ref.normals[~ref.valid]))


@pytest.mark.parametrize("kn,floor", [(8, 0.90), (16, 0.80)])
def test_drive_map_is_covered(pkg, kn, floor):
    """The drive's map (four scans at their true poses, voxel 0.5, 20 points per voxel: 22 876 points, 2.8 per voxel):
    measured 96.1 % of the points with a normal at normal_k 8 and 85.0 % at 16."""
    ref = mc.reference("drive", kn)
    l2 = np.where(ref.lam[:, 2] > 0, ref.lam[:, 2], 1.0)
    gap = (ref.lam[:, 1] - ref.lam[:, 0]) / l2
    print(f"drive map normal_k {kn}: {ref.points.shape[0]} points, with >= normal_k candidates {(ref.n_cand >= kn).mean():.4f}, "
          f"valid {ref.valid.mean():.4f}, median candidates {np.median(ref.n_cand):.0f}, smallest gap {gap[ref.valid].min():.3e}")
    assert ref.valid.mean() >= floor
    assert gap[ref.valid].min() >= mc.GAP_FLOOR


def test_scan_to_map_step_on_the_oracle(pkg, orc):
    """Scan 4 of the drive registered from scan 3's true pose against the four-scan map, 8 particles, 20 iterations, K = 50,
    max_dist 1, delta 0.1, normals from the map's cells at normal_k 8: plane mode ends within half of point mode's error in
    translation and in rotation.  Measured: point 22.9 mm / 4.1e-3 rad, plane 1.7 mm / 9.8e-5 rad, 94 % of the pairs accepted."""
    sc = pkg.scans
    ref = mc.reference("drive", 8)
    _, src, T4 = mc._drive_scan(4)
    T3 = mc.drive_pose(sc, 3)
    src = np.ascontiguousarray(src, np.float64)
    tgt = ref.points
    D = np.linalg.inv(T3) @ T4
    true6 = np.concatenate([D[:3, 3], pkg.pipeline.so3_log(D[:3, :3])])
    init = sc.make_particles(8)
    o = orc.Solver(init, iterations=20, lr=1.0, max_dist=1.0, knn_count=50)
    o.add_cloud(src, tgt, init)
    o.set_initial_mean(T3[:3, :3], T3[:3, 3])
    o.stein_align()
    pt, pa = pr.pose_error(o.get_transformation(), true6)
    r = pr.run(orc, src, tgt, ref.normals, init, K=50, iterations=20, max_dist=1.0, delta=0.1, R0=T3[:3, :3], t0=T3[:3, 3])
    qt, qa = pr.pose_error(r.solver.get_transformation(), true6)
    print(f"{src.shape[0]} source points, {tgt.shape[0]} map points: point mode {pt:.4e} m {pa:.4e} rad | plane {qt:.4e} m {qa:.4e} rad "
          f"| pairs accepted {r.stats[:, 0].mean() / src.shape[0]:.3f}")
    assert qt <= 0.5 * pt and qa <= 0.5 * pa


def test_map_normals_needs_the_device_map_and_plane_mode(pkg):
    pl = pkg.pipeline
    plane = pkg.SteinICPParam(residual="plane")
    with pytest.raises(ValueError, match="gpu_map"):
        pl.PipelineConfig(map_normals=True, solver=plane)
    with pytest.raises(ValueError, match="residual"):
        pl.PipelineConfig(map_normals=True, gpu_map=True)
    assert pl.PipelineConfig(map_normals=True, gpu_map=True, solver=plane).map_normals
    assert pl.PipelineConfig(gpu_map=True, solver=plane).map_normals is False      # plane mode with the solver's own pass


@pytest.mark.parametrize("name,above64,above128", [("dense65", 15, 0), ("dense130", 19, 15), ("dense256", 26, 16)])
def test_dense_cases_fill_voxels_past_the_first_block(pkg, name, above64, above128):
    """The dense cases of tests/test_map_normals_gpu.py: voxels filled over three calls up to max_points itself, 15 / 19 / 26
    of them past 64 points (the second 64-point block of k_map_normals), 15 and 16 past 128 at max_points 130 and 256."""
    mp, _ = mc.DENSE[name]
    sizes = np.array([len(v) for v in mc.host_map(name)._vox.values()])      # host_map asserts max == max_points, >= 10 above 64
    print(f"{name}: {sizes.size} voxels, {int(sizes.sum())} points, {int((sizes > 64).sum())} above 64, {int((sizes > 128).sum())} above 128")
    assert 85 <= sizes.size <= 94 and sizes.max() == mp
    assert int((sizes > 64).sum()) == above64 and int((sizes > 128).sum()) == above128
    assert len(mc.case_inputs(name)[3]) == 3
