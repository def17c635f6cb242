"""svnicp_evaluate without a device: the numpy restatement (tests/evaluate_reference.py) against a dense argmin, the figures
the feature was specified with, the preconditions the GPU cases (tests/test_evaluate_gpu.py) rely on, the ctypes mirror of
struct svnicp_eval against the header, and the host layers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import evaluate_cases as ec
import evaluate_reference as er
import plane_reference as pr


def test_reference_nearest_rows_equal_a_dense_argmin(pkg, orc):
    src, tgt = pkg.scans.random_clouds(300, 700, seed=3)
    T = pkg.pipeline.correction_to_pose([0.05, -0.03, 0.02, 0.004, -0.003, 0.006])
    ev = er.evaluate(orc, src, tgt, T, 0.3)
    q = src @ T[:3, :3].T + T[:3, 3]
    dense = ((q[:, None, :] - tgt[None, :, :]) ** 2).sum(axis=2)
    assert ev.evaluated == 300 and np.array_equal(ev.index, np.argmin(dense, axis=1))
    assert np.allclose(ev.d2, dense.min(axis=1), rtol=1e-12, atol=0)
    inl = dense.min(axis=1) < 0.09
    assert ev.inliers == int(inl.sum()) and ev.fitness == ev.inliers / 300
    assert ev.inlier_rmse == pytest.approx(np.sqrt(dense.min(axis=1)[inl].mean()), rel=1e-12)
    # the contract's neighbours (the helper for clouds with bad rows) agree with the oracle's on finite clouds
    ev2 = er.evaluate(orc, src, tgt, T, 0.3, finite=False)
    assert np.array_equal(ev.index, ev2.index) and np.array_equal(ev.d2, ev2.d2)


@pytest.fixture(scope="module")
def pair_figures(pkg, orc):
    src, tgt, poses = ec.clouds(pkg, "pair")
    nrm, _, _ = pr.normals(orc, tgt, 16)
    return {name: er.evaluate(orc, src, tgt, poses[name], 0.3, normals=nrm) for name in ("identity", "true_pose")}


# pose: fitness, inlier RMSE, plane inliers, plane RMSE — oracle transform + knn_topk(K = 1), plane_reference.normals(kn = 16),
# scans.make_pair(2048, 8192), gate 0.3 m, as the feature was specified
TABLE = {"identity": (0.8481, 0.1304, 1652, 0.0939), "true_pose": (0.8560, 0.1247, 1701, 0.0216)}


@pytest.mark.parametrize("pose", sorted(TABLE))
def test_specified_figures(pair_figures, pose):
    ev = pair_figures[pose]
    fit, rmse, n_pl, prmse = TABLE[pose]
    print(f"{pose}: fitness {ev.fitness:.6f} inlier_rmse {ev.inlier_rmse:.6f} plane_inliers {ev.plane_inliers} plane_rmse {ev.plane_rmse:.6f}")
    assert ev.fitness == pytest.approx(fit, rel=1e-3)
    assert ev.inlier_rmse == pytest.approx(rmse, rel=1e-3)
    assert ev.plane_inliers == pytest.approx(n_pl, rel=1e-3)
    assert ev.plane_rmse == pytest.approx(prmse, rel=1e-3)


def test_plane_rmse_separates_the_true_pose_where_the_point_figures_do_not(pair_figures):
    a, b = pair_figures["identity"], pair_figures["true_pose"]
    print(f"plane rmse ratio {b.plane_rmse / a.plane_rmse:.3f}, inlier rmse ratio {b.inlier_rmse / a.inlier_rmse:.3f}")
    assert b.plane_rmse < 0.5 * a.plane_rmse


@pytest.mark.parametrize("cloud", ec.CLOUDS)
@pytest.mark.parametrize("gate", ec.GATES)
def test_preconditions_of_the_gpu_cases(pkg, orc, cloud, gate):
    """The GPU cases compare indices and counts exactly: no row may sit on the gate (|d2 - thr2| <= 1e-9 thr2) or have its
    two nearest targets within 1e-12 relative, at either explicit pose."""
    src, tgt, poses = ec.clouds(pkg, cloud)
    for name in ("identity", "true_pose"):
        near_gate, tie = er.preconditions(er.evaluate(orc, src, tgt, poses[name], gate, with_second=True), gate)
        assert near_gate.size == 0 and tie.size == 0, (cloud, name, gate, near_gate, tie)


_FIELDS = ("struct_size", "has_normals", "rows", "evaluated", "inliers", "plane_inliers", "sum_d2", "sum_r2", "fitness",
           "inlier_rmse", "plane_rmse", "R", "t")


def test_eval_struct_matches_header(pkg, tmp_path):
    from svnicp_amd.binding import EvalStruct
    root = os.path.dirname(os.path.dirname(pkg.library_path()))
    src = tmp_path / "probe.c"
    body = "".join(f'  printf("%zu\\n", offsetof(svnicp_eval, {f}));\n' for f in _FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "svnicp_hip.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(svnicp_eval));\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert [name for name, _ in EvalStruct._fields_] == list(_FIELDS)
    assert got == [C.sizeof(EvalStruct)] + [getattr(EvalStruct, f).offset for f in _FIELDS]
    assert pkg.abi_version() == 1


def test_binding_declares_the_evaluate_symbols(pkg):
    names = ("svnicp_evaluate", "svnicp_eval_index_devptr", "svnicp_eval_dist2_devptr", "svnicp_get_eval_pairs")
    assert set(names) <= set(pkg.declared_symbols())
    L = pkg.load_library()
    for n in names:
        assert getattr(L, n).argtypes is not None, n
    assert L.svnicp_eval_index_devptr.restype is C.c_void_p and L.svnicp_eval_dist2_devptr.restype is C.c_void_p
    assert all(hasattr(pkg.SVNICP, m) for m in ("evaluate", "get_eval_pairs", "eval_index_ptr", "eval_dist2_ptr"))
    assert pkg.RegistrationEval.__dataclass_fields__.keys() >= {"fitness", "inlier_rmse", "plane_rmse", "plane_inliers", "pose"}


def test_pipeline_without_eval_dist_leaves_the_fields_unset(pkg):
    pl = pkg.pipeline
    assert pl.PipelineConfig().eval_dist == 0
    pipe = pl.RegistrationPipeline(pl.PipelineConfig(eval_dist=0, voxel_size=0.5, map_voxel_size=0.5))
    pts = pkg.scans.lidar_scan(pkg.scans.make_scene(), np.eye(3), np.zeros(3), 4096, stream=700)
    res = pipe.process_scan(pts, 0.0)           # the first scan seeds the host map: no solver, no device
    assert res.state is None and len(pipe.map) > 0
    assert res.fitness is None and res.inlier_rmse is None and res.plane_rmse is None and res.plane_inliers is None
