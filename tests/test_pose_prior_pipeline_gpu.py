"""The pose prior through both pipelines (pipeline.py: PipelineConfig.prior_sigma; registration_pipeline.hpp through
pipeline_drive's switch): eight scans of a corridor — floor and two walls, no end walls (tests/pose_prior_cases.py) — with the
device map, 32 particles, the plane residual and the map's normals, with and without the prior.

Measured on an MI355X (variance of the correction along the corridor, cov[0], per registered scan): DESIGN.md section 4.18."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_prior_cases as cases

pytestmark = pytest.mark.gpu

P, I, K, VOXEL, N_SCANS = 32, 15, 20, 0.5, 8


@pytest.fixture(scope="module")
def drive_inputs(hip, tmp_path_factory):
    pl = hip.pipeline
    d = tmp_path_factory.mktemp("pose_prior_pipeline")
    rng = np.random.default_rng(11)
    scans = [(0.1 * k, cases.corridor_scan(k)) for k in range(N_SCANS)]
    parts = [hip.initialize_particles(P, pl.PRIOR_UB, pl.PRIOR_LB, rng) for _ in range(N_SCANS)]
    with open(d / "scans.bin", "wb") as f:
        f.write(struct.pack("<i", N_SCANS))
        for stamp, pts in scans:
            f.write(struct.pack("<di", stamp, pts.shape[0])); f.write(np.ascontiguousarray(pts, np.float32).tobytes())
    with open(d / "particles.bin", "wb") as f:
        for p in parts:
            f.write(np.ascontiguousarray(p, np.float64).tobytes())
    return d, scans, parts


def _python_run(hip, scans, parts, **kw):
    pl = hip.pipeline
    cfg = pl.PipelineConfig(min_range=1.0, max_range=80.0, voxel_size=VOXEL, map_voxel_size=VOXEL, map_voxel_max_points=20,
                            map_range=100.0, particle_count=P, gpu_map=True, map_normals=True,
                            solver=hip.SteinICPParam(iterations=I, lr=1.0, max_dist=1.0, KNN_count=K, SVN_full_grad=False, residual="plane"),
                            **kw)
    pipe = pl.RegistrationPipeline(cfg, device=0)
    it = iter(parts)
    pipe._particles = lambda: next(it)
    res = [pipe.process_scan(pts, stamp) for stamp, pts in scans]
    assert res[0].state is None and all(r.state == int(hip.SteinICPState.ALIGN_SUCCESS) for r in res[1:])
    return res


def _drive(root, d, prior):
    from test_pipeline_gpu import _build_pipeline_drive
    exe = _build_pipeline_drive(root)
    args = [exe, str(d / "scans.bin"), str(d / "out.bin"), str(P), str(I), str(K), str(VOXEL), str(d / "particles.bin"),
            "1", "0", "0", "1", "0", "off", "off", "0", "0", "0", "0", "8", "0", "0", "0", "0", "0"]
    if prior:
        args += [repr(cases.CORRIDOR_POINT_SIGMA)] + [repr(v) for v in cases.CORRIDOR_SIGMA]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(d / "out.bin", "rb").read()
    off = 0

    def take(dtype, n):
        nonlocal off
        a = np.frombuffer(raw, dtype, n, off); off += a.nbytes
        return a
    poses = []
    for k in range(N_SCANS):
        aligned = int(take("<i4", 1)[0])
        pose = take("<f8", 12)
        take("<f8", 12 + 6 + 6 + 36)
        B, M = (int(v) for v in take("<i8", 2))
        take("<f8", 3 * B + 3 * M + 6 * P)
        if aligned:
            take("<i8", 1)
        assert aligned == (1 if k else 0)
        T = np.eye(4); T[:3, :3] = pose[:9].reshape(3, 3); T[:3, 3] = pose[9:]
        poses.append(T)
    assert off == len(raw)
    chi2 = {int(l.split()[1].rstrip(":")): float(l.split()[2]) for l in r.stdout.splitlines() if l.startswith("prior ")}
    return poses, chi2


@pytest.fixture(scope="module")
def runs(hip, drive_inputs):
    _, scans, parts = drive_inputs
    return {"off": _python_run(hip, scans, parts),
            "off_again": _python_run(hip, scans, parts, prior_sigma=None),
            "on": _python_run(hip, scans, parts, prior_sigma=cases.CORRIDOR_SIGMA, prior_point_sigma=cases.CORRIDOR_POINT_SIGMA)}


@pytest.mark.parametrize("prior", [False, True], ids=["off", "on"])
def test_cpp_drive_agrees_with_python(hip, drive_inputs, runs, prior):
    d = drive_inputs[0]
    root = os.path.dirname(os.path.dirname(hip.library_path()))
    poses, chi2 = _drive(root, d, prior)
    res = runs["on" if prior else "off"]
    print("prior %s: max |pose(python) - pose(drive)| per scan:" % ("on" if prior else "off"),
          " ".join("%.2e" % np.abs(res[k].pose - poses[k]).max() for k in range(N_SCANS)))
    for k in range(N_SCANS):
        assert np.allclose(res[k].pose, poses[k], rtol=0, atol=1e-9), k
    if prior:
        assert sorted(chi2) == list(range(1, N_SCANS))
        for k in range(1, N_SCANS):
            assert abs(chi2[k] - res[k].prior_chi2) <= 1e-6 * max(1.0, res[k].prior_chi2), k
    else:
        assert not chi2


def test_prior_chi2_only_when_asked(hip, runs):
    assert all(r.prior_chi2 is None for r in runs["off"])
    on = runs["on"]
    assert on[0].prior_chi2 is None     # the first scan seeds the map: no registration
    for r in on[1:]:
        want = float(np.sum((r.correction / np.asarray(cases.CORRIDOR_SIGMA)) ** 2))
        assert r.prior_chi2 is not None and np.isfinite(r.prior_chi2) and r.prior_chi2 == want


def test_prior_off_is_untouched(hip, runs):
    for a, b in zip(runs["off"], runs["off_again"]):
        assert np.array_equal(a.pose, b.pose)
        for x, y in ((a.correction, b.correction), (a.cov, b.cov), (a.particles, b.particles), (a.weights, b.weights)):
            assert (x is None and y is None) or np.array_equal(x, y)


def test_prior_narrows_the_unconstrained_direction(hip, runs):
    """The corridor's axis is x: cov[0] is the variance of the correction along it."""
    v_off = np.array([r.cov[0] for r in runs["off"][1:]])
    v_on = np.array([r.cov[0] for r in runs["on"][1:]])
    print("variance along the corridor per registered scan, without prior:", " ".join("%.3e" % v for v in v_off))
    print("variance along the corridor per registered scan, with prior:   ", " ".join("%.3e" % v for v in v_on))
    print("across the corridor (cov[7]) without / with:", " ".join("%.3e" % r.cov[7] for r in runs["off"][1:]), "/",
          " ".join("%.3e" % r.cov[7] for r in runs["on"][1:]))
    print("prior_chi2 per registered scan:", " ".join("%.3g" % r.prior_chi2 for r in runs["on"][1:]))
    assert np.isfinite(v_on).all()
    assert (v_on < v_off).all()
