"""svnicp_map_search_poses on the device: every level stage by stage against the helpers of pipeline.py and
against svnicp_map_score_poses, ties, determinism and side effects, the numpy restatement on the drive, refusals, and the
pipeline's seed_levels / seed_skip_fitness.  Pose tolerance: map_search_cases.assert_poses_match; records are compared bit for
bit with the scoring of the same poses, and with the restatement by map_score_cases.assert_scores_match."""
import ctypes as C
import importlib

import numpy as np
import pytest

import map_score_cases as ms
import map_search_cases as sc

pytestmark = pytest.mark.gpu
INVALID = -1   # SVNICP_ERR_INVALID
XYYAW = lambda e: (e, e, 0.0, 0.0, 0.0, e / 10.0)   # noqa: E731  three active axes
SIX = lambda e: (e, e, e, e / 10.0, e / 10.0, e / 10.0)   # noqa: E731  six


@pytest.fixture(scope="module")
def pl(hip):
    return importlib.import_module(hip.__name__ + ".pipeline")


def _device_map(pl, voxel, max_range, max_points, steps):
    dm = pl.DeviceVoxelHashMap(voxel, max_range, max_points, device=0)
    for cloud, T in steps:
        dm.add_pointcloud(cloud, T)
    return dm


@pytest.fixture(scope="module")
def drive(pl):
    voxel, mp, max_range, steps = ms.drive_steps()
    dm = _device_map(pl, voxel, max_range, mp, steps)
    yield dm
    dm.close()


def _on_device(rows):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(rows)).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    return t


def _search(dm, rows, guess, ext, stp, levels, keep, gate, dev_rows=None):
    if dev_rows is not None:
        return dm.search_poses_device(dev_rows.data_ptr(), rows.shape[0], guess, ext, stp, levels, keep, gate)
    return dm.search_poses(rows, guess, ext, stp, levels, keep, gate)


# ------------------------------------------------------------------------------------------------ 1. one level = the existing path
def test_one_level_is_the_flat_grid(pl, drive):
    rows, guess = ms.drive_scan(4)[0], sc.centre(sc.TRUTHS[0])
    nodes, zero = pl.correction_grid(ms.GRID_EXTENT, ms.GRID_STEP)
    res = drive.search_poses(rows, guess, ms.GRID_EXTENT, ms.GRID_STEP, 1, 8, sc.GATE)
    (lv,) = sc.check_search_stages(pl, drive, res, guess, ms.GRID_EXTENT, ms.GRID_STEP, 1, 8, sc.GATE, rows)
    assert pl.search_corrections(lv["lattice"], res["fine_step"]).tobytes() == nodes.tobytes()      # k · step, exactly
    sc.assert_poses_match(lv["poses"], pl.correction_poses(guess, nodes))
    assert lv["records"].tobytes() == drive.score_poses(rows, lv["poses"], sc.GATE).tobytes()
    best, first, order = pl.seed_from_scores(lv["records"], nodes, 8)
    top = drive.search_top()
    assert np.array_equal(lv["kept"], order) and top["corrections"].tobytes() == first.tobytes()
    assert res["best_correction"].tobytes() == best.tobytes() and res["zero_record"].tobytes() == lv["records"][zero].tobytes()


# ------------------------------------------------------------------------------------------------ 2. every level, stage by stage
@pytest.mark.parametrize("n,on_device,ext,levels,keep", [
    (1, False, XYYAW(0.3), 3, 8), (255, True, XYYAW(0.3), 3, 8), (256, False, XYYAW(0.3), 3, 8), (257, True, XYYAW(0.3), 3, 8),
    (300, False, SIX(0.3), 2, 2),            # six active axes: 729 nodes, then 2 · 729
    (300, True, XYYAW(0.3), 3, 1),           # keep = 1
    (64, False, XYYAW(1.5), 2, 1024),        # 11^3 = 1331 nodes, 1024 kept: 27 648 children
    (64, True, SIX(0.3), 2, 64),             # 64 · 729 = 46 656 nodes at level 1: two launches of the scoring's 32 768-pose batch
])
def test_every_level_stage_by_stage(pl, drive, n, on_device, ext, levels, keep):
    stp = XYYAW(0.3) if ext[2] == 0.0 else SIX(0.3)
    rows, guess = ms.drive_rows(n), sc.centre(sc.TRUTHS[1])
    dev = _on_device(rows) if on_device else None
    res = _search(drive, rows, guess, ext, stp, levels, keep, sc.GATE, dev)
    out = sc.check_search_stages(pl, drive, res, guess, ext, stp, levels, keep, sc.GATE, rows, dev.data_ptr() if on_device else None)
    assert len(out) == levels and out[-1]["lattice"].shape[0] == res["level_count"][-1]
    assert res["best_record"][3] <= res["zero_record"][3]


# ------------------------------------------------------------------------------------------------ 3. ties
@pytest.mark.parametrize("ext,levels,keep", [(XYYAW(0.3), 3, 5), (SIX(0.3), 2, 64)])
def test_ties_keep_the_lexicographically_smallest_nodes(pl, drive, ext, levels, keep):
    stp = XYYAW(0.3) if ext[2] == 0.0 else SIX(0.3)
    rows = ms.drive_rows(300)
    empty = pl.DeviceVoxelHashMap(0.5, 100.0, 20, device=0)
    corner = -(3 ** (levels - 1) + (3 ** (levels - 1) - 1) // 2)
    for dm, r in ((empty, rows), (drive, rows[:0])):
        res = dm.search_poses(r, np.eye(4), ext, stp, levels, keep, sc.GATE)
        out = sc.check_search_stages(pl, dm, res, np.eye(4), ext, stp, levels, keep, sc.GATE, r)
        for lv in out:
            assert np.array_equal(lv["records"], np.tile([0.0, 0.0, 0.0, sc.GATE ** 2], (lv["records"].shape[0], 1)))
            smallest = np.lexsort(lv["lattice"].T[::-1])[:keep]
            assert np.array_equal(lv["kept"], smallest)
        assert np.array_equal(out[0]["kept"], np.arange(min(keep, out[0]["lattice"].shape[0])))          # level 0: index order
        assert res["best_lattice"].tolist() == [corner if e else 0 for e in ext]
        assert res["best_record"].tolist() == [0.0, 0.0, 0.0, sc.GATE ** 2] == res["zero_record"].tolist()
    empty.close()


# ------------------------------------------------------------------------------------------------ 4. determinism, side effects
class _DeviceDoubles:
    """Library-owned float64 device memory as torch sees it (__cuda_array_interface__)."""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f8", "data": (int(ptr), False), "version": 2, "strides": None}


def _all_bytes(dm, res):
    parts = [np.asarray(res[k]).tobytes() for k in sorted(res)]
    top = dm.search_top()
    parts += [top[k].tobytes() for k in sorted(top)]
    for l in range(res["levels"]):
        lv = dm.search_level(l)
        parts += [lv[k].tobytes() for k in sorted(lv)]
    return b"".join(parts)


def test_determinism_and_no_side_effects(pl):
    import torch
    voxel, mp, max_range, steps = ms.drive_steps()
    dm = _device_map(pl, voxel, max_range, mp, steps[:3])
    twin = _device_map(pl, voxel, max_range, mp, steps[:3])
    centre, radius = ms.drive_scan(4)[1], 30.0
    _, M = dm.get_map(centre, radius)
    _, with_normal = dm.get_map_normals(16)
    scores = dm.score_poses(ms.drive_rows(800), ms.drive_poses(16), 0.5)
    rows0, nrm0, info0, size0, sptr0 = dm.download(), dm.download_normals(), dm.table_info(), len(dm), dm.scores_ptr
    assert M > 1000 and with_normal > 0 and sptr0 != 0
    rows, guess = ms.drive_rows(700), sc.centre(sc.TRUTHS[2])
    args = (guess, ms.GRID_EXTENT, ms.GRID_STEP, 3, 8, sc.GATE)
    first = _all_bytes(dm, dm.search_poses(rows, *args))
    assert _all_bytes(dm, dm.search_poses(rows, *args)) == first                                        # two calls
    dev = _on_device(rows)
    assert _all_bytes(dm, dm.search_poses_device(dev.data_ptr(), rows.shape[0], *args)) == first         # rows on the device
    assert dm.scores_ptr == sptr0
    view = torch.as_tensor(_DeviceDoubles(sptr0, (16, 4)), device="cuda:0")
    assert view.cpu().numpy().tobytes() == scores.tobytes()                                             # the earlier scoring's records
    assert np.array_equal(dm.download(), rows0) and np.array_equal(dm.download_normals(), nrm0)
    assert dm.get_map_normals(16)[1] == with_normal and np.array_equal(dm.download_normals(), nrm0)     # the query is still valid
    assert dm.table_info() == info0 and len(dm) == size0
    cloud, T = steps[3]
    dm.add_pointcloud(cloud, T); twin.add_pointcloud(cloud, T)
    dm.get_map(); twin.get_map()
    assert dm.table_info() == twin.table_info() and len(dm) == len(twin)
    assert dm.download().tobytes() == twin.download().tobytes()
    dm.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 5. against the restatement
@pytest.mark.parametrize("kt", sc.TESTED_TRUTHS)
def test_device_against_the_restatement_on_the_drive(pl, drive, kt):
    want = sc.host_search(kt, 2, 8)
    got = drive.search_poses(ms.drive_scan(4)[0], sc.centre(kt), ms.GRID_EXTENT, ms.GRID_STEP, 2, 8, sc.GATE)
    assert got["best_lattice"].tolist() == want["best_lattice"].tolist() == list(kt)
    ms.assert_scores_match(got["best_record"][None], want["best_record"][None])
    zero = pl.search_zero_index(pl.search_lattice(ms.GRID_EXTENT, ms.GRID_STEP, 2)[2])
    assert got["zero_record"].tobytes() == drive.search_level(0)["records"][zero].tobytes()
    ms.assert_scores_match(got["zero_record"][None], want["zero_record"][None])


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(pl, drive):
    from_binding = importlib.import_module(pl.__name__.rsplit(".", 1)[0] + ".binding")
    L, h = drive._L, drive._h
    rows = ms.drive_rows(100)
    G = np.ascontiguousarray(sc.centre(sc.TRUTHS[0]))
    R, t = np.ascontiguousarray(G[:3, :3]), np.ascontiguousarray(G[:3, 3])
    dp = C.POINTER(C.c_double)
    rp, Rp, tp = rows.ctypes.data_as(C.c_void_p), R.ctypes.data_as(dp), t.ctypes.data_as(dp)

    def opt(ext=ms.GRID_EXTENT, stp=ms.GRID_STEP, levels=2, keep=8, gate=0.5):
        o = from_binding.MapSearchOptStruct()
        o.extent[:], o.step[:] = [float(v) for v in ext], [float(v) for v in stp]
        o.levels, o.keep, o.max_corr_dist = levels, keep, gate
        return o

    out = from_binding.MapSearchStruct()

    def refused(rows_p, n, Rq, tq, o, outp):
        rc = L.svnicp_map_search_poses(h, rows_p, n, 0, Rq, tq, o, outp)
        return rc == INVALID and len(L.svnicp_map_last_error(h).decode()) > 10

    fresh = pl.DeviceVoxelHashMap(0.5, 100.0, 20, device=0)                                             # before any search
    n_out = C.c_int(0)
    assert L.svnicp_map_search_top(fresh._h, 8, None, None, None, None, C.byref(n_out)) == INVALID
    assert L.svnicp_map_search_level(fresh._h, 0, 0, None, None, None, None, None, None) == INVALID
    fresh.close()
    for bad in (dict(levels=0), dict(levels=9), dict(keep=0), dict(keep=1025), dict(gate=0.5 + 1e-9), dict(gate=0.0), dict(gate=float("nan")),
                dict(ext=(1, 1, 1, 1, 0, 0), stp=(0.05,) * 6),                                         # 41^4 nodes at level 0
                dict(ext=(500, 0, 0, 0, 0, 0), stp=(1, 0, 0, 0, 0, 0), levels=8),                       # lattice overflow
                dict(ext=(1e7, 0, 0, 0, 0, 0), stp=(1, 0, 0, 0, 0, 0), levels=1),
                dict(ext=(1, 0, 0, 0, 0, 0), stp=(0, 0, 0, 0, 0, 0)), dict(ext=(-1, 0, 0, 0, 0, 0)), dict(ext=(float("inf"), 0, 0, 0, 0, 0))):
        assert refused(rp, 100, Rp, tp, C.byref(opt(**bad)), C.byref(out)), bad
    assert refused(rp, 100, Rp, tp, None, C.byref(out)) and refused(rp, 100, Rp, tp, C.byref(opt()), None)   # NULL option, NULL output
    assert refused(rp, 100, None, tp, C.byref(opt()), C.byref(out)) and refused(rp, 100, Rp, None, C.byref(opt()), C.byref(out))
    assert refused(None, 100, Rp, tp, C.byref(opt()), C.byref(out)) and refused(rp, -1, Rp, tp, C.byref(opt()), C.byref(out))
    for bad_value in (np.nan, np.inf):
        Rb, tb = R.copy(), t.copy()
        Rb[1, 1] = bad_value
        assert refused(rp, 100, Rb.ctypes.data_as(dp), tp, C.byref(opt()), C.byref(out))
        tb[2] = bad_value
        assert refused(rp, 100, Rp, tb.ctypes.data_as(dp), C.byref(opt()), C.byref(out))
    assert L.svnicp_map_search_poses(None, rp, 100, 0, Rp, tp, C.byref(opt()), C.byref(out)) == INVALID
    assert L.svnicp_map_search_poses(h, rp, 100, 0, Rp, tp, C.byref(opt()), C.byref(out)) == 0          # and the same call, valid
    assert out.levels == 2 and list(out.level_count[:2]) == [729, 216]
    for level in (-1, 2, 8):
        assert L.svnicp_map_search_level(h, level, 0, None, None, None, None, None, None) == INVALID
    assert L.svnicp_map_search_level(h, 1, -1, None, None, None, None, None, None) == INVALID
    assert L.svnicp_map_search_top(h, -1, None, None, None, None, C.byref(n_out)) == INVALID
    assert L.svnicp_map_search_top(h, 3, None, None, None, None, C.byref(n_out)) == 0 and n_out.value == 8
    assert drive.search_top(3)["lattice"].shape == (3, 6)


# ------------------------------------------------------------------------------------------------ 7. / 8. the pipeline
def _drive_truth(scans_mod, k):
    """The six-scan drive of tests/test_map_score_gpu.py; from scan 3 on the true pose is off the constant-velocity track by
    map_search_cases.JUMP = (4, -2, 0, 0, 0, 5) · GRID_STEP / 3: off the coarse lattice, on the lattice of two levels."""
    t = np.array([0.0, 0.0, 0.05 * k])
    yaw = np.radians(0.3 * k)
    if k >= 3:
        t = t + sc.JUMP[:3]
        yaw += sc.JUMP[5]
    return ms.pose(scans_mod.rot_zyx(0.0, 0.0, yaw), t)


@pytest.fixture(scope="module")
def jump_scans(hip):
    scans_mod = hip.scans
    scene = scans_mod.make_scene()
    out = []
    for k in range(6):
        T = _drive_truth(scans_mod, k)
        out.append((T, scans_mod.lidar_scan(scene, T[:3, :3], T[:3, 3], 32768, stream=900 + k)))
    return out


GRID = (ms.GRID_EXTENT, ms.GRID_STEP)


def _run(hip, pl, scans, **kw):
    cfg = pl.PipelineConfig(min_range=1.0, max_range=80.0, voxel_size=0.5, map_voxel_size=0.5, map_voxel_max_points=20, map_range=100.0,
                            particle_count=32, seed=5,
                            solver=hip.SteinICPParam(iterations=20, lr=1.0, max_dist=1.0, KNN_count=50, SVN_full_grad=False), **kw)
    pipe = pl.RegistrationPipeline(cfg, device=0)
    return pipe, [pipe.process_scan(pts, stamp=0.1 * k) for k, (_, pts) in enumerate(scans)]


def _errors(pl, T, E):
    return float(np.linalg.norm(T[:3, 3] - E[:3, 3])), float(np.linalg.norm(pl.so3_log(T[:3, :3].T @ E[:3, :3])))


@pytest.fixture(scope="module")
def two_level_runs(hip, pl, jump_scans):
    """seed_levels=2 over the six scans with the device map; with the host map (the numpy restatement searches) the first four."""
    return {gpu_map: _run(hip, pl, jump_scans if gpu_map else jump_scans[:4], gpu_map=gpu_map, seed_grid=GRID, seed_levels=2)[1]
            for gpu_map in (False, True)}


def test_pipeline_with_two_levels_recovers_a_jump_off_the_coarse_lattice(hip, pl, jump_scans, two_level_runs):
    """The bounds are those test_pipeline_seeded_with_the_best_node_recovers_a_jump asserts (0.05 m, 0.01 rad).  Printed, not
    asserted: how far the registration's start is from the truth with one level and with two."""
    runs, truth = two_level_runs, jump_scans[3][0]
    _, flat = _run(hip, pl, jump_scans[:4], gpu_map=True, seed_grid=GRID)
    for name, r in (("one level ", flat[3]), ("two levels", runs[True][3])):
        st, sr = _errors(pl, truth, r.initial_guess)
        et, er = _errors(pl, truth, r.pose)
        print(f"scan 3, {name}: start {st:.4f} m {sr:.5f} rad from the truth, result {et:.4f} m {er:.5f} rad, seed cost {r.seed['cost']:.5f} "
              f"at {r.seed.get('lattice', r.seed.get('index'))}")
    for gpu_map in (False, True):
        r3 = runs[gpu_map][3]
        s = r3.seed
        assert np.array_equal(r3.initial_guess, s["prediction"] @ pl.correction_to_pose(s["correction"]))
        assert s["cost"] <= s["cost_level0"] and s["levels"] == 2 and s["nodes_scored"] == 729 + 216
        assert np.array_equal(s["correction"], s["lattice"].astype(np.float64) * s["fine_step"])
        et, er = _errors(pl, truth, r3.pose)
        assert et < 0.05 and er < 0.01, (gpu_map, et, er)
        assert runs[gpu_map][0].seed is None                                                            # scan 0 seeds the map
    dev, host = (np.array([r.pose for r in runs[g][:4]]) for g in (True, False))
    assert np.allclose(dev, host, rtol=0, atol=1e-9)
    assert all(np.array_equal(a.seed["lattice"], b.seed["lattice"]) for a, b in zip(runs[True][1:4], runs[False][1:]))
    for k in (4, 5):                                                                                    # the drive goes on from the recovered pose
        et, er = _errors(pl, jump_scans[k][0], runs[True][k].pose)
        assert et < 0.05 and er < 0.01, (k, et, er)


def test_pipeline_top_mode_hands_over_the_first_nodes_of_the_search(hip, pl, jump_scans, monkeypatch):
    handed, tops = [], []
    real = hip.SVNICP.add_cloud_device_target
    real_search = pl.DeviceVoxelHashMap.search_poses

    def spy(self, new_cloud, target_devptr, M, init_pose):
        handed.append(np.array(init_pose, float))
        return real(self, new_cloud, target_devptr, M, init_pose)

    def spy_search(self, *a, **k):
        res = real_search(self, *a, **k)
        tops.append((self.search_top(32), a[4], a[5]))
        return res

    monkeypatch.setattr(hip.SVNICP, "add_cloud_device_target", spy)
    monkeypatch.setattr(pl.DeviceVoxelHashMap, "search_poses", spy_search)
    _, res = _run(hip, pl, jump_scans[:4], gpu_map=True, seed_grid=GRID, seed_levels=2, seed_mode="top")
    assert len(handed) == len(tops) == 3
    for k in (1, 2, 3):
        top, levels, keep = tops[k - 1]
        assert (levels, keep) == (2, 32)                                                                # keep = max(seed_keep, particle_count)
        assert handed[k - 1].tobytes() == np.ascontiguousarray(top["corrections"].T).tobytes()
        s = res[k].seed
        assert np.array_equal(res[k].initial_guess, s["prediction"]) and not s["correction"].any()     # the mean stays the prediction
        assert np.array_equal(s["nodes"], top["lattice"]) and np.array_equal(s["lattice"], top["lattice"][0])


def test_one_level_with_defaults_is_todays_path(hip, pl, jump_scans, monkeypatch):
    _, a = _run(hip, pl, jump_scans[:4], gpu_map=True, seed_grid=GRID)

    def boom(*args, **kw):
        raise AssertionError("search_poses called although seed_levels == 1")

    for cls in (pl.DeviceVoxelHashMap, pl.VoxelHashMap):
        monkeypatch.setattr(cls, "search_poses", boom)
    monkeypatch.setattr(pl.DeviceVoxelHashMap, "search_poses_device", boom)
    _, b = _run(hip, pl, jump_scans[:4], gpu_map=True, seed_grid=GRID, seed_levels=1, seed_keep=8, seed_skip_fitness=0.0)
    assert all(x.pose.tobytes() == y.pose.tobytes() for x, y in zip(a, b))
    want = {"index", "cost", "cost_zero", "correction", "prediction"}
    assert all(set(x.seed) == want == set(y.seed) for x, y in zip(a[1:], b[1:]))


# The skip test's search: level 0 at three times the grid's step, so that the FINE level is the 0.5 m / 2.5 deg lattice.  Scan 3 of a
# run that skips scans 1-2 can only equal, byte for byte, scan 3 of a run that searched them if those searches returned the zero
# correction.  A fine step of 0.167 m lies inside the cost's sampling noise while the map holds one or two scans (measured with
# GRID at two levels: scan 1 moved off the zero node, and scan 2's fitness_zero then differs, 0.871 against 0.905); at 0.5 m /
# 2.5 deg the nearest node wins by a factor of two in cost, and on the track that node is the zero.
SKIP_GRID = (ms.GRID_EXTENT, tuple(3.0 * v for v in ms.GRID_STEP))


def test_skip_policy_searches_only_where_the_prediction_fits_badly(hip, pl, jump_scans, monkeypatch):
    scans = jump_scans[:4]
    _, first = _run(hip, pl, scans, gpu_map=True, seed_grid=SKIP_GRID, seed_levels=2)
    fit = [r.seed["fitness_zero"] for r in first[1:]]
    print("fitness of the prediction, scans 1-3:", [round(f, 4) for f in fit], "lattice:", [r.seed["lattice"].tolist() for r in first[1:]])
    assert fit[2] < min(fit[:2])
    threshold = 0.5 * (fit[2] + min(fit[:2]))
    calls = []
    for name in ("search_poses", "search_poses_device"):
        real = getattr(pl.DeviceVoxelHashMap, name)
        monkeypatch.setattr(pl.DeviceVoxelHashMap, name, (lambda real: lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])(real))
    real_scan = pl.RegistrationPipeline.process_scan
    per_scan = []

    def counted_scan(self, *a, **k):
        before = len(calls)
        r = real_scan(self, *a, **k)
        per_scan.append(len(calls) - before)
        return r

    monkeypatch.setattr(pl.RegistrationPipeline, "process_scan", counted_scan)
    _, res = _run(hip, pl, scans, gpu_map=True, seed_grid=SKIP_GRID, seed_levels=2, seed_skip_fitness=threshold)
    assert per_scan == [0, 0, 0, 1]                                                                      # scans 1-2 make no search, scan 3 does
    for k in (1, 2):
        s = res[k].seed
        assert set(s) == {"searched", "fitness_zero", "cost_zero", "prediction"} and s["searched"] is False
        assert s["fitness_zero"] >= threshold and np.array_equal(res[k].initial_guess, s["prediction"])
    s = res[3].seed
    assert s["searched"] is True and s["fitness_zero"] < threshold and "lattice" in s
    assert res[3].pose.tobytes() == first[3].pose.tobytes()
