"""The coarse-to-fine pose search against the voxel map, host side: the lattice and rank helpers, the numpy
restatement (pipeline.VoxelHashMap.search_poses) on the drive and on the crafted map, the C++ restatement
(registration_pipeline.hpp, tests/map_search_driver.cpp) against the numpy one, the declarations and the refusals."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import map_normals_cases as mn
import map_score_cases as ms
import map_search_cases as sc

pkg = ge.load_package()
pl = pkg.pipeline
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the lattice
def test_level0_of_one_level_is_the_correction_grid():
    for ext, stp in ((ms.GRID_EXTENT, ms.GRID_STEP), ((0.3, 0, 0.2, 0.01, 0, 0), (0.1, 0, 0.1, 0.01, 1, -1)), (np.zeros(6), np.zeros(6))):
        nodes, zero = pl.correction_grid(ext, stp)
        lat, fine, m, active = pl.search_lattice(ext, stp, 1)
        assert lat.dtype == np.int32 and pl.search_corrections(lat, fine).tobytes() == nodes.tobytes()
        assert pl.search_zero_index(m) == zero and not lat[zero].any()
        assert active == [a for a in range(6) if m[a] >= 1]
    lat, fine, m, active = pl.search_lattice(ms.GRID_EXTENT, ms.GRID_STEP, 3)
    assert m == [4, 4, 0, 0, 0, 4] and active == [0, 1, 5] and lat[0].tolist() == [-36, -36, 0, 0, 0, -36]
    assert fine.tolist() == [0.5 / 9.0, 0.5 / 9.0, 0.0, 0.0, 0.0, np.radians(2.5) / 9.0]                  # one division


def test_children_of_all_nodes_are_the_next_finer_grid():
    ext, stp = (1.0, 0.5, 0, 0, 0, 0.2), (0.5, 0.5, 0, 0, 0, 0.1)                                       # m = (2, 1, 0, 0, 0, 2)
    lat, fine, m, active = pl.search_lattice(ext, stp, 2)
    assert m == [2, 1, 0, 0, 0, 2]
    kids = pl.search_children(lat, 0, 2, active)
    assert kids.shape == (lat.shape[0] * 27, 6) and kids.dtype == np.int32
    assert len({tuple(k) for k in kids.tolist()}) == kids.shape[0]                                       # no duplicates
    finer_ext = [(3 * k + 1) * s / 3.0 if k else 0.0 for k, s in zip(m, stp)]                            # m' = 3m + 1
    finer, _, m2, _ = pl.search_lattice(finer_ext, [s / 3.0 for s in stp], 1)
    assert m2 == [7, 4, 0, 0, 0, 7]
    assert {tuple(k) for k in kids.tolist()} == {tuple(k) for k in finer.tolist()}
    nodes, _ = pl.correction_grid(finer_ext, [s / 3.0 for s in stp])
    assert np.allclose(np.sort(pl.search_corrections(kids, fine), axis=0), np.sort(nodes, axis=0), rtol=0, atol=1e-15)
    # the index formula: child = rank * 3^A + offset index, offsets lexicographic over the active axes with x slowest
    kept = lat[[7, 3, 11]]
    kids = pl.search_children(kept, 0, 2, active)
    offs = list(itertools.product((-1, 0, 1), repeat=3))
    for rank in range(3):
        for oi, o in enumerate(offs):
            want = kept[rank].astype(np.int64)
            want[active] += np.array(o)
            assert kids[rank * 27 + oi].tolist() == want.tolist()
    three = pl.search_children(kept[:1], 0, 3, active)                                                  # three levels: level-1 offsets are 3
    assert three[0].tolist() == (kept[0] + np.array([-3, -3, 0, 0, 0, -3])).tolist()
    assert pl.search_children(three[:1], 1, 3, active)[-1].tolist() == (three[0] + np.array([1, 1, 0, 0, 0, 1])).tolist()


def test_an_axis_with_an_extent_below_its_step_is_inactive():
    lat, fine, m, active = pl.search_lattice((0.4, 1.0, 0, 0, 0, 0), (0.5, 0.5, 0, 0, 0, 0), 2)
    assert m == [0, 2, 0, 0, 0, 0] and active == [1] and lat.shape == (5, 6) and not lat[:, 0].any()
    assert pl.search_children(lat[:2], 0, 2, active).shape == (6, 6)
    assert pl.search_level_counts(m, 2, 8) == ([5, 15], [5, 8])


# ------------------------------------------------------------------------------------------------ 2. the rank
def test_rank_orders_by_cost_then_lattice():
    nodes, _ = pl.correction_grid((1, 0, 0, 0, 0, 1), (0.5, 0, 0, 0, 0, 0.5))                            # 25 nodes
    lat, _, _, active = pl.search_lattice((1, 0, 0, 0, 0, 1), (0.5, 0, 0, 0, 0, 0.5), 1)
    scores = np.zeros((25, 4))
    scores[:, 3] = 1.0
    scores[[17, 4, 9], 3] = 0.25
    scores[20, 3] = 0.5
    assert pl.search_rank(scores, lat, 6).tolist() == pl.seed_from_scores(scores, nodes, 6)[2].tolist() == [4, 9, 17, 20, 0, 1]
    assert pl.search_rank(scores, lat, 1024).tolist() == pl.seed_from_scores(scores, nodes, 25)[2].tolist()      # keep > count
    # a child level: index order is not lexicographic order.  Parents (0,..,0) and (-3,..): the second parent's children are smaller
    lat2, _, _, active = pl.search_lattice((1, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0), 2)
    kids = pl.search_children(lat2[[1, 0]], 0, 2, active)                                               # [-1, 0, 1, -4, -3, -2] on x
    assert kids[:, 0].tolist() == [-1, 0, 1, -4, -3, -2]
    rec = np.zeros((6, 4))
    rec[:, 3] = [0.5, 0.25, 0.25, 0.25, 0.5, 0.25]
    assert pl.search_rank(rec, kids, 3).tolist() == [3, 5, 1]                                           # the tie goes to the smaller vector, the higher index
    assert pl.search_rank(rec, kids, 99).tolist() == [3, 5, 1, 2, 4, 0]
    with pytest.raises(ValueError):
        pl.search_rank(rec[:5], kids, 3)


# ------------------------------------------------------------------------------------------------ 3. the restatement on the drive
@pytest.mark.parametrize("kt", sc.TESTED_TRUTHS)
def test_two_levels_find_the_true_fine_node(kt):
    for keep in (8, 1):
        r = sc.host_search(kt, 2, keep)
        l0, l1 = r["level"]
        c0, c1 = l0["records"][l0["kept"][0], 3], r["best_record"][3]
        print(f"truth {kt} keep {keep}: best {r['best_lattice'].tolist()} cost {c1:.5f}, best of level 0 {c0:.5f}, nodes {r['nodes_scored']}")
        assert r["best_lattice"].tolist() == list(kt)
        assert c1 <= c0
        assert r["level_count"] == [729, 27 * keep] and r["nodes_scored"] == 729 + 27 * keep
        assert np.array_equal(r["best_correction"], sc.truth_correction(kt))                             # k · (step / 3), bit for bit


@pytest.mark.parametrize("kt", sc.TESTED_TRUTHS)
def test_three_levels_end_within_one_fine_step(kt):
    r = sc.host_search(kt, 3, 8)
    print(f"truth {kt}: best {r['best_lattice'].tolist()} (truth {[3 * k for k in kt]}) cost {r['best_record'][3]:.5f}")
    assert np.all(np.abs(r["best_lattice"] - 3 * np.array(kt)) <= 1)
    assert r["level_count"] == [729, 216, 216]


# ------------------------------------------------------------------------------------------------ 4. exhaustive equivalence
CRAFTED_EXT, CRAFTED_STEP = (0.375, 0.375, 0, 0, 0, 0.09), (0.375, 0.375, 0, 0, 0, 0.09)            # m = 1 on three axes
CRAFTED_GUESS = ms.pose(ms.rot90(2, 1), (0.25, -0.5, 1 / 64))


def test_everything_kept_equals_the_flat_grid_of_a_third_of_the_step():
    _, rows, _ = ms.crafted(1.0)
    hm = ms.crafted_host_map(1.0, 20)
    two = hm.search_poses(rows, CRAFTED_GUESS, CRAFTED_EXT, CRAFTED_STEP, 2, 27, 1.0)
    third = [s / 3.0 for s in CRAFTED_STEP]
    flat = hm.search_poses(rows, CRAFTED_GUESS, [4 * s if s else 0.0 for s in third], third, 1, 1, 1.0)
    assert two["level_count"] == [27, 729] and flat["level_count"] == [729]
    assert np.array_equal(two["best_lattice"], flat["best_lattice"])
    assert two["best_correction"].tobytes() == flat["best_correction"].tobytes()
    assert two["best_record"].tobytes() == flat["best_record"].tobytes()
    assert two["best_record"][3] < two["zero_record"][3]


# ------------------------------------------------------------------------------------------------ 5. the C++ restatement
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("search") / "map_search_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "svn-icp_amd", "host"), os.path.join(ROOT, "tests", "map_search_driver.cpp"), "-o", out])
    return out


def _cpp(driver, tmp_path, voxel, max_points, steps, rows, guess, ext, stp, levels, keep, gate, map_range=1e9):
    rows = np.ascontiguousarray(rows, np.float32)
    G = np.asarray(guess, float)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<ddidi", voxel, map_range, max_points, gate, len(steps)))
        for cloud, T in steps:
            cloud = np.ascontiguousarray(cloud, np.float32)
            f.write(np.ascontiguousarray(np.asarray(T, float)[:3, :3]).tobytes()); f.write(np.ascontiguousarray(np.asarray(T, float)[:3, 3]).tobytes())
            f.write(struct.pack("<i", cloud.shape[0])); f.write(cloud.tobytes())
        f.write(struct.pack("<i", rows.shape[0])); f.write(rows.tobytes())
        f.write(np.ascontiguousarray(G[:3, :3]).tobytes()); f.write(np.ascontiguousarray(G[:3, 3]).tobytes())
        f.write(np.asarray(ext, np.float64).tobytes()); f.write(np.asarray(stp, np.float64).tobytes())
        f.write(struct.pack("<ii", levels, keep))
    r = subprocess.run([driver, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        return r.returncode, r.stderr
    buf = open(tmp_path / "out.bin", "rb").read()
    nl, active = struct.unpack_from("<ii", buf, 0)
    off, level = 8, []
    for _ in range(nl):
        count, kept = struct.unpack_from("<qi", buf, off)
        off += 12
        lat = np.frombuffer(buf, np.int32, 6 * count, off).reshape(-1, 6); off += 24 * count
        rec = np.frombuffer(buf, np.float64, 4 * count, off).reshape(-1, 4); off += 32 * count
        idx = np.frombuffer(buf, np.int32, kept, off); off += 4 * kept
        level.append({"lattice": lat, "records": rec, "kept": idx})
    best_lat = np.frombuffer(buf, np.int32, 6, off); off += 24
    best_x, best_rec, zero_rec, fine = (np.frombuffer(buf, np.float64, k, off + 8 * o) for k, o in ((6, 0), (4, 6), (4, 10), (6, 14)))
    return 0, {"levels": nl, "active_axes": active, "level": level, "best_lattice": best_lat, "best_correction": best_x, "best_record": best_rec,
               "zero_record": zero_rec, "fine_step": fine}


def _same_search(got, want):
    assert got["levels"] == want["levels"] and got["active_axes"] == want["active_axes"]
    for g, w in zip(got["level"], want["level"]):
        assert np.array_equal(g["lattice"], w["lattice"]) and np.array_equal(g["kept"], w["kept"])
        ms.assert_scores_match(g["records"], w["records"])
    assert np.array_equal(got["best_lattice"], want["best_lattice"]) and got["best_correction"].tobytes() == want["best_correction"].tobytes()
    assert got["fine_step"].tobytes() == np.asarray(want["fine_step"]).tobytes()
    ms.assert_scores_match(got["best_record"][None], want["best_record"][None])
    ms.assert_scores_match(got["zero_record"][None], want["zero_record"][None])


def test_cpp_restatement_on_the_crafted_case(driver, tmp_path):
    stored, rows, _ = ms.crafted(1.0)
    want = ms.crafted_host_map(1.0, 20).search_poses(rows, CRAFTED_GUESS, CRAFTED_EXT, CRAFTED_STEP, 3, 5, 1.0)
    rc, got = _cpp(driver, tmp_path, 1.0, 20, [(stored, np.eye(4))], rows, CRAFTED_GUESS, CRAFTED_EXT, CRAFTED_STEP, 3, 5, 1.0)
    assert rc == 0, got
    _same_search(got, want)
    for bad in (dict(levels=0), dict(levels=9), dict(keep=0), dict(keep=1025), dict(gate=1.5)):
        kw = dict(levels=2, keep=4, gate=1.0)
        kw.update(bad)
        rc, err = _cpp(driver, tmp_path, 1.0, 20, [(stored, np.eye(4))], rows[:4], CRAFTED_GUESS, CRAFTED_EXT, CRAFTED_STEP, kw["levels"], kw["keep"], kw["gate"])
        assert rc == 2 and "refused" in err, (bad, rc, err)


def test_cpp_restatement_on_a_drive_truth(driver, tmp_path):
    voxel, max_points, map_range, steps = ms.drive_steps()
    kt = sc.TESTED_TRUTHS[0]
    want = sc.host_search(kt, 2, 1)
    rc, got = _cpp(driver, tmp_path, voxel, max_points, steps, ms.drive_scan(4)[0], sc.centre(kt), ms.GRID_EXTENT, ms.GRID_STEP, 2, 1, sc.GATE, map_range)
    assert rc == 0, got
    _same_search(got, want)
    assert got["best_lattice"].tolist() == list(kt)


# ------------------------------------------------------------------------------------------------ 6. declarations and refusals
def test_header_and_binding_declare_the_search():
    txt = open(os.path.join(ROOT, "include", "svnicp_hip.h")).read()
    assert "typedef struct svnicp_map_search_opt" in txt and "} svnicp_map_search;" in txt
    names = pkg.binding.declared_symbols()
    src = open(os.path.join(ROOT, "svn-icp_amd", "binding.py")).read()
    for fn in ("svnicp_map_search_poses", "svnicp_map_search_top", "svnicp_map_search_level"):
        assert fn in names and f"L.{fn}.argtypes" in src
    import ctypes as C
    b = pkg.binding
    assert C.sizeof(b.MapSearchOptStruct) == 12 * 8 + 2 * 4 + 8                                          # as the C struct lays out
    assert C.sizeof(b.MapSearchStruct) == 8 + 8 + 64 + 32 + 48 + 24 + 48 + 96 + 32 + 32
    assert pl.SEARCH_MAX_LEVELS == b.MAP_SEARCH_MAX_LEVELS == 8 and pl.SEARCH_MAX_KEEP == b.MAP_SEARCH_MAX_KEEP == 1024


def test_pipeline_config_refuses_inconsistent_search_fields():
    grid = (ms.GRID_EXTENT, ms.GRID_STEP)
    cfg = pl.PipelineConfig()
    assert cfg.seed_levels == 1 and cfg.seed_keep == 8 and cfg.seed_skip_fitness == 0.0
    for kw in (dict(seed_levels=2), dict(seed_skip_fitness=0.5), dict(seed_grid=grid, seed_levels=0), dict(seed_grid=grid, seed_levels=9),
               dict(seed_grid=grid, seed_keep=0), dict(seed_grid=grid, seed_keep=1025), dict(seed_grid=grid, seed_skip_fitness=-0.1),
               dict(seed_grid=grid, seed_skip_fitness=1.5), dict(seed_grid=grid, seed_skip_fitness=float("nan")),
               dict(seed_grid=grid, seed_levels=2, seed_mode="top", particle_count=1025),
               dict(seed_grid=((0.5, 0, 0, 0, 0, 0), (0.5, 0, 0, 0, 0, 0)), seed_levels=2, seed_mode="top", particle_count=10),   # 3 then 9 nodes
               dict(seed_grid=((500, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0)), seed_levels=8), dict(seed_grid=grid, seed_levels=2.0)):
        with pytest.raises(ValueError):
            pl.PipelineConfig(map_voxel_size=0.5, **kw)
    pl.PipelineConfig(seed_grid=grid, seed_levels=2, seed_mode="top", particle_count=128, map_voxel_size=0.5)   # keep = 128: 3456 nodes
    pl.PipelineConfig(seed_grid=grid, seed_levels=3, seed_keep=8, seed_skip_fitness=0.8, map_voxel_size=0.5)


def test_refusals_and_empties_of_the_restatement():
    hm = ms.crafted_host_map(1.0, 20)
    rows = ms.crafted(1.0)[1][:16]
    ok = dict(cloud=rows, guess=np.eye(4), extent6=CRAFTED_EXT, step6=CRAFTED_STEP, levels=2, keep=4, gate=1.0)
    hm.search_poses(**ok)
    six = dict(extent6=(1,) * 6, step6=(1,) * 6)
    for bad in (dict(levels=0), dict(levels=9), dict(keep=0), dict(keep=1025), dict(gate=1.0 + 1e-9), dict(gate=0.0), dict(gate=float("nan")),
                dict(extent6=(1, 1, 1, 1, 0, 0), step6=(0.05,) * 6),                                    # 41^4 nodes at level 0
                dict(extent6=(500, 0, 0, 0, 0, 0), step6=(1, 0, 0, 0, 0, 0), levels=8),                  # 500 * 3^7 + (3^7 - 1) / 2 >= 2^20
                dict(extent6=(1e7, 0, 0, 0, 0, 0), step6=(1, 0, 0, 0, 0, 0), levels=1),
                dict(extent6=(1, 0, 0, 0, 0, 0), step6=(0, 0, 0, 0, 0, 0)), dict(extent6=(-1, 0, 0, 0, 0, 0)),
                dict(guess=np.full((4, 4), np.nan)), dict(guess=np.eye(3))):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError):
            hm.search_poses(**kw)
    assert pl.search_level_counts([1] * 6, 3, 1024) == ([729, 531441, 746496], [729, 1024, 1024])       # the largest levels there are
    assert hm.search_poses(**dict(ok, **six, levels=1, keep=1024))["level_kept"] == [729]
    # n == 0 and an empty map: all costs tie at gate^2, the lexicographically smallest nodes are kept
    for r in (hm.search_poses(**dict(ok, cloud=np.zeros((0, 3), np.float32))), pl.VoxelHashMap(1.0, 1e9, 20).search_poses(**ok)):
        assert r["best_record"].tolist() == [0.0, 0.0, 0.0, 1.0] == r["zero_record"].tolist()
        assert r["best_lattice"].tolist() == [-4, -4, 0, 0, 0, -4]                                       # the most negative corner
        assert r["level"][0]["kept"].tolist() == [0, 1, 2, 3] and r["level"][1]["kept"].tolist() == [0, 1, 2, 27]
