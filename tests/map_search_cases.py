"""Inputs and rules shared by tests/test_map_search_cpu.py and tests/test_map_search_gpu.py (svnicp_map_search_poses, DESIGN.md
§4.17): the drive search whose truth is a node of the fine lattice, the pose tolerance, and the stage-by-stage check of a device
search.  Everything is computed once and never modified."""
import functools

import numpy as np

import map_normals_cases as mn
import map_score_cases as ms

GATE = 0.5
# true corrections in units of GRID_STEP / 3: off the coarse lattice, on the lattice of a two-level search
TRUTHS = ((4, -2, 0, 0, 0, 5), (-5, 7, 0, 0, 0, -4), (1, 1, 0, 0, 0, 1), (10, -8, 0, 0, 0, 11))
TESTED_TRUTHS = (TRUTHS[0], TRUTHS[3])
JUMP_LATTICE = np.array(TRUTHS[0])
JUMP = JUMP_LATTICE * (np.array(ms.GRID_STEP) / 3.0)      # the pipeline's jump: (4, -2, 0, 0, 0, 5) · step / 3


def _pl():
    return ms._pkg().pipeline


def truth_correction(kt):
    return np.array(kt, float) * (np.array(ms.GRID_STEP) / 3.0)


def centre(kt):
    """The guess of a search on scan 4 of the drive whose true correction is kt · step / 3."""
    return ms.drive_scan(4)[1] @ np.linalg.inv(_pl().correction_to_pose(truth_correction(kt)))


@functools.lru_cache(maxsize=None)
def host_search(kt, levels, keep):
    """The numpy restatement on the drive map, scan 4's rows, gate 0.5, the grid of map_score_cases."""
    return mn.host_map("drive").search_poses(ms.drive_scan(4)[0], centre(kt), ms.GRID_EXTENT, ms.GRID_STEP, levels, keep, GATE)


def assert_poses_match(got, want, what=""):
    """1e-12 absolute on R, 1e-12 · max(1, |t|_inf) on t: four orders below half a float32 ulp of a 100 m coordinate, far above a
    dozen roundings plus the device's sin / cos.  -> the two maxima (R, t relative to its bound)."""
    got, want = np.asarray(got).reshape(-1, 12), np.asarray(want).reshape(-1, 12)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    eR = float(np.abs(got[:, :9] - want[:, :9]).max())
    bound = 1e-12 * np.maximum(1.0, np.abs(want[:, 9:]).max(axis=1))
    et = np.abs(got[:, 9:] - want[:, 9:]).max(axis=1)
    assert eR <= 1e-12, (what, eR)
    assert np.all(et <= bound), (what, float((et / bound).max()))
    return eR, float(et.max())


def check_search_stages(pl, dm, res, guess, ext, stp, levels, keep, gate, rows, rows_on_device=None):
    """Every level of the device's last search, stage by stage, each stage from the device's OWN output of the stage before:
    children == search_children of the kept list, poses against numpy, records bit-identical to svnicp_map_score_poses of the
    level's poses (rows on the same side as the search's), kept list == search_rank of the device's records.  -> the levels."""
    lat0, fine, m, active = pl.search_lattice(ext, stp, levels)
    counts, kepts = pl.search_level_counts(m, levels, keep)
    assert res["levels"] == levels and res["active_axes"] == len(active)
    assert res["level_count"] == counts and res["level_kept"] == kepts and res["nodes_scored"] == sum(counts)
    assert np.array_equal(res["fine_step"], fine)
    out, worst = [], (0.0, 0.0)
    for l in range(levels):
        lv = dm.search_level(l)
        want_lat = lat0 if l == 0 else pl.search_children(out[-1]["lattice"][out[-1]["kept"]], l - 1, levels, active)
        assert np.array_equal(lv["lattice"], want_lat), l
        e = assert_poses_match(lv["poses"], pl.correction_poses(guess, pl.search_corrections(lv["lattice"], fine)), f"level {l}")
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
        if rows_on_device is not None:
            alone = dm.score_poses_device(rows_on_device, rows.shape[0], lv["poses"], gate)
        else:
            alone = dm.score_poses(rows, lv["poses"], gate)
        assert lv["records"].tobytes() == alone.tobytes(), l
        assert np.array_equal(lv["kept"], pl.search_rank(lv["records"], lv["lattice"], keep)), l
        out.append(lv)
    last = out[-1]
    top = dm.search_top()
    order = last["kept"]
    assert np.array_equal(top["lattice"], last["lattice"][order]) and top["poses"].tobytes() == last["poses"][order].tobytes()
    assert top["records"].tobytes() == last["records"][order].tobytes()
    assert top["corrections"].tobytes() == pl.search_corrections(top["lattice"], fine).tobytes()
    assert np.array_equal(res["best_lattice"], top["lattice"][0]) and res["best_correction"].tobytes() == top["corrections"][0].tobytes()
    assert res["best_pose"].tobytes() == top["poses"][0].tobytes() and res["best_record"].tobytes() == top["records"][0].tobytes()
    assert res["zero_record"].tobytes() == out[0]["records"][pl.search_zero_index(m)].tobytes()
    print(f"levels {levels} keep {keep} counts {counts}: max pose error R {worst[0]:.3e} t {worst[1]:.3e}")
    return out
