"""Cases of the visibility-clearing tests (svnicp_map_clear_seen_through), shared by test_map_visibility_cpu.py
and test_map_visibility_gpu.py: a tiny hand-placed sensor with expectations written out by hand, and the moving-box drive."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

F32 = np.float32


def tiny_sensor(pl):
    """8 rows x 90 columns at 4 degrees: rows cover elevations -16..+16, a column is 4 degrees of azimuth."""
    return pl.SegParams(n_scan=8, horizon_scan=90, ground_scan_ind=3, ang_res_x=4.0, ang_res_y=4.0, ang_bottom=16.0, min_range=1.0)


def beam(row, col, r, sensor=None):
    """The point at range r on the centre line of pixel (row, col) of tiny_sensor (or ``sensor``), float32, sensor frame."""
    ry = 4.0 if sensor is None else float(sensor.ang_res_y)
    rx = 4.0 if sensor is None else float(sensor.ang_res_x)
    bottom = 16.0 if sensor is None else float(sensor.ang_bottom)
    H = 90 if sensor is None else int(sensor.horizon_scan)
    el = math.radians(-bottom + (row + 0.5) * ry)
    h = math.radians(90.0 - (col - H // 2) * rx)          # h = atan2(x, y)
    return np.array([r * math.cos(el) * math.sin(h), r * math.cos(el) * math.cos(h), r * math.sin(el)], F32)


@dataclass
class Case:
    name: str
    scan: np.ndarray            # float32 [n,3], sensor frame
    points: np.ndarray          # float32 [m,3] map points, SENSOR frame (the test moves them into the map frame with ``pose``)
    removed: list               # expected, per map point, by hand
    tested: int                 # expected points_tested, by hand
    filled: int                 # expected pixels_filled, by hand
    window: tuple = (1, 1)
    margin: tuple = (0.3, 0.02)
    max_range: float = 100.0
    pose: np.ndarray = field(default_factory=lambda: np.eye(4))


def _a(*rows):
    return np.array(rows, F32).reshape(-1, 3)


def crafted_cases():
    """Every case: what the rule must do, decided by hand from the contract.  A point on the +x axis has elevation 0 and
    h = 90 degrees: pixel (4, 45) exactly, and its range is its x coordinate exactly — the threshold cases use that."""
    out = []
    # --- the threshold, absolute margin: r_min = 10, margin = max(0.3, 0.02 * 10 = 0.2) = 0.3
    thr = F32(10.0) - F32(0.3)
    out.append(Case("threshold_abs", _a([10, 0, 0]),
                    _a([thr, 0, 0], [np.nextafter(thr, F32(0)), 0, 0], [9.9, 0, 0], [12, 0, 0], [2, 0, 0]),
                    [False, True, False, False, True], tested=5, filled=1, window=(0, 0)))
    # --- the threshold, relative margin: r_min = 50, margin = max(0.3, 0.02f * 50) (about 1.0)
    thr = F32(50.0) - F32(0.02) * F32(50.0)
    out.append(Case("threshold_rel", _a([50, 0, 0]),
                    _a([thr, 0, 0], [np.nextafter(thr, F32(0)), 0, 0], [49.5, 0, 0], [48.5, 0, 0]),
                    [False, True, False, True], tested=4, filled=1, window=(0, 0)))
    # --- own pixel empty: kept whatever the neighbours say (far neighbours would remove it, near ones are no reason either)
    out.append(Case("own_pixel_empty", np.stack([beam(4, 44, 20), beam(4, 46, 20), beam(3, 45, 5), beam(5, 45, 20)]),
                    np.stack([beam(4, 45, 8)]), [False], tested=0, filled=4))
    # --- the window wraps across column 0 / H-1: own pixel far (20), the near return (10.1) sits across the seam
    seam_scan = np.stack([beam(4, 0, 20), beam(4, 89, 10.1), beam(2, 89, 20), beam(2, 0, 10.1)])
    seam_pts = np.stack([beam(4, 0, 10), beam(2, 89, 10)])
    out.append(Case("wrap_saves", seam_scan, seam_pts, [False, False], tested=2, filled=4, window=(0, 1)))
    out.append(Case("wrap_single_pixel", seam_scan, seam_pts, [True, True], tested=2, filled=4, window=(0, 0)))
    # --- rows do not wrap: a near return in row 7 does not save a point of row 0 (and the other way round) ...
    out.append(Case("rows_do_not_wrap", np.stack([beam(0, 10, 20), beam(7, 10, 10.1), beam(7, 30, 20), beam(0, 30, 10.1)]),
                    np.stack([beam(0, 10, 10), beam(7, 30, 10)]), [True, True], tested=2, filled=4, window=(1, 0)))
    # --- ... while the one row the edge leaves in the window still saves
    out.append(Case("rows_clamped", np.stack([beam(0, 10, 20), beam(1, 10, 10.1), beam(7, 30, 20), beam(6, 30, 10.1)]),
                    np.stack([beam(0, 10, 10), beam(7, 30, 10)]), [False, False], tested=2, filled=4, window=(1, 0)))
    # --- the ground at grazing incidence in miniature: the pixel below returned from nearly the point's range
    graze_scan = np.stack([beam(3, 60, 20), beam(2, 60, 10.2)])
    out.append(Case("neighbour_saves", graze_scan, np.stack([beam(3, 60, 10)]), [False], tested=1, filled=2, window=(1, 1)))
    out.append(Case("neighbour_ignored", graze_scan, np.stack([beam(3, 60, 10)]), [True], tested=1, filled=2, window=(0, 0)))
    # --- a window of columns only does not look at the row below
    out.append(Case("neighbour_other_axis", graze_scan, np.stack([beam(3, 60, 10)]), [True], tested=1, filled=2, window=(0, 8)))
    # --- outside the vertical field of view (elevation 30 > 16), below min_range (0.5 < 1), beyond max_range (30 > 25): kept
    up = np.array([10 * math.cos(math.radians(30)), 0, 10 * math.sin(math.radians(30))], F32)
    out.append(Case("not_tested", np.stack([beam(4, 45, 60), beam(7, 45, 60)]), np.stack([up, beam(4, 45, 0.5), beam(4, 45, 30)]),
                    [False, False, False], tested=0, filled=2, window=(4, 8), max_range=25.0))
    out.append(Case("inside_max_range", np.stack([beam(4, 45, 60)]), np.stack([beam(4, 45, 30)]), [True], tested=1, filled=1,
                    window=(0, 0), max_range=30.5))
    # --- two scan points in one pixel: the nearer decides, whichever comes first
    out.append(Case("pixel_min_first", np.stack([beam(5, 20, 10.1), beam(5, 20, 20)]), np.stack([beam(5, 20, 10)]), [False],
                    tested=1, filled=1, window=(0, 0)))
    out.append(Case("pixel_min_last", np.stack([beam(5, 20, 20), beam(5, 20, 10.1)]), np.stack([beam(5, 20, 10)]), [False],
                    tested=1, filled=1, window=(0, 0)))
    out.append(Case("pixel_far_only", np.stack([beam(5, 20, 20), beam(5, 20, 25)]), np.stack([beam(5, 20, 10)]), [True],
                    tested=1, filled=1, window=(0, 0)))
    # --- scan points that take no part: NaN, inf, below min_range, outside the field of view; one valid far return
    junk = _a([np.nan, 1, 1], [np.inf, 0, 0], [0.5, 0, 0], [0, 0, 10], [20, 0, 0])
    out.append(Case("scan_junk", junk, _a([10, 0, 0]), [True], tested=1, filled=1, window=(0, 0)))
    # --- a pose that is not the identity: yaw 90 degrees plus a translation; margins far from the threshold
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = [3.5, -7.25, 0.75]
    out.append(Case("posed", np.stack([beam(3, 60, 20), beam(2, 60, 12), beam(5, 12, 30)]),
                    np.stack([beam(3, 60, 10), beam(3, 60, 11.9), beam(5, 12, 15), beam(5, 12, 29.9), beam(6, 70, 5)]),
                    [True, False, True, False, False], tested=4, filled=3, window=(1, 1), pose=T))
    return out


def to_map_frame(points, pose):
    """Sensor-frame float32 points -> map frame float32 (exact for the axis-aligned poses of the cases up to one rounding)."""
    p = np.asarray(points, np.float64)
    return (p @ np.asarray(pose)[:3, :3].T + np.asarray(pose)[:3, 3]).astype(F32)


def voxels_emptied(stored, keep, voxel=1.0):
    """Voxels (index = coordinates / voxel truncated toward zero) that hold stored points but none of the kept ones."""
    idx = np.trunc(np.asarray(stored, F32) / F32(voxel)).astype(np.int64)
    all_v = {tuple(v) for v in idx.tolist()}
    return len(all_v - {tuple(v) for v in idx[np.asarray(keep, bool)].tolist()})


def sorted_rows(a):
    """Rows in a canonical order (by x, y, z) — for maps whose voxel order differs (dict order on the host)."""
    a = np.asarray(a, np.float64).reshape(-1, 3)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


# ------------------------------------------------------------------------------------------------ the moving-box drive
BOX_SIZE = (4.0, 1.8, 1.6)
BOX_STEP = 1.5          # m per scan along the free lane (|y| < 3 m of scans.make_scene)
SENSOR_STEP = 1.0


def box_bounds(i):
    cx = -8.0 + BOX_STEP * i
    lo = np.array([cx - BOX_SIZE[0] / 2, -BOX_SIZE[1] / 2, -1.7])
    return lo, lo + np.array(BOX_SIZE)


def sensor_pose(i):
    T = np.eye(4)
    T[:3, 3] = [-18.0 + SENSOR_STEP * i, 0.3, 0.0]
    return T


def drive_scans(sc, sensor, n_scans=8, with_box=True, rays=None):
    """-> list of (pose 4x4, scan float32 [n,3] sensor frame).  ``rays``: keep every rays-th ... None = the full grid scan."""
    base = sc.make_scene()
    out = []
    for i in range(n_scans):
        scene = base
        if with_box:
            lo, hi = box_bounds(i)
            scene = sc.Scene(np.vstack([base.boxes_lo, lo]), np.vstack([base.boxes_hi, hi]))
        T = sensor_pose(i)
        out.append((T, sc.lidar_grid_scan(scene, T[:3, :3], T[:3, 3], sensor, stream=700 + i).astype(F32)))
    return out


def in_boxes(points, boxes, pad=0.15):
    """bool [m]: inside any of the boxes (list of indices), padded by ``pad`` (range noise is 0.02 m) — except below: the box
    stands on the ground, and the ground under a box that has moved on is scene, not ghost (0.1 m of the box's foot is given
    up for that)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    m = np.zeros(p.shape[0], bool)
    for i in boxes:
        lo, hi = box_bounds(i)
        m |= np.all((p >= lo + np.array([-pad, -pad, 0.1])) & (p <= hi + pad), axis=1)
    return m
