"""Numpy restatement of svnicp_map_query_normals (include/svnicp_hip.h) — test infrastructure.

Works from the host map ``pipeline.VoxelHashMap._vox`` (voxel index -> float32 points in insertion order), sorted by key:
that is the row order of a whole-map query of the device map.  For the point at row i, in voxel (vx, vy, vz):

    candidates   every point of the voxels (vx+a, vy+b, vz+c), a, b, c in {-1, 0, 1}, that exist (indices outside +-2^20 do
                 not), enumerated in ascending (x, y, z) voxel index, slots of a voxel ascending; the point itself is one
    distance     float64 of the widened float32 coordinates, d2 = ((dx*dx) + dy*dy) + dz*dz
    neighbours   the normal_k candidates smallest by (d2, enumeration order): a stable sort by d2; fewer candidates: no normal
                 (one ranking serves every normal_k: neighbourhoods())
    normal       offsets relative to the point, two-pass mean and scatter matrix in float64, numpy.linalg.eigh, the unit
                 eigenvector of lambda0; valid iff lambda2 > 0 and lambda1 >= MIN_RATIO * lambda2

The device sums in another order and diagonalises by Jacobi sweeps: results agree to rounding, not bit for bit.
"""
import numpy as np

MIN_RATIO = 0.01      # kPlaneMinRatio (csrc/plane_normal_device.hpp)
INDEX_LIMIT = 1 << 20


class MapNormals:
    """keys [V] sorted voxel indices, offs [V + 1] first row of each voxel, points [M,3] float64 rows, normals [M,3] (0 rows
    where there is none), valid [M], lam [M,3] ascending eigenvalues (0 where there were too few candidates), nbr [M, normal_k]
    whole-map row indices of the neighbours in (d2, enumeration) order (-1 where too few), n_cand [M], boundary_tie [M]: the
    normal_k-th and the next candidate are DISTINCT points at the same d2, so the tie rule decides the neighbour set."""


def rows_of(vox, pose=None, max_range=None):
    """Whole-map row indices that a query GetMap(pose, max_range) selects (all rows for pose None), in its output order."""
    keys = sorted(vox)
    offs = np.concatenate([[0], np.cumsum([len(vox[k]) for k in keys])])
    if pose is None:
        return np.arange(offs[-1])
    pos = np.asarray(pose, float)[:3, 3]
    r2 = max_range * max_range
    sel = [np.arange(offs[i], offs[i + 1]) for i, k in enumerate(keys)
           if float(np.sum((np.asarray(vox[k][0]).astype(float) - pos) ** 2)) < r2]
    return np.concatenate(sel) if sel else np.zeros(0, np.int64)


def _pack(k):
    return ((k[:, 0] + INDEX_LIMIT) << 42) | ((k[:, 1] + INDEX_LIMIT) << 21) | (k[:, 2] + INDEX_LIMIT)


class Neighbourhoods:
    """keys, offs, points as in MapNormals; n_cand [M]; order [M, <= K_MAX + 1] whole-map row indices of every point's
    candidates smallest by (d2, enumeration order), -1 past the last candidate; d2 [M, same] their distances (inf there)."""


K_MAX = 64


def neighbourhoods(vox):
    """The candidate enumeration and the (d2, enumeration order) ranking of the definition, for every normal_k at once."""
    keys = sorted(vox)                                       # ascending (x, y, z) voxel index = ascending packed key
    V = len(keys)
    K = np.array(keys, np.int64).reshape(-1, 3)
    cnt = np.array([len(vox[k]) for k in keys], np.int64)
    offs = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    M = int(offs[-1])
    pts = np.concatenate([np.asarray(vox[k], np.float32).reshape(-1, 3) for k in keys], 0).astype(np.float64)
    packed = _pack(K)
    nb = np.full((V, 27), -1, np.int64)                      # the 27 voxels of every block, in enumeration order
    o = 0
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            for c in (-1, 0, 1):
                kk = K + np.array([a, b, c])
                exists = np.all((kk >= -INDEX_LIMIT) & (kk < INDEX_LIMIT), axis=1)
                pk = _pack(kk)
                j = np.minimum(np.searchsorted(packed, pk), V - 1)
                nb[:, o] = np.where(exists & (packed[j] == pk), j, -1)
                o += 1
    c_nb = np.where(nb >= 0, cnt[np.maximum(nb, 0)], 0)
    start = np.cumsum(c_nb, axis=1) - c_nb
    n_cand_v = c_nb.sum(axis=1)
    width = int(n_cand_v.max())
    cand = np.full((V, width), -1, np.int64)                 # candidate rows of a voxel's points, enumeration order
    for o in range(27):
        for s in range(int(c_nb[:, o].max())):               # slots of a voxel ascending
            m = np.flatnonzero(c_nb[:, o] > s)
            cand[m, start[m, o] + s] = offs[nb[m, o]] + s
    vox_of = np.repeat(np.arange(V), cnt)
    keep = min(K_MAX + 1, width)
    out = Neighbourhoods()
    out.keys, out.offs, out.points, out.n_cand = keys, offs, pts, n_cand_v[vox_of]
    out.order = np.full((M, keep), -1, np.int64)
    out.d2 = np.full((M, keep), np.inf)
    step = max(1, 2_000_000 // width)
    for lo in range(0, M, step):
        hi = min(M, lo + step)
        c = cand[vox_of[lo:hi]]
        pad = c < 0
        q, p = pts[np.where(pad, 0, c)], pts[lo:hi]
        dx, dy, dz = q[:, :, 0] - p[:, None, 0], q[:, :, 1] - p[:, None, 1], q[:, :, 2] - p[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d2[pad] = np.inf
        idx = np.argsort(d2, axis=1, kind="stable")[:, :keep]            # (d2, enumeration order)
        out.order[lo:hi] = np.take_along_axis(c, idx, axis=1)
        out.d2[lo:hi] = np.take_along_axis(d2, idx, axis=1)
    return out


def map_normals(vox, normal_k, nbh=None):
    """nbh: neighbourhoods(vox), when the caller keeps it for several normal_k."""
    if not 1 <= normal_k <= K_MAX:
        raise ValueError("normal_k")
    nbh = nbh or neighbourhoods(vox)
    pts, M = nbh.points, nbh.points.shape[0]
    enough = nbh.n_cand >= normal_k                          # fewer candidates: no normal
    have = nbh.order.shape[1]
    nbr = np.full((M, normal_k), -1, np.int64)
    nbr[:, :min(have, normal_k)] = nbh.order[:, :normal_k]
    nbr[~enough] = -1
    sel = np.where(enough[:, None], nbr, 0)
    off = pts[sel] - pts[:, None, :]                         # offsets relative to the point
    mean = off.sum(axis=1) / normal_k
    cen = off - mean[:, None, :]
    cov = np.einsum("pki,pkj->pij", cen, cen)
    cov[~enough] = 0.0
    lam, vec = np.linalg.eigh(cov)
    out = MapNormals()
    out.keys, out.offs, out.points, out.nbr, out.n_cand = nbh.keys, nbh.offs, pts, nbr, nbh.n_cand
    out.boundary_tie = np.zeros(M, bool)
    if have > normal_k:
        last, nxt = nbh.order[:, normal_k - 1], nbh.order[:, normal_k]
        out.boundary_tie = (nxt >= 0) & (nbh.d2[:, normal_k - 1] == nbh.d2[:, normal_k]) & np.any(pts[last] != pts[np.maximum(nxt, 0)], axis=1)
    out.lam = np.where(enough[:, None], lam, 0.0)
    out.valid = enough & (lam[:, 2] > 0.0) & (lam[:, 1] >= MIN_RATIO * lam[:, 2])
    n = vec[:, :, 0].copy()
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[~out.valid] = 0.0
    out.normals = n
    return out
