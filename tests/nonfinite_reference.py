"""The contract for non-finite and huge cloud points (include/svnicp_hip.h under svnicp_set_clouds), in plain
numpy float64 — no device, no oracle.

The oracle cannot be the reference where a squared distance is NaN: its KNN mirrors the reference's heap, which inserts while
size < K whatever the distance, so a NaN among the first K targets sits at the heap's root and blocks every later insertion
(tests/test_nonfinite_cpu.py pins those divergences).  Everywhere else the two agree bit for bit.
"""
import numpy as np

KINDS = ("nan1", "nan3", "+inf", "-inf", "big32", "big64")
NAN_KINDS = ("nan1", "nan3")
NUMBER_KINDS = ("+inf", "-inf", "big32", "big64")      # their d² against a finite point is a number (+inf included)


def dist2(q, tgt):
    """d² = ((dx·dx) + dy·dy) + dz·dz, every product and sum rounded on its own (no contraction), [len(q), len(tgt)]."""
    q, tgt = np.asarray(q, np.float64), np.asarray(tgt, np.float64)
    with np.errstate(all="ignore"):
        dx = q[:, None, 0] - tgt[None, :, 0]
        d = dx * dx
        dy = q[:, None, 1] - tgt[None, :, 1]
        d = d + dy * dy
        dz = q[:, None, 2] - tgt[None, :, 2]
        d = d + dz * dz
    return d


def knn_contract(queries, tgt, K, rows=256):
    """Stage A: per query the K smallest (d², index) among the targets whose d² is not NaN (+inf is a number); positions
    past the number of eligible targets hold index 0 and d² = 0.0.  Returns int64 [B, K] and float64 [B, K]."""
    queries, tgt = np.asarray(queries, np.float64).reshape(-1, 3), np.asarray(tgt, np.float64).reshape(-1, 3)
    B, M = queries.shape[0], tgt.shape[0]
    idx = np.zeros((B, K), np.int64)
    d2 = np.zeros((B, K), np.float64)
    for r0 in range(0, B, rows):
        d = dist2(queries[r0:r0 + rows], tgt)
        order = np.argsort(d, axis=1, kind="stable")[:, :K]          # stable: ties by index; NaN sorts behind +inf
        ds = np.take_along_axis(d, order, axis=1)
        ok = ~np.isnan(ds)
        n = min(K, M)
        idx[r0:r0 + rows, :n] = np.where(ok, order, 0)
        d2[r0:r0 + rows, :n] = np.where(ok, ds, 0.0)
    return idx, d2


def nearest_of_k(Ts, tgt, cand):
    """The per-iteration search: Ts [..., B, 3] transformed source rows, cand [B, K] target indices.  Strict `<` from
    candidate 0 — a NaN first distance is never replaced, an all-NaN row keeps candidate 0.  Returns the position in the
    K list (int64 [..., B]) and its squared distance (float64 [..., B])."""
    Ts, tgt, cand = np.asarray(Ts, np.float64), np.asarray(tgt, np.float64), np.asarray(cand)
    K = cand.shape[1]
    best = np.zeros(Ts.shape[:-1], np.int64)
    bd = None
    with np.errstate(all="ignore"):
        for k in range(K):
            c = tgt[cand[:, k]]
            dx = Ts[..., 0] - c[:, 0]
            d = dx * dx
            dy = Ts[..., 1] - c[:, 1]
            d = d + dy * dy
            dz = Ts[..., 2] - c[:, 2]
            d = d + dz * dz
            if k == 0:
                bd = d
                continue
            take = d < bd
            best = np.where(take, k, best)
            bd = np.where(take, d, bd)
    return best, bd


def bad_row(kind, base):
    """One poisoned copy of the finite row `base`."""
    r = np.array(base, np.float64)
    if kind == "nan1":
        r[1] = np.nan
    elif kind == "nan3":
        r[:] = np.nan
    elif kind == "+inf":
        r[0] = np.inf
    elif kind == "-inf":
        r[2] = -np.inf
    elif kind == "big32":            # finite in float32, squares overflow float32
        r[0] = 1e20
        r[2] = -3e38
    elif kind == "big64":            # its square overflows float64
        r[1] = 1e160
    else:
        raise ValueError(kind)
    return r


def poison(cloud, rows, kind):
    """A copy of `cloud` with `rows` made bad; kind is one of KINDS, or a sequence of kinds cycled over the rows."""
    out = np.array(cloud, np.float64)
    kinds = (kind,) if isinstance(kind, str) else tuple(kind)
    for n, r in enumerate(rows):
        out[r] = bad_row(kinds[n % len(kinds)], out[r])
    return out


def remove_rows(cloud, rows):
    """`cloud` without `rows`, and the monotone old -> new index map (-1 for a removed row)."""
    cloud = np.asarray(cloud)
    keep = np.ones(cloud.shape[0], bool)
    keep[np.asarray(list(rows), np.int64)] = False
    old_to_new = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)
    return cloud[keep].copy(), old_to_new
