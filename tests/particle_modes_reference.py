"""numpy float64 restatement of include/svnicp_hip.h "particle modes": the link rule, union-find over the finite particles,
and every per-mode sum in ascending particle order.  Every product and every sum is written out one operation at a time on
Python floats (IEEE double, one rounding per operation), so nothing can be fused or re-associated.

Also: ``closure_labels``, an independent second statement of the modes (the boolean link matrix closed by repeated
squaring) that tests/test_particle_modes_cpu.py holds the union-find against, and ``bounds``, the rounding bound of each
reported sum computed from its own terms."""
import numpy as np

MODES_MAX = 32


def _sq3(a, b, c):
    return ((a * a) + b * b) + c * c


def linked(xp, xq, lt2, lr2):
    """xp, xq: six Python floats each."""
    dt2 = _sq3(xp[0] - xq[0], xp[1] - xq[1], xp[2] - xq[2])
    dr2 = _sq3(xp[3] - xq[3], xp[4] - xq[4], xp[5] - xq[5])
    return dt2 <= lt2 and dr2 <= lr2


def link_matrix(x, link_trans, link_rot):
    """[P, P] bool, vectorised: the same unfused expressions elementwise (numpy rounds every ufunc once)."""
    x = np.asarray(x, np.float64).reshape(6, -1)
    lt2, lr2 = np.float64(link_trans) * np.float64(link_trans), np.float64(link_rot) * np.float64(link_rot)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x[:, :, None] - x[:, None, :]
        dt2 = ((d[0] * d[0]) + d[1] * d[1]) + d[2] * d[2]
        dr2 = ((d[3] * d[3]) + d[4] * d[4]) + d[5] * d[5]
        A = (dt2 <= lt2) & (dr2 <= lr2)
    fin = np.isfinite(x).all(axis=0)
    return A & fin[:, None] & fin[None, :], fin


def union_find_labels(x, link_trans, link_rot):
    """label[p] = lowest particle index of p's component, -1 for a non-finite particle."""
    A, fin = link_matrix(x, link_trans, link_rot)
    P = A.shape[0]
    parent = list(range(P))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for p, q in zip(*np.nonzero(np.triu(A, 1))):
        a, b = find(int(p)), find(int(q))
        if a != b:
            parent[max(a, b)] = min(a, b)      # the lower index stays the root
    return np.array([find(p) if fin[p] else -1 for p in range(P)], np.int64)


def closure_labels(x, link_trans, link_rot):
    """The second statement: reachability = the link matrix (with the diagonal) squared until it stops growing; the label
    of p is the first particle it reaches."""
    A, fin = link_matrix(x, link_trans, link_rot)
    R = A | np.diag(fin)
    while True:
        R2 = (R.astype(np.float32) @ R.astype(np.float32)) > 0
        if np.array_equal(R2, R):
            break
        R = R2
    return np.array([int(np.argmax(R[p])) if fin[p] else -1 for p in range(R.shape[0])], np.int64)


def modes(x, link_trans, link_rot, max_modes=8, weights=None, cost=None):
    """Returns a dict with the fields of struct svnicp_modes (n_reported entries per array), ``labels`` (per particle: rank
    of its mode, -1 non-finite) and ``terms`` for ``bounds``."""
    x = np.asarray(x, np.float64).reshape(6, -1)
    P = x.shape[1]
    w = [1.0] * P if weights is None else [float(v) for v in np.asarray(weights, np.float64).reshape(-1)]
    root = union_find_labels(x, link_trans, link_rot)
    roots = sorted(set(int(r) for r in root if r >= 0))
    members = {r: [p for p in range(P) if root[p] == r] for r in roots}
    W = {}
    for r in roots:
        s = 0.0
        for p in members[r]:
            s = s + w[p]
        W[r] = s
    W_all = 0.0
    for p in range(P):
        if root[p] >= 0:
            W_all = W_all + w[p]
    order = sorted(roots, key=lambda r: (-W[r], r))
    rank = {r: k for k, r in enumerate(order)}
    n = min(len(order), max_modes)
    out = dict(particles=P, nonfinite=int((root < 0).sum()), n_modes=len(order), n_reported=n, has_scores=cost is not None,
               label=np.array(order[:n], np.int32), count=np.array([len(members[r]) for r in order[:n]], np.int32),
               best=np.full(n, -1, np.int32), mass=np.zeros(n), cost_min=np.zeros(n), cost_mean=np.zeros(n),
               mean=np.zeros((n, 6)), cov=np.zeros((n, 6, 6)),
               labels=np.array([rank[int(r)] if r >= 0 else -1 for r in root], np.int32),
               terms=dict(mass=np.zeros(n), mean=np.zeros((n, 6)), cov=np.zeros((n, 6, 6))))
    xs = x.tolist()
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, r in enumerate(order[:n]):
            mem, Wk = members[r], np.float64(W[r])
            out["mass"][k] = Wk / np.float64(W_all)
            out["terms"]["mass"][k] = sum(abs(w[p]) for p in mem)
            for i in range(6):
                s, sa = 0.0, 0.0
                for p in mem:
                    t = w[p] * xs[i][p]
                    s = s + t
                    sa += abs(t)
                out["mean"][k, i] = np.float64(s) / Wk
                out["terms"]["mean"][k, i] = sa
            m = [float(v) for v in out["mean"][k]]
            for a in range(6):
                for b in range(6):
                    s, sa = 0.0, 0.0
                    for p in mem:
                        t = w[p] * ((xs[a][p] - m[a]) * (xs[b][p] - m[b]))
                        s = s + t
                        sa += abs(t)
                    out["cov"][k, a, b] = np.float64(s) / Wk
                    out["terms"]["cov"][k, a, b] = sa
            if cost is not None:
                c = [float(v) for v in np.asarray(cost, np.float64).reshape(-1)]
                best, cmin, s = mem[0], c[mem[0]], 0.0
                for p in mem:
                    s = s + c[p]
                    if c[p] < cmin:
                        best, cmin = p, c[p]
                out["best"][k], out["cost_min"][k], out["cost_mean"][k] = best, cmin, np.float64(s) / np.float64(len(mem))
    return out


def bounds(ref):
    """Rounding bound of each reported figure: count * 2^-52 * sum |terms| of its own sum, divided by W as the figure is
    (mass: by W_all; its terms are the weights).  With the sums added in the same order on both sides the difference is
    expected to be 0; this is what may be tolerated."""
    eps = 2.0 ** -52
    n = ref["n_reported"]
    cnt = ref["count"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        W = ref["terms"]["mass"]                                   # = sum |w| = W for weights >= 0
        mass = cnt * eps * ref["mass"] if n else np.zeros(0)
        mean = cnt[:, None] * eps * ref["terms"]["mean"] / W[:, None]
        cov = cnt[:, None, None] * eps * ref["terms"]["cov"] / W[:, None, None]
    return mass, mean, cov
