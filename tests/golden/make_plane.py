"""tests/golden/make_plane.py — regenerates tests/golden/plane.npz, the fixture of tests/test_plane_alone_{cpu,gpu}.py.

Normal cases (tests/plane_cases.normal_cases), per cluster: the eigenvalues of the exact scatter matrix in mpmath at 60 digits,
each kept as two doubles (hi + lo), and whether the cluster has a normal; per case E_ref = the largest eigen-residual and
Rayleigh excess (plane_mp_reference.criterion) of numpy's eigh on plane_reference.neighbourhood_eig's float64 matrix, taken
over every row of every valid cluster — the yardstick the device is held to.  The matrices themselves are not stored: a
reader forms them in exact rationals from the case module's coordinates.

Accumulate cases (plane_cases.all_cases), per particle that gets mpmath (stage_b_reference.mp_particles): the 29 values of
the record in mpmath and the sum of |term| of each, held as corrections to the float64 restatement
(plane_mp_reference.sums_f64, i.e. plane_reference.record_one), exactly as tests/golden/stage_b.npz holds stage B's sums:

    a_eps [record][29] float32   (v_mp - v_f64) / max(sum|term|_mp, 1e-300): |eps| is the restatement's E
    a_rho [record][29] float32   sum|term|_mp / sum|term|_f64 (1 where both are 0)
    a_yard [case][5]             the largest |eps| per sum group (plane_mp_reference.GROUPS)
    *_chk, a_crc                 checksums of a case's inputs, and of the recomputed float64 values the corrections belong to

No clouds, tables or poses are stored.  The readers need numpy only (the generator: mpmath and the oracle's knn_topk).

Run from the repo root:  python tests/golden/make_plane.py
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (TESTS, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import plane_cases as cases  # noqa: E402
import plane_mp_reference as pm  # noqa: E402
import plane_reference as pr  # noqa: E402

FIXTURE = os.path.join(HERE, "plane.npz")
TINY = pm.TINY


# ------------------------------------------------------------------------------------------------ normals
def restatement_normals(orc, case):
    """(unit normals [M][3] with 0 rows, valid [M]) of plane_reference.normals, and the neighbour lists it searched."""
    n, valid, _ = pr.normals(orc, case.tgt, case.kn)
    return n, valid


def cluster_of(case):
    out = np.zeros(case.M, np.int64)
    for i, c in enumerate(case.clusters):
        out[c.rows] = i
    return out


def generate_normals(orc):
    names, chk, at, lam_all, valid_all, eref = [], [], [0], [], [], []
    for c in cases.normal_cases():
        truth = cases.normal_truth(c)
        n, nv = restatement_normals(orc, c)
        for cl, t in zip(c.clusters, truth):
            if cl.judged:
                assert (nv[cl.rows] == t["valid"]).all(), "%s %s: the restatement's validity differs from the exact one" % (c.name, cl.kind)
        wrong, fig, axes = pm.judge_clusters(c, [t["lam"] for t in truth], [t["valid"] and cl.judged for cl, t in zip(c.clusters, truth)],
                                             np.where(np.array([cl.judged for cl in c.clusters])[cluster_of(c)][:, None], n, 0.0))
        assert not wrong and not axes, (c.name, wrong[:3], axes[:3])
        fig = np.array(list(fig.values()))
        names.append(c.name); chk.append(c.checksum()); at.append(at[-1] + len(truth))
        lam_all += [[pm.split_double(l) if l < 2 ** 1000 and (l == 0 or l > 2.0 ** -900) else (0.0, 0.0) for l in t["lam"]] for t in truth]
        valid_all += [t["valid"] for t in truth]
        eref.append([fig[:, 1].max(), fig[:, 2].max()])
        print("%s: %d clusters, E_ref residual %.3e, rayleigh %.3e, |n|-1 %.3e" % (c.name, len(truth), fig[:, 1].max(), fig[:, 2].max(), fig[:, 0].max()))
    return dict(n_names=np.array(names), n_chk=np.array(chk, np.int64), n_at=np.array(at, np.int32), n_lam=np.array(lam_all, np.float64),
                n_valid=np.array(valid_all, bool), n_eref=np.array(eref, np.float64))


def normal_reference(fix, case):
    """A normal case's reference out of the fixture: chk, lam [cluster][3] Fractions, valid [cluster], eref (residual, rayleigh)."""
    from fractions import Fraction
    i = fix["n_row"][case.name]
    a, b = fix["n_at"][i], fix["n_at"][i + 1]
    lam = [[Fraction(float(hi)) + Fraction(float(lo)) for hi, lo in row] for row in fix["n_lam"][a:b]]
    return dict(chk=int(fix["n_chk"][i]), lam=lam, valid=fix["n_valid"][a:b], eref=tuple(float(x) for x in fix["n_eref"][i]))


# ------------------------------------------------------------------------------------------------ accumulate
def crc_of(s, mag, idx):
    return np.int64(zlib.crc32(np.ascontiguousarray(s[idx]).tobytes() + np.ascontiguousarray(mag[idx]).tobytes()))


def generate_accumulate(only=None):
    names, chk, crc, n, idx_all, eps_all, rho_all, yard = [], [], [], [], [], [], [], []
    for c in cases.all_cases():
        if only and c.name not in only:
            continue
        idx = c.mp_particles()
        s64, m64 = c.f64()
        mp_s, mp_m = pm.sums_mp(c.src, c.tgt, c.nrm, c.cand, c.poses, c.delta, c.discrete(), idx)
        eps = pm.signed_error_f64(s64[idx], mp_s, mp_m)
        rho = np.array([[float(a / float(b)) if b > 0 else 1.0 for a, b in zip(ra, rb)] for ra, rb in zip(mp_m, m64[idx])], np.float32)
        assert all((float(a) == 0.0) == (b == 0.0) for ra, rb in zip(mp_m, m64[idx]) for a, b in zip(ra, rb)), c.name
        names.append(c.name); chk.append(c.checksum()); crc.append(crc_of(s64, m64, idx)); n.append(len(idx))
        idx_all.append(idx); eps_all.append(eps); rho_all.append(rho)
        yard.append([np.abs(eps[:, list(ix)]).max() for _, ix in pm.GROUPS])
        print("%s: %d records, E_f64 %s" % (c.name, len(idx), " ".join("%s %.2e" % (g, y) for (g, _), y in zip(pm.GROUPS, yard[-1]))))
    return dict(a_names=np.array(names), a_chk=np.array(chk, np.int64), a_crc=np.array(crc, np.int64), a_n=np.array(n, np.int32),
                a_idx=np.concatenate(idx_all).astype(np.int16), a_eps=np.concatenate(eps_all), a_rho=np.concatenate(rho_all),
                a_yard=np.array(yard, np.float64))


def load(path=FIXTURE):
    z = np.load(path, allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["a_at"] = np.concatenate([[0], np.cumsum(d["a_n"])])
    d["a_row"] = {str(nm): i for i, nm in enumerate(d["a_names"])}
    d["n_row"] = {str(nm): i for i, nm in enumerate(d["n_names"])}
    return d


def case_reference(fix, case):
    """An accumulate case's reference out of the fixture, joined with the recomputed float64 restatement: chk, crc_ok, idx [n],
    v64 / mag [P][29] (every particle; mag is sum|term| floored at TINY, of mpmath on idx), eps [n][29], yard {group: E_f64}."""
    i = fix["a_row"][case.name]
    a, b = fix["a_at"][i], fix["a_at"][i + 1]
    idx = fix["a_idx"][a:b].astype(np.int64)
    s64, m64 = case.f64()
    mag = m64.copy()
    mag[idx] = m64[idx] * fix["a_rho"][a:b].astype(np.float64)
    return dict(chk=int(fix["a_chk"][i]), crc_ok=int(fix["a_crc"][i]) == int(crc_of(s64, m64, idx)), idx=idx, v64=s64, mag=np.maximum(mag, TINY),
                eps=fix["a_eps"][a:b], yard={g: float(fix["a_yard"][i][j]) for j, (g, _) in enumerate(pm.GROUPS)})


def main():
    import __graft_entry__ as graft
    orc = graft.load_oracle()
    orc.build()
    d = generate_normals(orc)
    d.update(generate_accumulate())
    np.savez_compressed(FIXTURE, **d)
    print("%s: %d normal cases, %d accumulate cases, %d records, %d bytes" % (FIXTURE, len(d["n_names"]), len(d["a_names"]), len(d["a_idx"]),
                                                                              os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    main()
