"""tests/golden/make_gicp.py — regenerates tests/golden/gicp/gicp.npz, the fixture of tests/test_gicp_alone_gpu.py.

Per case of tests/gicp_cases.all_cases that is not `exact`, per particle that gets mpmath (stage_b_reference.mp_particles): the
29 values of the record in mpmath at 60 digits and the yardstick mag = sum of cond(S_pair) |term| of each
(tests/gicp_mp_reference.py), held as corrections to the float64 restatement (gicp_mp_reference.sums_f64, i.e.
gicp_reference.record_one), exactly as tests/golden/plane.npz holds plane mode's sums:

    a_eps [record][29] float32   (v_mp - v_f64) / max(mag_mp, 1e-300): |eps| is the restatement's E
    a_rho [record][29] float32   mag_mp / mag_f64 (1 where both are 0)
    a_yard [case][5]             the largest |eps| per sum group (plane_mp_reference.GROUPS)
    a_chk, a_crc                 checksums of a case's inputs, and of the recomputed float64 values the corrections belong to

No clouds, tables or poses are stored.  The readers need numpy only (the generator: mpmath).

Run from the repo root:  python tests/golden/make_gicp.py
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

import gicp_cases as cases  # noqa: E402
import gicp_mp_reference as gm  # noqa: E402
import plane_mp_reference as pm  # noqa: E402

FIXTURE = os.path.join(HERE, "gicp", "gicp.npz")   # a directory of its own: helpers.golden_cases takes every *.npz beside the generators for a whole-registration vector
TINY = gm.TINY


def crc_of(s, mag, idx):
    return np.int64(zlib.crc32(np.ascontiguousarray(s[idx]).tobytes() + np.ascontiguousarray(mag[idx]).tobytes()))


def generate():
    names, chk, crc, n, idx_all, eps_all, rho_all, yard = [], [], [], [], [], [], [], []
    for c in cases.all_cases():
        if "exact" in c.tags:
            continue
        idx = c.mp_particles()
        s64, m64 = gm.sums_f64(c)
        mp_s, mp_m = gm.sums_mp(c, idx)
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
    return d


def case_reference(fix, case):
    """A case's reference out of the fixture, joined with the recomputed float64 restatement: chk, crc_ok, idx [n], v64 / mag
    [P][29] (every particle; mag is floored at TINY, of mpmath on idx), eps [n][29], yard {group: E_f64}."""
    i = fix["a_row"][case.name]
    a, b = fix["a_at"][i], fix["a_at"][i + 1]
    idx = fix["a_idx"][a:b].astype(np.int64)
    s64, m64 = gm.sums_f64(case)
    mag = m64.copy()
    mag[idx] = m64[idx] * fix["a_rho"][a:b].astype(np.float64)
    return dict(chk=int(fix["a_chk"][i]), crc_ok=int(fix["a_crc"][i]) == int(crc_of(s64, m64, idx)), idx=idx, v64=s64, mag=np.maximum(mag, TINY),
                eps=fix["a_eps"][a:b], yard={g: float(fix["a_yard"][i][j]) for j, (g, _) in enumerate(pm.GROUPS)})


def main():
    d = generate()
    np.savez_compressed(FIXTURE, **d)
    print("%s: %d cases, %d records, %d bytes" % (FIXTURE, len(d["a_names"]), len(d["a_idx"]), os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    main()
