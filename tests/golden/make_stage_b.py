"""tests/golden/make_stage_b.py — regenerates tests/golden/stage_b.npz.

For every case of tests/stage_b_cases.all_cases() and every particle that gets mpmath (stage_b_reference.mp_particles): the
22 sums in mpmath at 60 digits and the sum of |term| of each, held as corrections to the plain float64 restatement
(stage_b_reference.sums_f64), which every reader recomputes from the case module in numpy:

    eps [record][22]  float32   (v_mp - v_f64) / max(sum|term|_mp, 1e-300), formed in mpmath: the mpmath sum is
                                v_f64 + eps * sum|term|_mp to 1e-7 of the float64 rounding error, and |eps| IS the float64
                                restatement's E, the yardstick of tests/test_stage_b_gpu.py
    rho [record][22]  float32   sum|term|_mp / sum|term|_f64 (1 where both are 0)
    yard [case][5]              the largest |eps| of the case per sum group (stage_b_reference.GROUPS)
    chk, crc [case]             checksum of the case's inputs; checksum of the recomputed float64 sums the corrections belong to

Held this way the file is a third of the size of the sums themselves (it must stay below svn_p64_k100.npz), and the sums
keep 60 digits where a double would round them to the very accuracy under test.  Clouds, tables and poses are not stored.
The readers need numpy only.

Run from the repo root:  python tests/golden/make_stage_b.py
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import stage_b_cases as cases  # noqa: E402
import stage_b_reference as ref  # noqa: E402

FIXTURE = os.path.join(HERE, "stage_b.npz")
TINY = 1e-300


def f64_sums(case):
    """(sums, sum|term|) [P][22] of the float64 restatement for every particle of the case."""
    return ref.sums_f64(case.src, case.discrete(), case.max_dist, case.svgd)


def crc_of(s, mag, idx):
    return np.int64(zlib.crc32(np.ascontiguousarray(s[idx]).tobytes() + np.ascontiguousarray(mag[idx]).tobytes()))


def generate(only=None):
    names, chk, crc, n, idx_all, eps_all, rho_all, yard = [], [], [], [], [], [], [], []
    for c in cases.all_cases():
        if only and c.name not in only:
            continue
        idx = c.mp_particles()
        s64, m64 = f64_sums(c)
        mp_s, mp_m = ref.sums_mp(c.src, c.discrete(), c.max_dist, idx, c.svgd)
        eps = ref.signed_error_f64(s64[idx], mp_s, mp_m)
        rho = np.array([[float(a / float(b)) if b > 0 else 1.0 for a, b in zip(ra, rb)] for ra, rb in zip(mp_m, m64[idx])], np.float32)
        assert all((float(a) == 0.0) == (b == 0.0) for ra, rb in zip(mp_m, m64[idx]) for a, b in zip(ra, rb)), c.name
        names.append(c.name); chk.append(c.checksum()); crc.append(crc_of(s64, m64, idx)); n.append(len(idx))
        idx_all.append(idx); eps_all.append(eps); rho_all.append(rho)
        yard.append([np.abs(eps[:, list(ix)]).max() for _, ix in ref.GROUPS])
    return dict(names=np.array(names), chk=np.array(chk, np.int64), crc=np.array(crc, np.int64), n=np.array(n, np.int32),
                idx=np.concatenate(idx_all).astype(np.int16), eps=np.concatenate(eps_all), rho=np.concatenate(rho_all),
                yard=np.array(yard, np.float64))


def load(path=FIXTURE):
    z = np.load(path, allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["at"] = np.concatenate([[0], np.cumsum(d["n"])])
    d["row"] = {str(nm): i for i, nm in enumerate(d["names"])}
    return d


def case_reference(fix, case):
    """A case's reference out of the fixture, joined with the recomputed float64 restatement:
    chk, crc_ok, idx [n], v64 / mag [P][22] (every particle; mag is sum|term| floored at TINY, of mpmath on idx), eps [n][22],
    yard {group: E_f64}."""
    i = fix["row"][case.name]
    a, b = fix["at"][i], fix["at"][i + 1]
    idx = fix["idx"][a:b].astype(np.int64)
    s64, m64 = f64_sums(case)
    mag = m64.copy()
    mag[idx] = m64[idx] * fix["rho"][a:b].astype(np.float64)
    return dict(chk=int(fix["chk"][i]), crc_ok=int(fix["crc"][i]) == int(crc_of(s64, m64, idx)), idx=idx, v64=s64, mag=np.maximum(mag, TINY),
                eps=fix["eps"][a:b], yard={g: float(fix["yard"][i][j]) for j, (g, _) in enumerate(ref.GROUPS)})


def main():
    d = generate()
    np.savez_compressed(FIXTURE, **d)
    print("%s: %d cases, %d records, %d bytes" % (FIXTURE, len(d["names"]), len(d["idx"]), os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    main()
