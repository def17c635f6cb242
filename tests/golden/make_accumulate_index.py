"""tests/golden/make_accumulate_index.py — records tests/golden/accumulate_index/accumulate_index.npz on a GPU: for every case of
tests/accumulate_index_cases.py the 22 sums per particle behind each iteration's accumulate launch and the final
particles, with the default stage B (accum = split) in the general chain, and the final particles of the default chain.
The file pins the accumulate kernel's bits as they were when the test was added; the test compares bit for bit.  Inputs
are not stored (numpy default_rng, seeds in the case list).

    python tests/golden/make_accumulate_index.py [--root CHECKOUT] [--out FILE]

--root: the checkout whose built library records (default: this one).
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import accumulate_index_cases as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(TESTS))
    ap.add_argument("--out", default=os.path.join(HERE, "accumulate_index", "accumulate_index.npz"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("graft_entry_of_root", os.path.join(os.path.abspath(a.root), "__graft_entry__.py"))
    graft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(graft)
    pkg = graft.load_package()
    out = {}
    for c in cases.CASES:
        sums, particles, _ = cases.run(pkg, c, "split")
        out[c.name + "/sums"], out[c.name + "/particles"] = sums, particles
        out[c.name + "/particles_default_chain"] = cases.run(pkg, c, "split", chain="auto")[1]
        print(c.name, "sums", sums.shape, "finite", bool(np.isfinite(sums).all()), "Σw of particle 0:", sums[:, 0, 0])
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
