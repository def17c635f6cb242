"""tests/golden/make_knn_ref.py — regenerates tests/golden/knn_ref/knn_cpu_ref.npz.

The file holds the inputs and outputs of the reference's own float32 KNearestNeighborIdxCpu (oracle/_ref, built by
`make -C oracle ref` where the reference tree is present) for the KNN cases of tests/test_oracle_cpu.py, so that those
tests pin the oracle to the reference on machines without it.  Where oracle/_ref is built the tests also call it live
and require these very outputs.

Run from the repo root:  python tests/golden/make_knn_ref.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "knn_ref", "knn_cpu_ref.npz")

# integer-grid clouds: every distance is exact in float32 and float64 and massively tied
TIES = [(40, 300, 1), (64, 500, 7), (33, 257, 32), (16, 150, 100), (5, 3, 4)]


def grid_cloud(n, seed, span=6):
    rng = np.random.default_rng(seed)
    return rng.integers(-span, span + 1, size=(n, 3)).astype(np.float64)


def main():
    orc = graft.load_oracle()
    orc.build()
    if not orc.ref_available():
        raise SystemExit("oracle/_ref is not built: the reference tree is needed to regenerate these vectors")
    cases = [(f"ties_{B}_{M}_{K}", grid_cloud(B, 1), grid_cloud(M, 2), K) for B, M, K in TIES]
    rng = np.random.default_rng(3)
    q = rng.normal(size=(50, 3)).astype(np.float32)
    t = rng.normal(size=(700, 3)).astype(np.float32)
    cases.append(("random", q, t, 20))
    out = {}
    for name, q, t, K in cases:
        idx, d2 = orc.ref_knn_cpu_f32(q, t, K)
        out.update({f"{name}_q": q, f"{name}_t": t, f"{name}_k": np.int64(K), f"{name}_idx": idx, f"{name}_d2": d2})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(cases)} cases")


if __name__ == "__main__":
    main()
