"""The clouds, poses and gates the evaluate tests share (tests/test_evaluate_cpu.py checks the preconditions of the cases
tests/test_evaluate_gpu.py compares exactly)."""
import numpy as np

CLOUDS = ("random", "pair", "ragged")
GATES = (0.3, 1.0)
RANDOM_OFFSET = (0.05, -0.03, 0.02, 0.004, -0.003, 0.006)     # scans.random_clouds' default displacement


def clouds(pkg, name):
    """(source [B,3], target [M,3], {"identity", "true_pose"} -> 4x4)."""
    c2p = pkg.pipeline.correction_to_pose
    if name == "random":
        src, tgt = pkg.scans.random_clouds(2048, 8192, seed=3)
        true = c2p(RANDOM_OFFSET)
    elif name == "ragged":
        src, tgt = pkg.scans.random_clouds(1001, 3000, seed=5)
        true = c2p(RANDOM_OFFSET)
    elif name == "pair":
        p = pkg.scans.make_pair(2048, 8192)
        src, tgt, true = p.source, p.target, c2p(p.true_pose)
    else:
        raise ValueError(name)
    return src, tgt, {"identity": np.eye(4), "true_pose": true}
