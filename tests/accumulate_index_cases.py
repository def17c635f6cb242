"""Cases of tests/test_accumulate_index_gpu.py and tests/golden/make_accumulate_index.py: whole registrations through the split
stage B (more than 8 particles, K = 100, no early stop) at source sizes around the accumulate kernel's trips, and the
runner both share.  Inputs come from numpy's default_rng with the seed in the case; only outputs are stored.

With 12 particles the accumulate kernel runs 16 particles per wave: a wave step holds BW = 4 points, a workgroup's four
waves STEP = 16, and one loop trip U * STEP = 64 points (stein_split_device.hpp: accumulate_body).  With 70 particles
(64 per wave, two waves along the particles — the instantiation the flagship runs) STEP = 2 and a trip is 8 points.
"""
from collections import namedtuple

import numpy as np

K, ITERS, M = 100, 3, 600
STEP, TRIP = 16, 64

Case = namedtuple("Case", "name P B seed svgd trace ends")
CASES = [
    Case("tail_only_b1", 12, 1, 1, False, False, False),                 # every block has only the tail trip
    Case("one_trip", 12, 4 * STEP, 2, False, False, False),              # one full trip, no tail
    Case("ragged_tail", 12, 4 * STEP * 2 + 1, 3, False, False, False),   # full trips and a tail of one point
    Case("size_257", 12, 257, 4, False, False, False),                   # around pts_per_block
    Case("size_1000", 12, 1000, 5, False, False, False),
    Case("size_4099", 12, 4099, 6, False, False, False),
    Case("index_ends", 12, 300, 7, False, False, True),                  # every winner is target 0 or target M - 1
    Case("svgd", 12, 1000, 8, True, False, False),                       # the SVGD count in place of one sum
    Case("trace", 12, 1000, 9, False, True, False),                      # not PLAIN: winner byte -> candidate row, trace written
    Case("p70_size_1000", 70, 1000, 10, False, False, False),            # 64 particles per wave, two waves along the particles
]
BY_NAME = {c.name: c for c in CASES}


def inputs(case):
    """src [B][3], tgt [M][3], init [6][P]"""
    g = np.random.default_rng(1000 + case.seed)
    if case.ends:
        # two clusters of source points 0.2 m wide, target 0 in the middle of one and target M - 1 of the other; every other
        # target at least 5 m from both, so that it is a candidate (K = 100) and never the winner
        ca, cb = np.array([2.0, 1.0, 0.5]), np.array([-3.0, 2.0, 1.0])
        src = np.where((np.arange(case.B) % 2 == 0)[:, None], ca, cb) + g.uniform(-0.1, 0.1, (case.B, 3))
        tgt = g.uniform(-30.0, 30.0, (M, 3))
        far = np.minimum(np.linalg.norm(tgt - ca, axis=1), np.linalg.norm(tgt - cb, axis=1)) < 5.0
        tgt[far] += np.array([0.0, 0.0, 40.0])
        tgt[0], tgt[M - 1] = ca, cb
        scale = 0.01
    else:
        tgt = g.uniform(-6.0, 6.0, (M, 3))
        src = tgt[g.integers(0, M, case.B)] + g.normal(0.0, 0.05, (case.B, 3))
        scale = 0.02
    init = g.normal(0.0, scale, (6, case.P))
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt), np.ascontiguousarray(init)


def run(pkg, case, accum, chain="general"):
    """The registration of `case` with option accum: (sums [ITERS][P][22] behind each iteration's accumulate, particles [6][P],
    the winners' target indices [ITERS][P][B] or None without the trace).  chain = general: k_reduce_partials leaves the
    sums where they can be read; chain = auto is the default, the small chain at these sizes (at most 32 accumulate workgroups,
    so more points per block; nothing reduces their records, and the sums returned are zeros)."""
    import torch
    from svnicp_amd.sharded import _DevView
    L = pkg.load_library()
    src, tgt, init = inputs(case)
    prm = pkg.SteinICPParam(iterations=ITERS, lr=1.0, max_dist=1.0, KNN_count=K, check_early_stop=False, record_trace=case.trace)
    if case.svgd:
        prm.optimizer = "Adam"
    s = (pkg.SVGDICP if case.svgd else pkg.SVNICP)(prm, init)
    s.add_cloud(src, tgt, init)
    s.set_option("accum", accum)
    s.set_option("chain", chain)
    s._check(L.svnicp_align_begin(s.handle), "svnicp_align_begin")
    s._check(L.svnicp_stage_candidates(s.handle, 0, case.B), "svnicp_stage_candidates")
    s._check(L.svnicp_build_candidate_table(s.handle), "svnicp_build_candidate_table")
    sums = np.zeros((ITERS, case.P, 22))
    for it in range(ITERS):
        s._check(L.svnicp_iter_accumulate(s.handle, it), "svnicp_iter_accumulate")
        s.synchronize()
        ptr = L.svnicp_sums_devptr(s.handle)
        assert ptr
        if chain == "general":
            sums[it] = torch.as_tensor(_DevView(ptr, (case.P, 22), "<f8"), device="cuda").cpu().numpy()
        s._check(L.svnicp_iter_update(s.handle, it), "svnicp_iter_update")
    s._check(L.svnicp_finish(s.handle), "svnicp_finish")
    s.synchronize()
    particles = np.array(s.get_particles(), np.float64)
    corr = None
    if case.trace:   # the trace holds the winner's position in the point's candidate row: [ITERS][P][B] target indices from it
        pos = s.get_trace()["corr"].astype(np.int64)
        cand = np.asarray(s.get_candidates(), np.int64).reshape(case.B, K)
        corr = np.where(pos >= 0, cand[np.arange(case.B)[None, None, :], np.clip(pos, 0, K - 1)], -1)
    s.close()
    return sums, particles, corr
