"""The accumulate kernel's winner gather and block ends (stein_split_device.hpp: accumulate_body), pinned bit for bit: the
clamp of the winner's target index, the row address formed from it, and the selects of a point past the block in a block's
last trip are integers, addresses and products with exactly 0.0 or 1.0 — whatever is done to them (DESIGN §4.2 records a
32-bit clamp and a peeled last trip that were measured and not kept) may not move a sum by a bit.

Whole registrations (tests/accumulate_index_cases.py: 12 particles so that the split stage B runs, K = 100, no early stop;
one case with 70 particles for the 64-particle waves of the flagship) at source sizes around one trip and around
pts_per_block, winners at target 0 and M - 1, one SVGD case and one with the trace on, so that every instantiation of the
shared body runs.  Each is compared
  * with the kept float64 reference kernel (option accum = f64) under the tolerances test_gpu_parity.py holds this pair
    of kernels to (test_stage_b_f32_search_is_bit_identical_to_f64_kernel: raw sums rtol 1e-12 / atol 1e-9, particles 1e-9);
  * bit for bit with tests/golden/accumulate_index/accumulate_index.npz, recorded on an MI355X (tests/golden/make_accumulate_index.py).
"""
import os

import numpy as np
import pytest

import accumulate_index_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "accumulate_index", "accumulate_index.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_sums_and_particles_keep_their_bits(hip, golden, name):
    case = cases.BY_NAME[name]
    sums, particles, corr = cases.run(hip, case, "split")
    # the reference kernel; for the crafted winners it also records who won
    ref_case = case._replace(trace=True) if case.ends else case
    rsums, rparticles, rcorr = cases.run(hip, ref_case, "f64")
    assert np.isfinite(sums).all() and np.isfinite(particles).all()
    assert sums[:, :, 0].min() > 0.0 or case.B == 1, "no pair was accepted: the case does not exercise the sums"
    if case.ends:
        assert set(np.unique(rcorr)) == {0, cases.M - 1}, "the winners are not the two ends of the index range"
    if case.trace:
        assert np.array_equal(corr, rcorr)
    print(name, "max |split - f64| sums %.3g particles %.3g" % (np.abs(sums - rsums).max(), np.abs(particles - rparticles).max()))
    np.testing.assert_allclose(sums, rsums, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(particles, rparticles, rtol=0, atol=1e-9)
    gs, gp = golden[name + "/sums"], golden[name + "/particles"]
    assert gs.shape == sums.shape and gp.shape == particles.shape
    assert np.array_equal(sums.view(np.int64), gs.view(np.int64)), "a sum differs from the recorded bits"
    assert np.array_equal(particles.view(np.int64), gp.view(np.int64)), "a particle differs from the recorded bits"
    # the default chain of these sizes: fewer, longer blocks
    pd = cases.run(hip, case, "split", chain="auto")[1]
    assert np.array_equal(pd.view(np.int64), golden[name + "/particles_default_chain"].view(np.int64)), "default chain: a particle differs"
