"""Static register budget of the Stein-step kernels on the default path (no GPU needed).

The device pieces of the Stein step are stated once in stein_step_device.hpp and inlined into every launch shape; the
kernels a default registration launches per iteration must not pay for that sharing.  This test cross-compiles the
Stein-step translation units for gfx950 with the Makefile's flags and bounds, per kernel, the vector registers and the
scratch bytes by what the hand-copied code had before the pieces were shared (VGPRs / scratch bytes below).  It also
keeps generic addressing out: a pointer that may be LDS or global inside a shared function must still resolve to
ds_* / global_* after inlining, so no kernel that issued no flat_load / flat_store then may issue one now.
"""
import os
import re
import shutil
import subprocess

import pytest

from test_search_isa_budget import CSRC, HIPCC, _makefile_flags

UNITS = ("particle_update.hip", "reduce_partials.hip")

# kernel: (next_free_vgpr, private_segment_fixed_size) before the device pieces were shared
BUDGET = {
    "k_upd_prepare": (134, 0),
    "k_upd_prepare_median": (228, 8),
    "k_upd_direction": (239, 0),
    "k_upd_finish": (16, 0),
    "k_upd_hist": (35, 0),
    "k_upd_collect": (62, 0),
    "k_upd_select": (34, 0),
    "k_reduce_partials": (32, 0),
}
# kernels of these units that issued flat_load / flat_store before (k_particle_update reads H through a pointer that is LDS
# or global by a launch-time flag); every other kernel must stay free of them
FLAT_BEFORE = {"k_particle_update"}


def kernels(asm):
    """{kernel name: (next_free_vgpr, private_segment_fixed_size, flat loads and stores in its body)} of an assembly file."""
    lines = asm.splitlines()
    flat, cur = {}, None
    for l in lines:
        m = re.match(r"^(_Z\w+):", l)
        if m:
            cur = m.group(1)
            flat[cur] = 0
        elif l.startswith(".Lfunc_end"):
            cur = None
        elif cur and re.match(r"\s+flat_(load|store)", l):
            flat[cur] += 1
    out, cur = {}, None
    for l in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            cur, meta = m.group(1), {}
        m = re.match(r"\s+\.amdhsa_(next_free_vgpr|private_segment_fixed_size)\s+(\d+)", l)
        if m and cur:
            meta[m.group(1)] = int(m.group(2))
        if ".end_amdhsa_kernel" in l and cur:
            name = re.match(r"_ZN6svnicp12_GLOBAL__N_1(\d+)", cur)
            short = cur[name.end():name.end() + int(name.group(1))] if name else cur
            out[short] = (meta["next_free_vgpr"], meta["private_segment_fixed_size"], flat.get(cur, 0))
            cur = None
    return out


@pytest.fixture(scope="module")
def step_kernels(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("isa_step")
    found = {}
    for unit in UNITS:
        out = tmp / (unit + ".s")
        subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, unit), "-o", str(out)],
                       check=True, cwd=str(tmp), capture_output=True)
        found.update(kernels(out.read_text()))
    return found


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_default_path_kernel_register_budget(step_kernels, kernel):
    vgpr, scratch, _ = step_kernels[kernel]
    print(f"{kernel}: {vgpr} VGPRs, {scratch} B scratch (budget {BUDGET[kernel]})")
    assert vgpr <= BUDGET[kernel][0], f"{kernel} needs {vgpr} VGPRs (budget {BUDGET[kernel][0]})"
    assert scratch <= BUDGET[kernel][1], f"{kernel} uses {scratch} B of scratch (budget {BUDGET[kernel][1]})"


def test_no_new_flat_addressing(step_kernels):
    assert set(BUDGET) <= set(step_kernels)
    now = {k for k, (_, _, flat) in step_kernels.items() if flat}
    assert now <= FLAT_BEFORE, f"generic (flat) loads or stores appeared in {sorted(now - FLAT_BEFORE)}"
