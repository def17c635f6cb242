"""Static instruction budget of the headline search kernel (no GPU needed).

k_stein_search_bf16<64, 2, 6, true> is the C3 search: 55 % of a registration, bound by vector instruction issue
(DESIGN.md §4.2).  Its time falls only when one (source point, 64-particle group) step issues fewer instructions, so
this test cross-compiles stein_split.hip for gfx950 with the Makefile's flags into a temporary directory, finds the
group loop of that instantiation (the innermost loop whose body holds the step's 24 MFMAs) and bounds the vector
instructions issued by one trip of it.  Blocks of loops nested inside it (the exact pass a full queue falls back to)
are not counted.  The budgets are the counts the code has now, so a change that adds work to the step fails here
first.  The same assembly also holds the plain accumulate kernels, which stand one or two registers below the four-wave
limit: their kernel descriptors are read for that limit.
"""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svn-icp_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SYM = "_ZN6svnicp12_GLOBAL__N_119k_stein_search_bf16ILi64ELi2ELi6ELb1EEEvNS_9AccumArgsE"

VECTOR_BUDGET = 372   # v_*, ds_*, global_* per group step (396 before the plane layout of the tile rows, the 32-bit offsets,
                      # the tile-index tags, the mask-free B split and the branch-free decision)
MOV_BUDGET = 13       # v_mov_b32 (25 before)
VGPR_BUDGET = 128     # four waves per SIMD: 512 VGPRs / 4
ACCUM_SYM = "_ZN6svnicp12_GLOBAL__N_120k_stein_accumulate_wILi64ELi%dELb1ELb%dEEEvNS_9AccumArgsE"   # <64, WP, true, SVGD>


def _makefile_flags():
    with open(os.path.join(CSRC, "Makefile")) as f:
        text = f.read()
    line = next(l for l in text.splitlines() if l.startswith("CXXFLAGS"))
    flags = line.split("=", 1)[1].split()
    return [x.replace("$(ARCH)", "gfx950") for x in flags if x != "-fPIC"]


def group_loop(asm, sym=SYM):
    """(instruction counts of one trip of the group loop, kernel descriptor fields) of kernel `sym` in `asm`."""
    lines = asm.splitlines()
    s = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
    e = next(i for i in range(s, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[s:e]
    labels, depth = {}, {}
    for i, l in enumerate(body):   # a block's loop depth, from the compiler's comments on its label line and the lines after
        m = re.match(r"^(\.LBB\w+):", l)
        if m:
            labels[m.group(1)] = i
            d, n = 0, i
            while n < len(body) and (n == i or body[n].lstrip().startswith(";")):
                for x in re.findall(r"(?:Header: |Header=\S+ )Depth=(\d+)", body[n]):
                    d = max(d, int(x))
                n += 1
            depth[i] = d
    best = None   # the shortest back edge whose loop holds the 24 MFMAs of a group step
    for j, l in enumerate(body):
        m = re.match(r"\s+s_(?:cbranch_\w+|branch)\s+(\.LBB\w+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < j:
            i = labels[m.group(1)]
            if sum("v_mfma" in x for x in body[i:j + 1]) >= 24 and (best is None or j - i < best[1] - best[0]):
                best = (i, j)
    assert best is not None, "no loop with the group step's 24 MFMAs"
    i, j = best
    cnt, cur = collections.Counter(), depth[i]
    for n in range(i, j + 1):
        if n in depth:
            cur = depth[n]
            continue
        st = body[n].strip()
        if st and not st.startswith((";", ".")) and cur <= depth[i]:
            cnt[st.split()[0]] += 1
    return cnt, kernel_descriptor(asm, sym)


def kernel_descriptor(asm, sym):
    """next_free_vgpr and group_segment_fixed_size of kernel `sym`, from its .amdhsa_kernel block in `asm`."""
    lines = asm.splitlines()
    meta = {}
    k = next(n for n in range(len(lines)) if lines[n].split() == [".amdhsa_kernel", sym])
    for l in lines[k:]:
        m = re.match(r"\s+\.amdhsa_(next_free_vgpr|group_segment_fixed_size)\s+(\d+)", l)
        if m:
            meta[m.group(1)] = int(m.group(2))
        if ".end_amdhsa_kernel" in l:
            break
    return meta


@pytest.fixture(scope="module")
def search_asm(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "stein_split.s"
    subprocess.run([HIPCC, *_makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, "stein_split.hip"),
                    "-o", str(out)], check=True, cwd=str(out.parent), capture_output=True)
    return out.read_text()


def test_group_step_vector_instruction_budget(search_asm):
    cnt, meta = group_loop(search_asm)
    vec = sum(v for k, v in cnt.items() if k.startswith(("v_", "ds_", "global_", "buffer_", "flat_")))
    assert sum(v for k, v in cnt.items() if k.startswith("v_mfma")) == 24
    assert vec <= VECTOR_BUDGET, f"group step issues {vec} vector instructions (budget {VECTOR_BUDGET}): {dict(cnt)}"
    movs = sum(v for k, v in cnt.items() if k.startswith("v_mov"))
    assert movs <= MOV_BUDGET, f"{movs} register copies in the group step (budget {MOV_BUDGET})"


def test_search_kernel_keeps_four_waves_per_simd(search_asm):
    _, meta = group_loop(search_asm)
    assert meta["next_free_vgpr"] <= VGPR_BUDGET
    assert 4 * meta["group_segment_fixed_size"] <= 160 * 1024   # four workgroups per CU in LDS


@pytest.mark.parametrize("svgd", [False, True])
@pytest.mark.parametrize("WP", [1, 2, 4])
def test_accumulate_kernel_keeps_four_waves_per_simd(search_asm, WP, svgd):
    """The plain accumulate kernels of 64-particle waves sit at the occupancy cliff (127, 127, 126 VGPRs in SVN mode, 120 in
    SVGD mode): one register more than 128 and a SIMD holds three waves of them, not four."""
    meta = kernel_descriptor(search_asm, ACCUM_SYM % (WP, int(svgd)))
    assert meta["next_free_vgpr"] <= VGPR_BUDGET, meta
