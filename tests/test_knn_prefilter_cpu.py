"""Option knn_prefilter (valu | mfma) from svnicp_set_option to the scan kernel's launch, without a GPU: the Tuning
field and its default compiled on the host, the parser's two values, the hand-over to the kernel arguments, the launcher's
four instantiations, and the words of INTEGRATION.md."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svn-icp_amd", "csrc")


def _text(*parts):
    return open(os.path.join(ROOT, *parts)).read()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host compiler")
def test_tuning_default_is_the_matrix_pipe(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstdio>\n#include "registration_plan.hpp"\n'
                   'int main() { svnicp::Tuning t; std::printf("%d\\n", t.knn_prefilter_mfma); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().strip() == "1"


def test_parser_takes_valu_and_mfma_only():
    api = _text("svn-icp_amd", "csrc", "api.hip")
    m = re.search(r'k == "knn_prefilter"\)\s*\{([^}]*)\}', api)
    assert m, "svnicp_set_option does not parse knn_prefilter"
    body = m.group(1)
    assert re.search(r'v == "mfma"\)\s*t\.knn_prefilter_mfma = 1', body)
    assert re.search(r'v == "valu"\)\s*t\.knn_prefilter_mfma = 0', body)
    assert "else ok = false" in body
    assert sorted(re.findall(r'v == "(\w+)"', body)) == ["mfma", "valu"]


def test_option_reaches_the_scan_kernel():
    host = _text("svn-icp_amd", "csrc", "stage_a_host.hpp")
    assert "k.prefilter_mfma = e.tune.knn_prefilter_mfma" in host
    assert "k.tile_a = tile_a.p" in host and "k.tile_o = tile_o.p" in host
    tiles = _text("svn-icp_amd", "csrc", "knn_tiles.hip")
    for sw in (4, 8):
        for mf in ("true", "false"):
            assert f"k_knn_scan_tiles<{sw}, {mf}>" in tiles, (sw, mf)
    assert re.search(r"if \(a\.prefilter_mfma\)", tiles)


def test_option_is_documented():
    doc = _text("INTEGRATION.md")
    row = [l for l in doc.splitlines() if l.startswith("| `knn_prefilter`")]
    assert len(row) == 1 and "`valu`" in row[0] and "`mfma`" in row[0]
