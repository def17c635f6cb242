"""Stage A's Morton sort alone: the project's three-pass radix chain against rocPRIM's radix_sort_pairs (option
sort_kernel = merge) and against std::stable_sort by key on the host, through tests/morton_order_driver (spatial_prep.hip
compiled into a program of its own; __graft_entry__.build_morton_order_driver).  A stable sort by key has one answer, so
every comparison is element by element and exact.  The driver runs all cases in one process; the tests read its lines.

The one-cell case also caps the data dependence of the sort's stream time: within 3x of a random cloud of the same size
(16 384 + 4 096 pairs), for both sorts.  Measured on an MI355X, one event pair around the two key kernels and the sort:
radix chain 47.6 us on the random cloud and 38.8 us on one cell; rocPRIM 46.2 us and 44.3 us.
"""
import subprocess

import pytest

pytestmark = pytest.mark.gpu

CASES = ["size_7780_1000", "size_7781_1001", "random_16384_4096", "flagship_262144_131072", "edge_below", "edge_at", "edge_above", "one_cell_16384_4096",
         "two_cells", "grid_duplicates", "nan_rows", "all_nan", "sentinel_queries"]
SHAPES = {"size_7780_1000": (7780, 1000), "size_7781_1001": (7781, 1001), "random_16384_4096": (16384, 4096),
          "edge_below": (16383, 8191), "edge_at": (16384, 8192), "edge_above": (16385, 8193), "one_cell_16384_4096": (16384, 4096)}
# what the crafted clouds must come out as, so that a case cannot quietly stop being what its name says
DISTINCT = {"one_cell_16384_4096": 2, "two_cells": 4, "all_nan": 2, "sentinel_queries": None}


@pytest.fixture(scope="module")
def lines():
    import __graft_entry__ as graft
    exe = graft.build_morton_order_driver()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for l in r.stdout.splitlines():
        t = l.split()
        if t and t[0] == "case":
            out[t[1]] = {t[i]: float(t[i + 1]) for i in range(2, len(t), 2)}
    print(r.stdout)
    return out


@pytest.mark.parametrize("name", CASES)
def test_order_is_the_stable_sort_by_key(lines, name):
    c = lines[name]
    print(name, c)
    if name in SHAPES:
        assert (c["M"], c["n"]) == SHAPES[name]
    assert c["radix_vs_host"] == 0 and c["merge_vs_host"] == 0 and c["radix_vs_merge"] == 0
    assert c["fill"] == 0, "the chunk table words behind the key kernel are not all -1"
    if DISTINCT.get(name) is not None:
        assert c["distinct_keys"] == DISTINCT[name]   # one key per cloud (the queries carry bit 30)
    if name == "grid_duplicates":
        assert c["distinct_keys"] < 0.25 * (c["M"] + c["n"])
    if name == "nan_rows":
        assert c["distinct_keys"] < c["M"] + c["n"]


def test_sentinel_queries_share_the_largest_key(lines):
    c = lines["sentinel_queries"]
    assert c["distinct_keys"] <= c["M"] + 1   # all 2 000 queries in one key


def test_one_cell_costs_what_a_random_cloud_does(lines):
    one, rnd = lines["one_cell_16384_4096"], lines["random_16384_4096"]
    print("radix chain: one cell %.1f us, random %.1f us | rocPRIM: one cell %.1f us, random %.1f us"
          % (one["radix_us"], rnd["radix_us"], one["merge_us"], rnd["merge_us"]))
    assert one["radix_us"] <= 3.0 * rnd["radix_us"]
    assert one["merge_us"] <= 3.0 * rnd["merge_us"]
