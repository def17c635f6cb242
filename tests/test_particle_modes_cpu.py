"""Particle modes (include/svnicp_hip.h "particle modes"), the part that needs no GPU: the numpy
restatement (tests/particle_modes_reference.py) against an independent second statement and against numpy's own weighted
statistics on every crafted set (tests/particle_modes_cases.py), the two-basin scene on the CPU oracle with the margins
that tests/test_particle_modes_gpu.py relies on, the ABI declarations and mirrors, and the refusals that need no device."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

import particle_modes_cases as pc
import particle_modes_reference as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = pc.crafted()


def _ref(c, **kw):
    return pm.modes(c["x"], c["link_trans"], c["link_rot"], c["max_modes"], c["weights"], **kw)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_reference_against_the_closure_and_numpy_statistics(c):
    x, w = c["x"], c["weights"]
    root = pm.union_find_labels(x, c["link_trans"], c["link_rot"])
    assert np.array_equal(root, pm.closure_labels(x, c["link_trans"], c["link_rot"]))
    r = _ref(c)
    e = c["expect"]
    assert r["n_modes"] == e["n_modes"] and r["n_reported"] == min(e["n_modes"], c["max_modes"])
    assert r["nonfinite"] == e.get("nonfinite", 0) and (r["labels"] < 0).sum() == r["nonfinite"]
    assert sorted(r["count"].tolist(), reverse=True) == sorted(e["counts"], reverse=True)
    if w is None:
        assert r["count"].tolist() == e["counts"]                 # equal weights: mass order is count order, ties by label
    if "labels_first" in e:
        assert r["label"][0] == e["labels_first"]
    ww = np.ones(x.shape[1]) if w is None else w
    fin = root >= 0
    mass = np.array([ww[root == l].sum() for l in r["label"]])
    assert (np.diff(mass) <= 0).all()                            # descending W …
    all_roots = np.unique(root[fin])
    assert r["labels"].max() == r["n_modes"] - 1 and np.unique(r["labels"][fin]).size == all_roots.size   # … and every mode ranked
    for k, l in enumerate(r["label"]):
        mem = root == l
        assert mem[l] and not mem[:l].any() and (r["labels"][mem] == k).all() and r["count"][k] == mem.sum()
        assert np.isclose(r["mass"][k], mass[k] / ww[fin].sum(), rtol=1e-12, atol=0)
        scale = np.abs(x[:, mem]).max() + 1e-300
        assert np.abs(r["mean"][k] - np.average(x[:, mem], axis=1, weights=ww[mem])).max() <= 1e-12 * scale
        if mem.sum() > 1:
            cov = np.cov(x[:, mem], aweights=ww[mem], ddof=0)
            assert np.abs(r["cov"][k] - cov).max() <= 1e-12 * np.abs(cov).max(), c["name"]   # relative to the matrix
        else:
            assert not r["cov"][k].any()


def test_scores_and_truncation_of_the_reference():
    c = next(c for c in CASES if c["name"] == "mass_not_count")
    cost = np.array([0.3, 0.1, 0.1, 0.25, 0.5])
    r = _ref(c, cost=cost)
    assert r["has_scores"] and r["label"].tolist() == [3, 0] and r["best"].tolist() == [3, 1]       # the tie 1 / 2 goes to 1
    assert r["cost_min"].tolist() == [0.25, 0.1] and r["cost_mean"].tolist() == [(0.25 + 0.5) / 2.0, ((0.3 + 0.1) + 0.1) / 3.0]
    assert _ref(c)["best"].tolist() == [-1, -1] and not _ref(c)["cost_min"].any()
    forty = next(c for c in CASES if c["name"] == "forty_singletons")
    r = _ref(forty)
    assert r["n_modes"] == 40 and r["n_reported"] == 4 and r["labels"].tolist() == list(range(40))
    edge = {c["name"]: _ref(c)["n_modes"] for c in CASES if c["name"].startswith("edge")}
    assert edge["edge_linked"] == 1 and edge["edge_not_linked"] == 2


# ------------------------------------------------------------------------------------------------ the two-basin scene
def test_two_basin_scene_on_the_oracle(pkg, orc):
    """A corridor along x (walls at y = +-1 m, a floor, flat posts that reach 0.4 m in from both walls) whose posts repeat
    every 3.0 m over x in [-30, 34]; the source is the stretch [-3, 3] of the same structure, displaced by 0.1 m.  B = 1024,
    M = 4096, P = 16: eight particles start within +-0.2 m of x = 0, eight within +-0.2 m of x = 3.0.  K = 384, three
    iterations, lr 1, max_dist 1.

    Final parameters against the sketch of the issue (posts every 2.0 m): the period is 3.0 m, because two clusters of any
    width whose centres are one period = 4 links = 2.0 m apart cannot keep every inter-mode pair 4 links apart; the posts
    are flat in x, because round posts sampled this sparsely leave point-to-point ICP no gradient along the corridor; and K is
    384, because stage A searches once at the initial mean and K = 256 does not reach the next post.  Measured on the
    oracle: closest inter-mode pair 5.47 links, farthest nearest neighbour of a mode 0.245 links (the bounds: 4 and 0.5)."""
    src, tgt, init = pc.two_basin(pkg)
    assert src.shape == (pc.BASIN_B, 3) and tgt.shape == (pc.BASIN_M, 3) and init.shape == (6, pc.BASIN_P)
    assert (np.abs(init[0, :8]) <= pc.BASIN_SPREAD).all() and (np.abs(init[0, 8:] - pc.POST_PERIOD) <= pc.BASIN_SPREAD).all()
    o = orc.Solver(init, iterations=pc.BASIN_I, lr=pc.BASIN_LR, max_dist=pc.BASIN_MAX_DIST, knn_count=pc.BASIN_K, svn_full_grad=False)
    o.add_cloud(src, tgt, init)
    o.stein_align()
    x = np.asarray(o.get_particles(), np.float64).reshape(6, -1)
    r = pm.modes(x, pc.LINK_T, pc.LINK_R)
    assert r["n_modes"] == 2 and r["count"].tolist() == [8, 8] and r["label"].tolist() == [0, 8]
    assert r["labels"].tolist() == [0] * 8 + [1] * 8
    inter, near = pc.margins(x, r["labels"])
    print(f"two-basin on the oracle: closest inter-mode pair {inter:.3f} links, farthest nearest same-mode neighbour {near:.3f} links; "
          f"mode means x = {r['mean'][:, 0]}")
    assert inter >= 4.0 and near <= 0.5
    # both groups moved towards their basin: the correction that registers the source is 0.1 (+ one period)
    x0 = init[0]
    assert abs(x[0, :8].mean() - pc.BASIN_OFFSET) < abs(x0[:8].mean() - pc.BASIN_OFFSET)
    assert abs(x[0, 8:].mean() - pc.BASIN_OFFSET - pc.POST_PERIOD) < abs(x0[8:].mean() - pc.BASIN_OFFSET - pc.POST_PERIOD)
    # the global mean lies between the modes, where no particle is
    assert np.abs(x[0] - x[0].mean()).min() > 1.0


# ------------------------------------------------------------------------------------------------ ABI, mirrors, refusals
def test_abi_declares_and_exports_the_modes_entry_points(pkg):
    names = pkg.declared_symbols()
    L = pkg.load_library()
    for n in ("svnicp_particle_modes", "svnicp_get_mode_labels"):
        assert n in names and hasattr(L, n), n
    b = pkg.binding
    assert L.svnicp_particle_modes.argtypes == [C.c_void_p, C.POINTER(b.ModesOptStruct), C.POINTER(b.ModesStruct)]
    assert L.svnicp_get_mode_labels.argtypes == [C.c_void_p, C.POINTER(C.c_int32)]
    hdr = open(os.path.join(ROOT, "include", "svnicp_hip.h")).read()
    assert re.search(r"#define\s+SVNICP_MODES_MAX\s+32\b", hdr) and re.search(r"#define\s+SVNICP_ABI_VERSION\s+1\b", hdr)
    assert b.MODES_MAX == 32 and pkg.abi_version() == 1
    # the C layout: 6 int32, three int32 arrays, then doubles; the options: 2 int32, 2 doubles, pointer, int32 + pad, pointer
    n = b.MODES_MAX
    assert C.sizeof(b.ModesStruct) == 24 + 3 * 4 * n + 8 * n * (3 + 6 + 36 + 9 + 3) and b.ModesStruct.mass.offset == 24 + 12 * n
    assert C.sizeof(b.ModesOptStruct) == 48 and b.ModesOptStruct.weightsP.offset == 40
    # a NULL context is refused, not dereferenced
    assert L.svnicp_particle_modes(None, None, None) == -1 and L.svnicp_get_mode_labels(None, None) == -1


def test_host_mirrors_carry_the_modes(pkg):
    assert [f.name for f in dataclasses.fields(pkg.ParticleModes)] == [
        "particles", "nonfinite", "n_modes", "n_reported", "has_scores", "label", "count", "best", "mass", "cost_min", "cost_mean", "mean", "cov", "pose"]
    assert callable(pkg.SVNICP.particle_modes) and callable(pkg.SVGDICP.get_mode_labels)
    cfg = pkg.pipeline.PipelineConfig()
    assert cfg.mode_link is None and cfg.mode_select == "mean" and cfg.mode_max == 8
    assert "modes" in [f.name for f in dataclasses.fields(pkg.pipeline.ScanResult)]
    for bad in (dict(mode_select="heaviest"), dict(mode_select="best", mode_link=(0.5, 0.05)), dict(mode_link=(0.5,)), dict(mode_link=(-0.5, 0.05)),
                dict(mode_link=(0.5, float("nan"))), dict(mode_link=(float("inf"), 0.05)), dict(mode_link=(0.5, 0.05), mode_max=0),
                dict(mode_link=(0.5, 0.05), mode_max=33)):
        with pytest.raises(ValueError):
            pkg.pipeline.PipelineConfig(**bad)
    ok = pkg.pipeline.PipelineConfig(mode_link=(0.5, 0.05), mode_select="heaviest")
    assert tuple(ok.mode_link) == (0.5, 0.05)
    shim = open(os.path.join(ROOT, "svn-icp_amd", "host", "svnicp_hip_shim.hpp")).read()
    for needle in ("particle_modes", "get_mode_labels", "svnicp_modes_opt"):
        assert needle in shim, needle
    host = open(os.path.join(ROOT, "svn-icp_amd", "host", "registration_pipeline.hpp")).read()
    for needle in ("mode_link_trans", "mode_link_rot", "mode_select_heaviest", "modes"):
        assert needle in host, needle
