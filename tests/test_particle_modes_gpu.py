"""Particle modes on the device (csrc/particle_modes.hip) against tests/particle_modes_reference.py, the
numpy restatement of include/svnicp_hip.h "particle modes".

Tolerances.  Everything that is an integer is compared exactly: n_modes, n_reported, nonfinite, the labels, and per mode
label, count, best and the order.  mass, mean and cov are the same unfused float64 expressions added in the same order on
both sides; what is tolerated is the rounding bound of each figure's own sum, count * 2^-52 * sum |terms| (divided by W as the
figure is), computed from the restatement's terms (particle_modes_reference.bounds).  The largest difference met is
printed; it is expected to be 0.  A mode's total pose against svnicp_evaluate(NULL, NULL)'s: 2^-23 relative, the size of
float32(1 / P) * P - 1 by which the global mean and a normalised mean may differ."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import particle_modes_cases as pc
import particle_modes_reference as pm

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
CASES = pc.crafted()
WIDE = (10.0, 10.0)
_STATE = {}


def _bare(hip):
    """A context with no clouds and no registration: caller-supplied sets need nothing else."""
    if "bare" not in _STATE:
        _STATE["bare"] = hip.SVNICP(hip.SteinICPParam(iterations=1), np.zeros((6, 1)))
    return _STATE["bare"]


def _err(s):
    return s._L.svnicp_last_error(s.handle).decode()


def _compare(got, labels, ref, what):
    """got: ParticleModes, labels: get_mode_labels(); ref: particle_modes_reference.modes."""
    assert (got.particles, got.nonfinite, got.n_modes, got.n_reported) == (ref["particles"], ref["nonfinite"], ref["n_modes"], ref["n_reported"]), what
    assert got.has_scores == ref["has_scores"], what
    assert np.array_equal(labels, ref["labels"]), what
    assert np.array_equal(got.label, ref["label"]) and np.array_equal(got.count, ref["count"]) and np.array_equal(got.best, ref["best"]), what
    b_mass, b_mean, b_cov = pm.bounds(ref)
    d_mass, d_mean, d_cov = np.abs(got.mass - ref["mass"]), np.abs(got.mean - ref["mean"]), np.abs(got.cov - ref["cov"])
    worst = max([float(d.max()) for d in (d_mass, d_mean, d_cov) if d.size] + [0.0])
    _STATE["worst"] = max(_STATE.get("worst", 0.0), worst)
    print(f"{what}: modes {got.n_modes} reported {got.n_reported} counts {got.count[:4].tolist()} | max |device - restatement| over mass, mean, cov = {worst:.3e}")
    assert (d_mass <= b_mass).all() and (d_mean <= b_mean).all() and (d_cov <= b_cov).all(), what
    if ref["has_scores"]:
        assert np.array_equal(got.cost_min, ref["cost_min"]), what                       # a member's own cost
        assert (np.abs(got.cost_mean - ref["cost_mean"]) <= ref["count"] * 2.0 ** -52 * np.abs(ref["cost_mean"])).all(), what
    else:
        assert not got.cost_min.any() and not got.cost_mean.any() and (got.best == -1).all(), what


def _from_registration(s, link, max_modes=8, scores=None):
    """Cluster the last registration's set and compare with the restatement on the device's own particles and weights."""
    got = s.particle_modes(link[0], link[1], max_modes)
    ref = pm.modes(s.get_particles(), link[0], link[1], max_modes, s.get_particle_weight(), cost=scores)
    return got, s.get_mode_labels(), ref


# ------------------------------------------------------------------------------------------------ 1. crafted sets
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_crafted_sets_agree_with_the_restatement(hip, c):
    s = _bare(hip)
    got = s.particle_modes(c["link_trans"], c["link_rot"], c["max_modes"], particles=c["x"], weights=c["weights"])
    labels = s.get_mode_labels()
    ref = pm.modes(c["x"], c["link_trans"], c["link_rot"], c["max_modes"], c["weights"])
    _compare(got, labels, ref, c["name"])
    assert got.n_modes == c["expect"]["n_modes"] and got.nonfinite == c["expect"].get("nonfinite", 0)
    assert not got.has_scores
    # the total pose of a mode: the initial mean (identity here) times the correction its mean is
    for k in range(got.n_reported):
        if np.isfinite(got.mean[k]).all():
            assert np.allclose(got.pose[k], hip.pipeline.correction_to_pose(got.mean[k]), rtol=0, atol=1e-12 * max(1.0, np.abs(got.mean[k]).max()))
    again = s.particle_modes(c["link_trans"], c["link_rot"], c["max_modes"], particles=c["x"], weights=c["weights"])
    for f in ("label", "count", "best", "mass", "mean", "cov", "pose"):
        assert getattr(again, f).tobytes() == getattr(got, f).tobytes(), f               # twice: the same bits
    assert np.array_equal(s.get_mode_labels(), labels)


# ------------------------------------------------------------------------------------------------ 2. registrations
def _solver(hip, src, tgt, init, iterations=4, K=16, svgd=False, weight=None, **kw):
    prm = hip.SteinICPParam(iterations=iterations, lr=0.01 if svgd else 1.0, max_dist=1.0, KNN_count=K, SVN_full_grad=False, **kw)
    s = hip.SVGDICP(prm, init) if svgd else hip.SVNICP(prm, init, weight or hip.ParticleWeightOpt())
    s.add_cloud(src, tgt, init)
    return s


def _pair(hip):
    if "pair" not in _STATE:
        p = hip.scans.make_pair(2048, 4096)
        _STATE["pair"] = (p.source, p.target, hip.scans.make_particles(16))
    return _STATE["pair"]


def test_wide_links_give_one_mode_and_zero_links_every_particle(hip):
    src, tgt, init = _pair(hip)
    T0 = hip.pipeline.correction_to_pose((0.01, -0.02, 0.005, 0.001, 0.002, -0.001))
    s = _solver(hip, src, tgt, init)
    s.set_initial_mean(T0)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    got, labels, ref = _from_registration(s, WIDE)
    _compare(got, labels, ref, "make_pair, wide links")
    assert got.n_modes == 1 and got.count.tolist() == [16] and got.label.tolist() == [0] and got.mass.tolist() == [1.0] and not got.has_scores
    ev = s.evaluate(0.5)                                       # svnicp_evaluate(NULL, NULL): the global mean's total pose
    rel = np.abs(got.pose[0] - ev.pose).max() / max(1.0, np.abs(ev.pose).max())
    print(f"mode pose against evaluate(NULL, NULL): {rel:.3e} relative (bound 2^-23 = {2.0 ** -23:.3e})")
    assert rel <= 2.0 ** -23
    x = s.get_particles().reshape(6, -1)
    distinct = np.unique(x.T, axis=0).shape[0]
    got, labels, ref = _from_registration(s, (0.0, 0.0), max_modes=32)
    _compare(got, labels, ref, "make_pair, zero links")
    assert got.n_modes == distinct and got.n_reported == min(distinct, 32)


def _basin(hip, weight=None):
    src, tgt, init = pc.two_basin(hip)
    s = hip.SVNICP(pc.two_basin_params(hip), init, weight or hip.ParticleWeightOpt())
    s.add_cloud(src, tgt, init)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    return s


def test_two_basin_scene_on_the_device(hip):
    s = _basin(hip)
    got, labels, ref = _from_registration(s, (pc.LINK_T, pc.LINK_R))
    _compare(got, labels, ref, "two-basin")
    assert got.n_modes == 2 and got.count.tolist() == [8, 8] and got.label.tolist() == [0, 8] and labels.tolist() == [0] * 8 + [1] * 8
    inter, near = pc.margins(s.get_particles(), labels)
    print(f"two-basin on the device: closest inter-mode pair {inter:.3f} links, farthest nearest same-mode neighbour {near:.3f} links")
    assert inter >= 4.0 and near <= 0.5
    assert not got.has_scores                                  # no weighting, no scoring yet
    assert abs(got.mean[1, 0] - got.mean[0, 0] - pc.POST_PERIOD) < 0.2
    # every per-pose tool can be pointed at a mode: both evaluate far better than the mean between them
    fit = [s.evaluate(0.3, pose=got.pose[k]).fitness for k in range(2)]
    print(f"fitness at the modes {fit}, at the global mean {s.evaluate(0.3).fitness}")
    assert min(fit) > s.evaluate(0.3).fitness
    # a scoring by hand supplies the scores
    sc = s.score_particles(0.5)
    got, labels, ref = _from_registration(s, (pc.LINK_T, pc.LINK_R), scores=sc.cost)
    _compare(got, labels, ref, "two-basin, scored by hand")
    assert got.has_scores and (got.best >= 0).all()
    # … which a new registration outdates
    s.add_cloud(*pc.two_basin(hip))
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    assert not s.particle_modes(pc.LINK_T, pc.LINK_R).has_scores
    _STATE["basin_particles"] = s.get_particles().reshape(6, -1).copy()


def test_two_basin_scene_with_softmin_weights(hip):
    s = _basin(hip, hip.ParticleWeightOpt(True, 0.5, 1e-3))
    w = s.get_particle_weight()
    assert np.unique(w).size > 1 and abs(w.sum() - 1.0) <= 1e-12   # not the uniform weights in disguise
    sc = s.get_particle_scores()                               # the registration's own scoring
    got, labels, ref = _from_registration(s, (pc.LINK_T, pc.LINK_R), scores=sc.cost)
    _compare(got, labels, ref, "two-basin, soft-min weights")
    assert got.has_scores and got.n_modes == 2 and sorted(got.count.tolist()) == [8, 8]
    assert abs(got.mass.sum() - 1.0) <= 1e-12 and got.mass[0] >= got.mass[1]
    for k in range(2):
        mem = np.nonzero(labels == k)[0]
        assert got.best[k] == mem[np.argmin(sc.cost[mem])] and got.cost_min[k] == sc.cost[mem].min()


@pytest.mark.parametrize("kind", ["svgd", "plane", "minibatch", "row_shard"])
def test_the_call_works_after_every_kind_of_registration(hip, kind):
    src, tgt, init = _pair(hip)
    if kind == "row_shard":
        import torch
        from svnicp_amd.sharded import _DevView, shard_range
        L, W, I, P, B = hip.load_library(), 2, 3, init.shape[1], src.shape[0]
        ranks = []
        for r in range(W):
            lo, hi = shard_range(B, W, r)
            s = _solver(hip, np.ascontiguousarray(src[lo:hi]), tgt, init, iterations=I)
            assert L.svnicp_set_row_shard(s.handle, r, W, B) == 0 and L.svnicp_align_begin(s.handle) == 0, _err(s)
            assert L.svnicp_stage_candidates(s.handle, 0, hi - lo) == 0 and L.svnicp_build_candidate_table(s.handle) == 0, _err(s)
            ranks.append(s)
        views = [torch.as_tensor(_DevView(L.svnicp_rank_sums_devptr(s.handle), (W, P, 22), "<f8"), device="cuda") for s in ranks]
        for it in range(I):
            for s in ranks:
                assert L.svnicp_iter_accumulate(s.handle, it) == 0 and L.svnicp_synchronize(s.handle) == 0
            views[1][0].copy_(views[0][0]); views[0][1].copy_(views[1][1])
            torch.cuda.synchronize()
            for s in ranks:
                assert L.svnicp_iter_update(s.handle, it) == 0
        out = []
        for s in ranks:
            assert L.svnicp_finish(s.handle) == 0 and L.svnicp_synchronize(s.handle) == 0
            got, labels, ref = _from_registration(s, (0.05, 0.002), max_modes=32)
            _compare(got, labels, ref, "row shard")
            out.append((got, labels))
        assert out[0][0].mean.tobytes() == out[1][0].mean.tobytes() and np.array_equal(out[0][1], out[1][1])   # the replicas agree
        return
    kw = dict(svgd=dict(svgd=True), plane=dict(residual="plane"), minibatch=dict(use_minibatch=True, batch_size=256, minibatch_seed=5))[kind]
    s = _solver(hip, src, tgt, init, **kw)
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
    for link in (WIDE, (0.05, 0.002)):
        got, labels, ref = _from_registration(s, link, max_modes=32)
        _compare(got, labels, ref, f"{kind} links {link}")
    assert got.n_modes >= 1 and got.count.sum() <= 16


# ------------------------------------------------------------------------------------------------ 3. side effects
def _snapshot(s):
    d = dict(transformation=s.get_transformation(), distribution=s.get_distribution(), cov=s.get_cov_matrix(),
             particles=s.get_particles(), weights=s.get_particle_weight(), history=s.get_particle_history(),
             candidates=s.get_candidates(), cand_d2=s.get_candidate_dist2(), fallbacks=np.array(s.get_knn_fallbacks()),
             ambiguous=np.array(s.get_ambiguous_pairs()), iterations=np.array(s.get_iterations_run()))
    for k, v in s.get_trace().items():
        d["trace_" + k] = v
    return d


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_the_call_changes_nothing(hip):
    src, tgt, init = _pair(hip)

    def again(s):
        s.add_cloud(src, tgt, init)
        assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS
        return _snapshot(s)

    f = _solver(hip, src, tgt, init, record_trace=True)          # the context that never asks
    s = _solver(hip, src, tgt, init, record_trace=True)
    fresh, before = again(f), again(s)
    _same(fresh, before)
    one = s.particle_modes(0.05, 0.002, 32)
    lab = s.get_mode_labels()
    _same(before, _snapshot(s))                                  # every getter returns what it returned before
    s.particle_modes(1.0, 1.0, 1, particles=pc.chain(65))       # a caller's set in between …
    assert s.get_mode_labels().shape == (65,)
    _same(before, _snapshot(s))
    two = s.particle_modes(0.05, 0.002, 32)                     # … and the same call again: the same bits
    for name in ("label", "count", "best", "mass", "mean", "cov", "pose"):
        assert getattr(one, name).tobytes() == getattr(two, name).tobytes(), name
    assert np.array_equal(s.get_mode_labels(), lab)
    _same(again(f), again(s))                                    # the next registration is that of the untouched context


# ------------------------------------------------------------------------------------------------ 4. refusals
def _raw(s, max_modes=8, link_trans=0.5, link_rot=0.05, x=None, P=None, w=None, opt_size=None, out_size=None):
    import sys
    binding = sys.modules[type(s).__module__.rsplit(".", 1)[0]].binding
    b = (s._L, binding)
    opt, out = binding.ModesOptStruct(), binding.ModesStruct()
    opt.struct_size = C.sizeof(opt) if opt_size is None else opt_size
    out.struct_size = C.sizeof(out) if out_size is None else out_size
    opt.max_modes, opt.link_trans, opt.link_rot = max_modes, link_trans, link_rot
    dp = C.POINTER(C.c_double)
    if x is not None:
        opt.particles6xP, opt.P = x.ctypes.data_as(dp), (x.shape[1] if P is None else P)
    if w is not None:
        opt.weightsP = w.ctypes.data_as(dp)
    return b[0].svnicp_particle_modes(s.handle, C.byref(opt), C.byref(out))


def test_refusals(hip):
    src, tgt, init = _pair(hip)
    s = _solver(hip, src, tgt, init)
    x, w = np.ascontiguousarray(pc.chain(65)), np.ones(65)
    lab = np.zeros(65, np.int32)
    assert s._L.svnicp_get_mode_labels(s.handle, lab.ctypes.data_as(C.POINTER(C.c_int32))) == ERR_INVALID and "no svnicp_particle_modes yet" in _err(s)
    assert _raw(s) == ERR_INVALID and "no finished registration" in _err(s)          # before any registration, without a set
    assert _raw(s, x=x) == 0, _err(s)                                                 # … a caller's set needs none
    for kw, needle in ((dict(opt_size=40), "svnicp_modes_opt.struct_size"), (dict(out_size=8), "svnicp_modes.struct_size"),
                       (dict(max_modes=0), "max_modes"), (dict(max_modes=33), "max_modes"), (dict(link_trans=-0.5), "link_trans"),
                       (dict(link_rot=float("nan")), "link_trans"), (dict(link_trans=float("inf")), "link_trans"), (dict(link_rot=-1e-300), "link_trans"),
                       (dict(P=0), "P >= 1"), (dict(P=-3), "P >= 1")):
        assert _raw(s, x=x, **kw) == ERR_INVALID and needle in _err(s), (kw, _err(s))
    assert _raw(s, w=w) == ERR_INVALID and "weightsP without particles6xP" in _err(s)
    for bad in (-1.0, float("nan"), float("inf")):
        wb = w.copy(); wb[7] = bad
        assert _raw(s, x=x, w=wb) == ERR_INVALID and "supplied weight" in _err(s)
    big = np.zeros((6, 2049))
    assert _raw(s, x=big) == ERR_INVALID and "2048" in _err(s)
    assert _raw(s, x=np.zeros((6, 2048)), max_modes=1) == 0, _err(s)                  # the largest set: one mode of 2048
    # the refused context stays usable
    assert s.stein_align() == hip.SteinICPState.ALIGN_SUCCESS and s.particle_modes(*WIDE).count.tolist() == [16]


# ------------------------------------------------------------------------------------------------ 5. the shim and the pipelines
def test_shim_driver_agrees_with_the_python_binding(hip, tmp_path):
    root = os.path.dirname(os.path.dirname(hip.library_path()))
    exe = str(tmp_path / "particle_modes_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-I",
                           os.path.join(root, "svn-icp_amd", "host"), os.path.join(root, "tests", "particle_modes_driver.cpp"), "-L",
                           os.path.join(root, "svn-icp_amd"), "-lsvnicp_hip", "-Wl,-rpath," + os.path.join(root, "svn-icp_amd"), "-o", exe])
    x = _STATE.get("basin_particles")
    if x is None:
        x = _basin(hip).get_particles().reshape(6, -1)
    w = np.linspace(0.5, 1.5, x.shape[1])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(struct.pack("<ii", x.shape[1], 1)); f.write(np.ascontiguousarray(x).tobytes()); f.write(w.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), repr(pc.LINK_T), repr(pc.LINK_R), "8"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    s = _bare(hip)
    got = s.particle_modes(pc.LINK_T, pc.LINK_R, 8, particles=x, weights=w)
    assert lines[0].split() == ["modes", "16", "0", "2", "2", "0"] and got.n_modes == 2
    for k in range(got.n_reported):
        v = lines[1 + k].split()
        assert v[:2] == ["mode", str(k)] and [int(t) for t in v[2:5]] == [got.label[k], got.count[k], got.best[k]]
        nums = np.array([float(t) for t in v[5:]])
        want = np.concatenate([[got.mass[k], got.cost_min[k], got.cost_mean[k]], got.mean[k], got.cov[k].ravel(), got.pose[k, :3, :3].ravel(), got.pose[k, :3, 3]])
        assert nums.tobytes() == want.tobytes(), k                 # %.17g round-trips: the same bits through both bindings
    assert [int(t) for t in lines[1 + got.n_reported].split()[1:]] == s.get_mode_labels().tolist()


def _drive(hip, n=4, points=8192):
    sc = hip.scans
    scene = sc.make_scene()
    return [(0.1 * k, sc.lidar_scan(scene, sc.rot_zyx(0.0, 0.0, np.radians(0.3 * k)), np.array([0.0, 0.0, 0.05 * k]), points, stream=300 + k)) for k in range(n)]


def test_python_pipeline_with_modes(hip):
    pl = hip.pipeline
    scans = _drive(hip)
    runs = {}
    for name, kw in (("off", {}), ("mean", dict(mode_link=WIDE)), ("heaviest", dict(mode_link=WIDE, mode_select="heaviest")),
                     ("tight", dict(mode_link=(0.02, 0.001), mode_max=32))):
        cfg = pl.PipelineConfig(min_range=1.0, max_range=80.0, voxel_size=0.5, map_voxel_size=0.5, map_voxel_max_points=20, map_range=100.0,
                                particle_count=16, solver=hip.SteinICPParam(iterations=8, lr=1.0, max_dist=1.0, KNN_count=30), **kw)
        pipe = pl.RegistrationPipeline(cfg, device=0)
        runs[name] = [pipe.process_scan(pts, stamp=t) for t, pts in scans]
    for k in range(1, len(scans)):
        off, mean, heavy, tight = (runs[n][k] for n in ("off", "mean", "heaviest", "tight"))
        assert off.modes is None and mean.modes is not None and mean.modes.n_modes == 1 and mean.modes.count.tolist() == [16]
        assert mean.pose.tobytes() == off.pose.tobytes() and mean.correction.tobytes() == off.correction.tobytes()   # "mean": bit-identical
        assert tight.pose.tobytes() == off.pose.tobytes() and tight.modes.n_modes >= 1
        rel = np.abs(heavy.pose - off.pose).max() / max(1.0, np.abs(off.pose).max())
        print(f"scan {k}: heaviest against mean {rel:.3e} relative; modes at the tight links {tight.modes.n_modes}")
        assert rel <= 2.0 ** -23 and np.allclose(heavy.pose, heavy.initial_guess @ pl.correction_to_pose(heavy.correction))
        assert np.array_equal(heavy.correction, heavy.modes.mean[0])


def test_cpp_pipeline_with_modes(hip, tmp_path):
    from test_pipeline_gpu import _build_pipeline_drive
    root = os.path.dirname(os.path.dirname(hip.library_path()))
    exe = _build_pipeline_drive(root)
    scans = _drive(hip, n=3)
    with open(tmp_path / "scans.bin", "wb") as f:
        f.write(struct.pack("<i", len(scans)))
        for stamp, pts in scans:
            f.write(struct.pack("<di", stamp, pts.shape[0])); f.write(np.ascontiguousarray(pts[:, :3], np.float32).tobytes())
    outs = {}
    for name, extra in (("off", []), ("mean", ["-", "0", "0", "0", "0", "0", "off", "mean", "10", "10"]),
                        ("heaviest", ["-", "0", "0", "0", "0", "0", "off", "heaviest", "10", "10"])):
        r = subprocess.run([exe, str(tmp_path / "scans.bin"), str(tmp_path / f"{name}.bin"), "16", "8", "30", "0.5"] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[name] = (open(tmp_path / f"{name}.bin", "rb").read(), [l for l in r.stdout.splitlines() if l.startswith("modes ")])
    assert outs["off"][0] == outs["mean"][0] and not outs["off"][1]          # every byte the drive writes: poses, corrections, clouds
    assert len(outs["mean"][1]) == len(scans) - 1
    for line in outs["mean"][1]:
        head = line.split(" | ")[0].split()
        assert head[2:] == ["1", "1", "0", "0"] and line.split(" | ")[1].split()[:3] == ["0", "16", "-1"], line
    # "heaviest" with wide links: the poses stay within 2^-23 relative of "mean"

    def poses(raw):
        off, out = 0, []
        for _ in scans:   # int32 aligned, f64 pose[12] guess[12] corr[6] var[6] cov[36], int64 B M, f64 src[3B] tgt[3M] init[6P]
            out.append(np.frombuffer(raw, "<f8", 12, off + 4))
            B, M = np.frombuffer(raw, "<i8", 2, off + 4 + 72 * 8)
            off += 4 + 72 * 8 + 16 + 8 * (3 * int(B) + 3 * int(M) + 6 * 16)
        assert off == len(raw)
        return np.array(out)
    pm_, ph = poses(outs["mean"][0]), poses(outs["heaviest"][0])
    rel = np.abs(ph - pm_).max() / max(1.0, np.abs(pm_).max())
    print(f"C++ pipeline: heaviest against mean {rel:.3e} relative")
    assert rel <= 2.0 ** -23
    assert outs["heaviest"][1][-1].split(" | ")[1].split()[:2] == ["0", "16"]
