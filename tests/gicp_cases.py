"""Hand-built inputs of k_gicp_accumulate alone (test infrastructure; tests/test_gicp_alone_gpu.py), handed through the
split-phase ABI exactly as tests/plane_cases.py hands its cases to k_plane_accumulate: src, tgt, supplied normals of BOTH
clouds, a candidate table cand [B][K], total poses [P][12], max_dist, delta, epsilon.

    geometry   plane_cases.geometry_cases (every (PW, WP) instantiation, B in {1, pass -+ 1, pass, 2 pass + 1, 3 pass}, padded
               particles, grid_y = 2, several passes per workgroup) with source normals added: random, not unit, every 7th row none
    exact      dyadic coordinates, axis normals, identity rotations and epsilon = 1 (W = I exactly): every product and sum of
               the record is exact in float64, so the device must equal the restatement bit for bit whatever the order
    numeric    plane_cases.conditioning_cases (kilometre coordinates, a cancelling b) with source normals, and epsilon = 1e-6
               with near-antiparallel and near-orthogonal normals
The mpmath values of the geometry and numeric cases are in tests/golden/gicp/gicp.npz (tests/golden/make_gicp.py).
"""
import zlib

import numpy as np

import gicp_mp_reference as gm
import plane_cases as pc
import plane_reference as pr
import stage_b_cases as sc
import stage_b_reference as sb


class GicpCase:
    def __init__(self, name, tags, src, tgt, nrm_t, nrm_s, cand, poses, max_dist, delta, eps, min_steps=1):
        self.name, self.tags = name, frozenset(tags)
        self.src, self.tgt = np.ascontiguousarray(src, np.float64), np.ascontiguousarray(tgt, np.float64)
        self.nt_supplied, self.ns_supplied = np.ascontiguousarray(nrm_t, np.float64), np.ascontiguousarray(nrm_s, np.float64)
        self.nt = pr.normalise_supplied(self.nt_supplied, self.tgt)         # what k_pack_normals keeps
        self.ns = pr.normalise_supplied(self.ns_supplied, self.src)
        self.cand, self.poses = np.ascontiguousarray(cand, np.int32), np.ascontiguousarray(poses, np.float64)
        self.max_dist, self.delta, self.eps, self.min_steps = float(max_dist), float(delta), float(eps), int(min_steps)
        self.B, self.K, self.M, self.P = self.src.shape[0], self.cand.shape[1], self.tgt.shape[0], self.poses.shape[0]
        assert self.cand.min() >= 0 and self.cand.max() < self.M, "every candidate index lies in [0, M)"
        assert self.ns.shape == (self.B, 3) and self.nt.shape == (self.M, 3) and self.poses.shape == (self.P, 12)
        self._D = None

    def options(self):
        return (("chain", "general"), ("accum_min_steps", str(self.min_steps)))

    def discrete(self):
        if self._D is None:
            self._D = gm.discrete(self)
        return self._D

    def checksum(self):
        blob = b"".join(a.tobytes() for a in (self.src, self.tgt, self.nt_supplied, self.ns_supplied, self.cand, self.poses)) + \
            repr((self.max_dist, self.delta, self.eps, self.min_steps)).encode()
        return np.int64(zlib.crc32(blob))

    def mp_particles(self):
        return sb.mp_particles(self.P)

    def padded_particles(self):
        PW, WP = sc.stage_b_shape(self.P)
        return -(-self.P // (PW * WP)) * PW * WP


def from_plane(case, eps=1e-3, ns=None, tags=()):
    rng = pc.rng_for("gicp_" + case.name)
    if ns is None:
        ns = pc.random_normals(rng, case.B) * rng.uniform(0.5, 2.0, (case.B, 1))   # supplied normals need not be unit
        ns[3::7] = 0.0
    return GicpCase(case.name, tuple(case.tags) + tuple(tags), case.src, case.tgt, case.nrm_supplied, ns, case.cand, case.poses, case.max_dist,
                    case.delta, eps, case.min_steps)


def geometry_cases():
    return [from_plane(c) for c in pc.geometry_cases()]


# ------------------------------------------------------------------------------------------------ exact
AX = np.eye(3)


def _dyadic_scene(P):
    """16 targets 8 m apart on x with axis normals (target 5 has none); 6 rows near targets 1, 2, 3, 5, 7, 9 (row 2 has no
    source normal); K = 4 candidates 32 m apart, the winner at slot 1; identity rotations, dyadic translations."""
    tgt = np.zeros((16, 3))
    tgt[:, 0] = 8.0 * np.arange(16)
    tgt[:, 1] = 0.5 * (np.arange(16) % 3)
    nt = AX[np.arange(16) % 3].copy()
    nt[5] = 0.0
    win = np.array([1, 2, 3, 5, 7, 9])
    off = np.array([[0.25, -0.5, 0.125], [-0.375, 0.25, 0.5], [0.5, 0.5, -0.25], [0.125, 0.0, 0.25], [-0.5, 0.375, 0.0], [0.0, -0.25, -0.625]])
    src = tgt[win] + off
    ns = AX[(np.arange(6) + 1) % 3] * np.array([1.0, -2.0, 1.0, 0.5, -1.0, 4.0])[:, None]
    ns[2] = 0.0
    cand = np.stack([(win + 4) % 16, win, (win + 8) % 16, (win + 12) % 16], 1)
    poses = np.tile(sc.IDENT, (P, 1))
    poses[:, 9] = 0.0625 * np.arange(P)
    poses[:, 11] = -0.03125 * np.arange(P)
    return src, tgt, nt, ns, cand, poses


def exact_cases():
    out = []
    src, tgt, nt, ns, cand, poses = _dyadic_scene(4)
    out.append(GicpCase("exact_dyadic_delta_inf", ("exact",), src, tgt, nt, ns, cand, poses, 64.0, np.inf, 1.0))
    out.append(GicpCase("exact_all_rejected_no_source_normals", ("exact", "all_rejected"), src, tgt, nt, np.zeros_like(ns), cand, poses, 64.0, np.inf, 1.0))
    out.append(GicpCase("exact_all_rejected_by_the_gate", ("exact", "all_rejected"), src, tgt, nt, ns, cand, poses, 2.0 ** -6, np.inf, 1.0))
    # the gate: row 0 of particle 0 has d2 = 0.25^2 + 0.5^2 + 0.125^2 = 0.328125 exactly
    s1, t1, nt1, ns1, c1, p1 = _dyadic_scene(1)
    d2 = 0.328125
    s1[1] = t1[2] + np.array([0.125, 0.25, 0.0])              # row 1 lies well inside (d2 = 0.078125) and has both normals
    r = [0, 1]
    out.append(GicpCase("exact_gate_d2_equals_max_dist", ("exact", "gate_rejects_row0"), s1[r], t1, nt1, ns1[r], c1[r], p1, d2, np.inf, 1.0))
    out.append(GicpCase("exact_gate_d2_one_ulp_below", ("exact", "gate_accepts_row0"), s1[r], t1, nt1, ns1[r], c1[r], p1, np.nextafter(d2, 1.0), np.inf, 1.0))
    # Huber: one pair, s = (0, 0, 2), e = (0.5, 0, 0), W = I: rho = 0.5 exactly; every term is w times a power of two
    tgt2 = np.array([[-0.5, 0.0, 2.0], [40.0, 0.0, 0.0], [0.0, 40.0, 0.0], [0.0, 0.0, 40.0]])
    args = (np.array([[0.0, 0.0, 2.0]]), tgt2, AX[[0, 1, 2, 0]], AX[[1]], np.array([[1, 0, 2, 3]]), np.tile(sc.IDENT, (1, 1)), 64.0)
    out.append(GicpCase("exact_rho_equals_delta", ("exact", "huber_w1"), *args, 0.5, 1.0))
    out.append(GicpCase("exact_rho_one_ulp_above_delta", ("exact", "huber_below1"), *args, np.nextafter(0.5, 0.0), 1.0))
    return out


# ------------------------------------------------------------------------------------------------ numeric
def rotation_poses(rng, P, rot=0.002, trans=0.02):
    """Rotations to round-off (Rodrigues), distinct per particle.  At epsilon = 1e-6 the smallest eigenvalue of S is 2e-6 for a
    UNIT m = Rt^T n_q; plane_cases' arbitrary doubles near the identity stretch m by up to `rot` and would make S indefinite."""
    poses = np.zeros((P, 12))
    for p in range(P):
        w = rng.uniform(-rot, rot, 3)
        a = np.linalg.norm(w)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        poses[p, :9] = (np.eye(3) + np.sin(a) / a * K + (1 - np.cos(a)) / a ** 2 * K @ K).reshape(9)
    poses[:, 9:] = rng.uniform(-trans, trans, (P, 3))
    return poses


def numeric_cases():
    out = []
    km, cancel = pc.conditioning_cases()                       # kilometre coordinates; rows in pairs with opposite residuals
    out.append(from_plane(km, tags=("mp",)))
    rng = pc.rng_for("gicp_cancel_ns")                        # a pair of rows is one source point: one source normal for both
    out.append(from_plane(cancel, ns=np.repeat(pc.random_normals(rng, cancel.B // 2), 2, axis=0), tags=("mp",)))
    for kind in ("antiparallel", "orthogonal"):
        c = pc.scene_case("gicp_eps1e-6_" + kind, 16, 40, ("numeric",), K=4, bare_every=0)
        rng = pc.rng_for("gicp_ns_" + kind)
        nq = pr.normalise_supplied(c.nrm_supplied, c.tgt)[c.discrete()["widx"][0]]
        ns = -nq if kind == "antiparallel" else np.cross(nq, pc.random_normals(rng, c.B))
        ns = ns / np.linalg.norm(ns, axis=1, keepdims=True) + 1e-4 * pc.random_normals(rng, c.B)
        g = GicpCase(c.name, ("numeric", "mp", kind), c.src, c.tgt, c.nrm_supplied, ns, c.cand, rotation_poses(rng, c.P), c.max_dist, c.delta, 1e-6)
        assert (g.discrete()["win"] == c.discrete()["win"]).all() and g.discrete()["ok"].sum(1).min() >= 10
        out.append(g)
    return out


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = geometry_cases() + exact_cases() + numeric_cases()
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES
