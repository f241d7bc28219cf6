"""Capsule casts and capsule overlaps on the host (no GPU): the nh_CapsuleCast record and NH_SHAPE_CAPSULE of include/nudge_hip.h against their
Python mirrors, and the capsule arithmetic of nudge_amd/csrc/nh_query.h -- built for the host by tests/hostcapsule_util.py, the same bits as the
device -- against an independent float64 model: the distance from the translating capsule's segment to a convex collider is convex in t, so the
model finds its minimum by ternary search and the first touch by bisection.  Named cases, the degenerate identities (half height 0 is a sphere cast
and a sphere query, bit for bit), start overlaps, invalid casts and the overlap predicate's AABB guard."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostcapsule_util as H                 # noqa: E402
import hostcast_util as CAST                 # noqa: E402
import hostoverlap_util as O                 # noqa: E402
import hostquery_util as Q                   # noqa: E402
from query_util import unit_quats as _unit_quats      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

NONE = 0xFFFFFFFF
IDENTITY = np.float32([0, 0, 0, 1])


def test_capsule_cast_record_and_shape_match_the_header(tmp_path):
    """nh_CapsuleCast: 64 bytes, every member offset as gcc lays it out, the ctypes mirror and the numpy record; its first 32 bytes are nh_Ray's.
    NH_SHAPE_CAPSULE is 2 on both sides."""
    members = ("origin", "max_t", "direction", "ignore_body", "rotation", "radius", "half_height", "reserved")
    body = "".join(f'  printf("%zu %zu\\n", sizeof(nh_CapsuleCast), offsetof(nh_CapsuleCast, {m}));\n' for m in members)
    body += "".join(f'  printf("%zu\\n", offsetof(nh_Ray, {m}));\n' for m in members[:4])
    body += '  printf("%u\\n", (unsigned)NH_SHAPE_CAPSULE);\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nudge_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    for k, m in enumerate(members):
        size, off = (int(v) for v in lines[k].split())
        assert ctypes.sizeof(E.CapsuleCast) == size == E.CAPSULE_CAST.itemsize == 64, size
        assert getattr(E.CapsuleCast, m).offset == off == E.CAPSULE_CAST.fields[m][1], (m, off)
        if k < 4:
            assert int(lines[len(members) + k]) == off == E.RAY.fields[m][1] == getattr(E.Ray, m).offset, m
    assert int(lines[len(members) + 4]) == E.NH_SHAPE_CAPSULE == 2
    assert len({E.NH_SHAPE_BOX, E.NH_SHAPE_SPHERE, E.NH_SHAPE_CAPSULE, E.NH_SHAPE_NONE}) == 4
    assert "nh_capsulecast" in E.EXPORTS


# ---- the float64 model ------------------------------------------------------------------------------------------------------------------------
def _mat(q):
    x, y, z, s = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y)],
                     [2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)],
                     [2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)]])


def _ternary(f, lo, hi, iters):
    """Argmin of functions convex on [lo, hi] (vectorised: lo, hi arrays; f maps an array of points to an array of values)."""
    lo, hi = lo.copy(), hi.copy()
    for _ in range(iters):
        m1, m2 = lo + (hi - lo) / 3.0, hi - (hi - lo) / 3.0
        left = f(m1) <= f(m2)
        hi = np.where(left, m2, hi)
        lo = np.where(left, lo, m1)
    return 0.5 * (lo + hi)


class _Model:
    """Capsules (c + t d, a, r) against boxes (p, R, h) or spheres (p, R = radius), float64, vectorised over n pairs."""

    def __init__(self, o, d, a, r, p, R=None, h=None, radius=None):
        self.o, self.d, self.a, self.r, self.p, self.R, self.h, self.rad = o, d, a, r, p, R, h, radius

    def _closest(self, x):
        """(closest collider point, distance) of world points x (n, 3)."""
        if self.h is None:
            v = x - self.p
            n = np.linalg.norm(v, axis=1)
            return self.p + v * (np.minimum(n, self.rad) / np.where(n > 0, n, 1.0))[:, None], np.maximum(n - self.rad, 0.0)
        xl = np.einsum("nji,nj->ni", self.R, x - self.p)
        cl = np.clip(xl, -self.h, self.h)
        return self.p + np.einsum("nij,nj->ni", self.R, cl), np.linalg.norm(xl - cl, axis=1)

    def seg(self, t):
        """(distance from the segment at t to the collider, the segment parameter of its closest point)."""
        c = self.o + t[:, None] * self.d
        u = _ternary(lambda u: self._closest(c + u[:, None] * self.a)[1], -np.ones(len(t)), np.ones(len(t)), 70)
        return self._closest(c + u[:, None] * self.a)[1], u

    def cast(self):
        """(hit, t, normal, start) of the first touch for t >= 0 (up to twice the time to pass the collider's centre, and beyond); t = 0 and -d/|d|
        for a start overlap."""
        n = len(self.o)
        g = lambda t: self.seg(t)[0] - self.r
        start = g(np.zeros(n)) <= 0.0
        T = 2.0 * (np.linalg.norm(self.o - self.p, axis=1) + 20.0) / np.linalg.norm(self.d, axis=1)
        tmin = _ternary(g, np.zeros(n), T, 100)
        hit = start | (g(tmin) <= 0.0)
        lo, hi = np.zeros(n), tmin.copy()
        for _ in range(70):
            mid = 0.5 * (lo + hi)
            inside = g(mid) <= 0.0
            hi = np.where(inside, mid, hi)
            lo = np.where(inside, lo, mid)
        t = np.where(start, 0.0, hi)
        _, u = self.seg(t)
        x = self.o + t[:, None] * self.d + u[:, None] * self.a
        q, _ = self._closest(x)
        nv = x - q
        nv = nv / np.maximum(np.linalg.norm(nv, axis=1), 1e-300)[:, None]
        inside = -self.d / np.linalg.norm(self.d, axis=1)[:, None]
        nv = np.where(start[:, None], inside, nv)
        return hit, t, nv, start


def _inside(d):
    """-d / |d| with the library's float32 operations and their order."""
    d = np.asarray(d, dtype=np.float32)
    l = np.sqrt(np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    return np.float32([-d[0] / l, -d[1] / l, -d[2] / l])


def _axes(q32, hh32):
    """World half axes a = rotate(q, (0, hh, 0)) in float64."""
    return np.stack([_mat(q)[:, 1] * float(h) for q, h in zip(q32, hh32)])


def _random_cases(rng, n, box=True, far=(2.0, 10.0), long=False):
    p = rng.uniform(-5.0, 5.0, size=(n, 3)).astype(np.float32)
    q, qb = _unit_quats(rng, n), _unit_quats(rng, n)
    r = rng.uniform(0.05, 1.0, size=n).astype(np.float32)
    hh = rng.uniform(0.1, 3.0 if long else 1.5, size=n).astype(np.float32)
    hb = rng.uniform(0.2, 2.0, size=(n, 3)).astype(np.float32)
    dirn = rng.normal(size=(n, 3))
    dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
    o = (p + dirn * (rng.uniform(*far, size=(n, 1)) + 5.0)).astype(np.float32)
    d = p + rng.normal(scale=1.5, size=(n, 3)) - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, size=(n, 1))).astype(np.float32)
    return o, d, q, r, hh, p, qb, hb


def _compare(o, d, q, r, hh, p, qb, hb, box, what, edge=1e-5, ttol=2e-5, ntol=2e-3, min_hits=50, min_stable=0.9):
    """The float32 predicate against the model for every case whose hit / miss is the same with r scaled by 1 -+ edge (away from grazing)."""
    n = len(o)
    f = lambda x: np.asarray(x, dtype=np.float64)
    a = _axes(q, hh)
    Rb = np.stack([_mat(x) for x in qb]) if box else None
    args = dict(R=Rb, h=f(hb)) if box else dict(radius=f(hb[:, 0]))
    ref = _Model(f(o), f(d), a, f(r), f(p), **args).cast()
    lo = _Model(f(o), f(d), a, f(r) * (1 - edge), f(p), **args).cast()
    hi = _Model(f(o), f(d), a, f(r) * (1 + edge), f(p), **args).cast()
    stable = (ref[0] == lo[0]) & (ref[0] == hi[0]) & (ref[3] == lo[3]) & (ref[3] == hi[3])
    hits = 0
    for i in np.nonzero(stable)[0]:
        if box:
            t, nn, hit = H.sweep_capsule_box(o[i], d[i], q[i], r[i], hh[i], p[i], qb[i], hb[i])
        else:
            t, nn, hit = H.sweep_capsule_sphere(o[i], d[i], q[i], r[i], hh[i], p[i], hb[i, 0])
        assert hit == ref[0][i], (what, i, hit, ref[1][i])
        if not hit:
            continue
        hits += 1
        assert abs(t - ref[1][i]) <= ttol * max(ref[1][i], 1.0), (what, i, t, ref[1][i], ref[3][i])
        assert abs(np.linalg.norm(nn.astype(np.float64)) - 1.0) <= 1e-5, (what, i, nn)
        if ref[3][i]:
            assert t == 0.0 and np.array_equal(nn, _inside(d[i])), (what, i)
            continue
        assert nn.astype(np.float64) @ d[i] < 0.0, (what, i, nn)
        if abs(hi[1][i] - lo[1][i]) <= 1e-3 * max(ref[1][i], 1.0):     # (the contact feature is stable: the normal is defined)
            assert np.abs(nn - ref[2][i]).max() <= ntol, (what, i, nn, ref[2][i])
    assert stable.mean() > min_stable, (what, stable.mean())
    assert hits >= min_hits, (what, hits)
    return hits


def test_capsule_box_sweeps_against_the_float64_model():
    rng = np.random.default_rng(51)
    _compare(*_random_cases(rng, 1500), box=True, what="random poses")
    _compare(*_random_cases(rng, 600, long=True), box=True, what="long capsules")
    _compare(*_random_cases(rng, 400, far=(200.0, 400.0)), box=True, what="far casts", ttol=1e-5)


def test_capsule_sphere_sweeps_against_the_float64_model():
    rng = np.random.default_rng(52)
    o, d, q, r, hh, p, qb, hb = _random_cases(rng, 1500)
    _compare(o, d, q, r, hh, p, qb, hb, box=False, what="random poses")
    _compare(*_random_cases(rng, 400, far=(200.0, 400.0)), box=False, what="far casts", ttol=1e-5)


def test_rolled_long_capsules_beside_box_edges_and_near_parallel_edges():
    """Long capsules rolled to lie along or across an edge of the box (its frame's axes, turned by a small angle -- down to parallel), swept at the
    edge: the edge roots, the skipped near-parallel pairs and the vertex / end-ball candidates that take over from them."""
    rng = np.random.default_rng(53)
    rows = []
    for i in range(900):
        qb = _unit_quats(rng, 1)[0]
        Rb = _mat(qb)
        hb = rng.uniform(0.3, 1.5, size=3)
        k = i % 3
        i1, i2 = (k + 1) % 3, (k + 2) % 3
        ang = [0.0, 1e-6, 1e-4, 1e-3, 3e-3, 1e-2, 0.1, 0.5][i % 8]
        # the capsule's axis: the edge's axis k turned by `ang` about the edge's outward diagonal
        axis = np.zeros(3); axis[k] = 1.0
        nrm = np.zeros(3); nrm[i1], nrm[i2] = 1.0, 1.0
        nrm /= np.linalg.norm(nrm)
        side = np.cross(nrm, axis)
        ax_l = np.cos(ang) * axis + np.sin(ang) * side
        ax_w = Rb @ ax_l
        # the rotation taking y to ax_w
        y = np.array([0.0, 1.0, 0.0])
        v, c = np.cross(y, ax_w), y @ ax_w
        q = np.array([*v, 1.0 + c]) if c > -0.999999 else np.array([1.0, 0.0, 0.0, 0.0])
        q /= np.linalg.norm(q)
        r = rng.uniform(0.05, 0.6)
        hh = rng.uniform(0.5, 3.0)
        edge_pt = np.zeros(3); edge_pt[i1], edge_pt[i2] = hb[i1], hb[i2]
        edge_pt[k] = rng.uniform(-0.5, 0.5) * hb[k]
        start_l = edge_pt + nrm * (r + rng.uniform(1.0, 4.0)) + rng.normal(scale=0.3, size=3) * 0.3
        dl = edge_pt - start_l + rng.normal(scale=0.1, size=3)
        p = rng.uniform(-5, 5, size=3)
        rows.append((p + Rb @ start_l, Rb @ dl, q, r, hh, p, qb, hb))
    cols = [np.asarray([row[j] for row in rows], dtype=np.float32) for j in range(8)]
    hits = _compare(*cols, box=True, what="edges", ttol=3e-5, min_hits=500)
    assert hits > 600


def test_grazing_casts_keep_their_answer_where_float64_is_stable():
    """Capsules that slide past a box at the touching distance -+ small offsets: where the float64 answer is stable under 1e-5 of r, the predicate
    agrees about hit or miss; at the exact touching distance it hits or misses but never reports t beyond the model's window."""
    rng = np.random.default_rng(54)
    rows = []
    for i in range(600):
        hb = rng.uniform(0.3, 1.5, size=3)
        r, hh = rng.uniform(0.1, 0.8), rng.uniform(0.2, 2.0)
        off = [0.0, 1e-6, -1e-6, 1e-4, -1e-4, 1e-2, -1e-2][i % 7]
        qb = _unit_quats(rng, 1)[0]
        Rb = _mat(qb)
        # upright in the box frame (axis along the box's y), sliding along x past the +z face
        q = _unit_quats(rng, 1)[0] if i % 2 else np.float32(qb)
        a_l = Rb.T @ (_mat(q)[:, 1] * hh)
        ext = np.abs(a_l) + r
        start_l = np.array([-(hb[0] + ext[0] + 2.0), 0.0, hb[2] + ext[2] + off])
        p = rng.uniform(-5, 5, size=3)
        rows.append((p + Rb @ start_l, Rb @ np.array([1.0, 0.0, 0.0]), q, r, hh, p, qb, hb))
    cols = [np.asarray([row[j] for row in rows], dtype=np.float32) for j in range(8)]
    _compare(*cols, box=True, what="grazing", min_hits=100, min_stable=0.5)


# ---- named cases --------------------------------------------------------------------------------------------------------------------------
def _rot_z(angle):
    return np.float32([0.0, 0.0, np.sin(angle / 2), np.cos(angle / 2)])


def test_an_upright_capsule_dropped_onto_a_face_hits_at_the_end_ball_distance():
    t, n, hit = H.sweep_capsule_box((0.3, 5, -0.2), (0, -1, 0), IDENTITY, 0.5, 1.0, (0, 0, 0), IDENTITY, (1, 1, 1))
    assert hit and t == 2.5 and np.array_equal(n, np.float32([0, 1, 0]))
    t2, n2, _ = CAST.sweep_box((0.3, 4, -0.2), (0, -1, 0), 0.5, (0, 0, 0), IDENTITY, (1, 1, 1))     # its lower end ball alone
    assert t2 == t and np.array_equal(n2, n)


def test_a_lying_capsule_swept_into_a_box_edge_touches_by_an_edge_root():
    s = np.sqrt(0.5)
    q = _rot_z(-3 * np.pi / 4)                        # the axis along (1, -1, 0) / sqrt(2): across the edge (1, 1, z)
    a = H.capsule_axis(q, 1.0)
    assert np.allclose(a, (s, -s, 0), atol=1e-6)
    t, n, hit = H.sweep_capsule_box((5, 5, 0), (-1, -1, 0), q, 0.5, 1.0, (0, 0, 0), IDENTITY, (1, 1, 1))
    assert hit and abs(t - (4.0 - 0.5 * s)) <= 2e-6, t
    assert np.allclose(n, (s, s, 0), atol=1e-6), n
    # neither end ball nor a vertex is there first: each alone reaches the box later
    for e in (-1, 1):
        tb, _, hb_ = CAST.sweep_box((5 + e * a[0], 5 + e * a[1], 0), (-1, -1, 0), 0.5, (0, 0, 0), IDENTITY, (1, 1, 1))
        assert not hb_ or tb > t + 0.01


def test_a_capsule_swept_past_a_corner_touches_by_a_vertex():
    """A capsule tilted to run diagonally past the corner (1, 1, 1), its segment's line 0.2 sqrt(2) from the corner in the y-z plane and both end
    balls clear of the faces: the vertex reaches its side first, at (x_c - 1)^2 + 0.08 = r^2."""
    tilt = np.float32([np.sin(-np.pi / 8), 0.0, 0.0, np.cos(-np.pi / 8)])     # the axis along (0, 1, -1) / sqrt(2)
    o = np.float32([5.0, 1.2, 1.2])
    t, n, hit = H.sweep_capsule_box(o, (-1, 0, 0), tilt, 0.5, 1.5, (0, 0, 0), IDENTITY, (1, 1, 1))
    xc = 1.0 + np.sqrt(0.25 - 0.08)
    assert hit and abs(t - (5.0 - xc)) <= 2e-6, t
    assert np.allclose(n, np.array([xc - 1.0, 0.2, 0.2]) / 0.5, atol=2e-6), n        # from the vertex towards the axis
    a = H.capsule_axis(tilt, 1.5)
    assert abs(float(n @ a)) <= 1e-5
    for e in (-1, 1):                                                  # the end balls alone reach the box later or never
        tb, _, hb_ = CAST.sweep_box(o + e * a, (-1, 0, 0), 0.5, (0, 0, 0), IDENTITY, (1, 1, 1))
        assert not hb_ or tb > t + 0.01
    ref = _Model(o[None].astype(np.float64), np.array([[-1.0, 0, 0]]), _axes([tilt], [1.5]), np.array([0.5]), np.zeros((1, 3)), R=np.eye(3)[None],
                 h=np.ones((1, 3))).cast()
    assert abs(ref[1][0] - t) <= 1e-5


def _world(boxes=(), spheres=(), bodies=None):
    nb = 1 + max([b for *_, b in list(boxes) + list(spheres)] + [0]) if bodies is None else bodies
    bt = np.zeros(nb, dtype=S.TRANSFORM)
    bt["rotation"][:, 3] = 1.0
    xt = np.zeros(len(boxes), dtype=S.TRANSFORM)
    xd = np.zeros(len(boxes), dtype=S.BOX)
    for i, (p, h, b) in enumerate(boxes):
        xt[i]["position"], xt[i]["body"], xt[i]["rotation"] = p, b, (0, 0, 0, 1)
        xd[i]["size"] = h
    st = np.zeros(len(spheres), dtype=S.TRANSFORM)
    sd = np.zeros(len(spheres), dtype=S.SPHERE)
    for i, (p, r, b) in enumerate(spheres):
        st[i]["position"], st[i]["body"], st[i]["rotation"] = p, b, (0, 0, 0, 1)
        sd[i]["radius"] = r
    scene = dict(box_transforms=xt, box_data=xd, box_tags=np.arange(len(boxes), dtype=np.uint32) + 100,
                 sphere_transforms=st, sphere_data=sd, sphere_tags=np.arange(len(spheres), dtype=np.uint32) + 200)
    return Q.records(bt, scene), len(boxes)


def _cast(world, o, d, r, hh, q=IDENTITY, max_t=np.inf, ignore=NONE):
    rec, nbox = world
    c = np.zeros(1, dtype=E.CAPSULE_CAST)
    c["origin"], c["direction"], c["radius"], c["half_height"], c["rotation"], c["max_t"], c["ignore_body"] = o, d, r, hh, q, max_t, ignore
    return CAST.cast(CAST.CAPSULE, rec, nbox, c)[0]


def test_a_slot_narrower_than_the_capsule_blocks_it_and_a_wider_one_lets_it_pass():
    for gap, blocked in ((0.9, True), (1.1, False)):
        w = _world(boxes=[((-(1 + gap / 2), 0, 0), (1, 1, 1), 1), ((1 + gap / 2, 0, 0), (1, 1, 1), 1)])
        h = _cast(w, (0, 5, 0), (0, -1, 0), 0.5, 1.0, max_t=20.0)
        if blocked:
            # the lower end ball rests on the two top edges: its centre at 1 + sqrt(r^2 - (gap / 2)^2)
            assert h["shape"] == E.NH_SHAPE_BOX and abs(h["t"] - (5 - 1 - 1 - np.sqrt(0.25 - 0.2025))) <= 2e-6, h
        else:
            assert h["shape"] == E.NH_SHAPE_NONE and h["t"] == 20.0, h
        # lying across the slot, it is blocked either way: its segment spans both boxes
        h = _cast(w, (0, 5, 0), (0, -1, 0), 0.5, 1.0, q=_rot_z(np.pi / 2), max_t=20.0)
        assert h["shape"] == E.NH_SHAPE_BOX and abs(h["t"] - 3.5) <= 1e-6, h


def test_a_non_unit_direction_scales_t():
    rng = np.random.default_rng(55)
    o, d, q, r, hh, p, qb, hb = _random_cases(rng, 400)
    hits = 0
    for i in range(len(o)):
        for box in (True, False):
            f = H.sweep_capsule_box if box else H.sweep_capsule_sphere
            args = (p[i], qb[i], hb[i]) if box else (p[i], hb[i, 0])
            a = f(o[i], d[i], q[i], r[i], hh[i], *args)
            b = f(o[i], d[i] * np.float32(2.0), q[i], r[i], hh[i], *args)
            assert a[2] == b[2]
            if a[2]:
                hits += 1
                assert abs(b[0] * 2 - a[0]) <= 1e-5 * max(a[0], 1.0) and np.allclose(a[1], b[1], atol=1e-4), (i, box, a, b)
    assert hits > 100


# ---- degenerate identities, bit for bit -----------------------------------------------------------------------------------------------------
def test_half_height_zero_is_the_sphere_cast_and_the_ray_bit_for_bit():
    rng = np.random.default_rng(56)
    o, d, q, r, hh, p, qb, hb = _random_cases(rng, 1500)
    r[::4] = 0.0
    qn = q.copy()
    qn[::2] = np.nan                                                   # (hh = 0 does not read the rotation)
    for i in range(len(o)):
        a = H.sweep_capsule_box(o[i], d[i], qn[i], r[i], 0.0, p[i], qb[i], hb[i])
        b = CAST.sweep_box(o[i], d[i], r[i], p[i], qb[i], hb[i])
        assert a[2] == b[2] and np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes() and a[1].tobytes() == b[1].tobytes(), i
        a = H.sweep_capsule_sphere(o[i], d[i], qn[i], r[i], 0.0, p[i], hb[i, 0])
        b = CAST.sweep_sphere(o[i], d[i], r[i], p[i], hb[i, 0])
        assert a[2] == b[2] and np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes() and a[1].tobytes() == b[1].tobytes(), i
        if r[i] == 0.0:
            c = Q.ray_box(o[i], d[i], p[i], qb[i], hb[i])
            assert H.sweep_capsule_box(o[i], d[i], qn[i], 0.0, 0.0, p[i], qb[i], hb[i])[0] == CAST.sweep_box(o[i], d[i], 0.0, p[i], qb[i], hb[i])[0]
            assert c[2] == H.sweep_capsule_box(o[i], d[i], qn[i], 0.0, 0.0, p[i], qb[i], hb[i])[2]
    # whole worlds: hh = 0 writes nh_spherecast's bytes, and r = hh = 0 nh_raycast's
    scene = S.pile(300, 200, seed=5)
    rec = Q.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    n = 4096
    lo, hi = np.float32([-12, -2, -12]), np.float32([12, 40, 12])
    caps = np.zeros(n, dtype=E.CAPSULE_CAST)
    caps["origin"] = rng.uniform(lo, hi, size=(n, 3))
    dd = rng.normal(size=(n, 3))
    caps["direction"] = dd / np.linalg.norm(dd, axis=1, keepdims=True)
    caps["max_t"] = rng.choice([np.inf, 5.0, 30.0], size=n)
    caps["ignore_body"] = np.where(rng.random(n) < 0.2, rng.integers(0, 64, size=n), NONE)
    caps["radius"] = rng.choice(np.float32([0.0, 0.25, 1.0]), size=n)
    caps["rotation"] = _unit_quats(rng, n)
    caps["rotation"][::3] = np.nan
    sph = np.zeros(n, dtype=E.SPHERE_CAST)
    for k in ("origin", "max_t", "direction", "ignore_body", "radius"):
        sph[k] = caps[k]
    got = CAST.cast(CAST.CAPSULE, rec, nbox, caps)
    assert got.tobytes() == CAST.cast(CAST.SPHERE, rec, nbox, sph).tobytes()
    assert (got["shape"] != NONE).mean() > 0.2
    zero = caps["radius"] == 0.0
    rays = np.zeros(int(zero.sum()), dtype=E.RAY)
    for k in ("origin", "max_t", "direction", "ignore_body"):
        rays[k] = caps[k][zero]
    assert got[zero].tobytes() == CAST.cast(CAST.RAY, rec, nbox, rays).tobytes()


def test_half_height_zero_capsule_overlap_is_the_sphere_predicate():
    rng = np.random.default_rng(57)
    o, d, q, r, hh, p, qb, hb = _random_cases(rng, 3000)
    c = (p + rng.normal(scale=1.5, size=(len(p), 3))).astype(np.float32)
    q[::2] = np.nan
    n_true = 0
    for i in range(len(c)):
        a = H.overlap_capsule_box(c[i], q[i], r[i], 0.0, p[i], qb[i], hb[i])
        assert a == O.sphere_box(c[i], r[i], p[i], qb[i], hb[i]), i
        b = H.overlap_capsule_sphere(c[i], q[i], r[i], 0.0, p[i], hb[i, 0])
        assert b == O.sphere_sphere(c[i], r[i], p[i], hb[i, 0]), i
        n_true += a + b
    assert n_true > 300


# ---- overlap predicates ----------------------------------------------------------------------------------------------------------------------
def test_capsule_overlap_predicates_against_the_float64_distance():
    rng = np.random.default_rng(58)
    o, d, q, r, hh, p, qb, hb = _random_cases(rng, 3000, long=True)
    c = (p + rng.normal(scale=2.0, size=(len(p), 3))).astype(np.float32)
    f = lambda x: np.asarray(x, dtype=np.float64)
    a = _axes(q, hh)
    Rb = np.stack([_mat(x) for x in qb])
    z = np.zeros(len(c))
    dist_b = _Model(f(c), np.zeros_like(a), a, f(r), f(p), R=Rb, h=f(hb)).seg(z)[0]
    dist_s = _Model(f(c), np.zeros_like(a), a, f(r), f(p), radius=f(hb[:, 0])).seg(z)[0]
    ends = 0
    for i in range(len(c)):
        box = H.overlap_capsule_box(c[i], q[i], r[i], hh[i], p[i], qb[i], hb[i])
        sph = H.overlap_capsule_sphere(c[i], q[i], r[i], hh[i], p[i], hb[i, 0])
        if abs(dist_b[i] - r[i]) > 1e-5 * max(r[i], 1.0):
            assert box == (dist_b[i] <= r[i]), (i, dist_b[i], r[i])
        if abs(dist_s[i] - r[i]) > 1e-5 * max(r[i], 1.0):
            assert sph == (dist_s[i] <= r[i]), (i, dist_s[i], r[i])
        # whatever the sphere query accepts at either end point is accepted
        ax = H.capsule_axis(q[i], hh[i])
        for e in (c[i] - ax, c[i] + ax):
            if O.sphere_box(e, r[i], p[i], qb[i], hb[i]):
                ends += 1
                assert box, i
    assert ends > 100


def test_the_overlap_guard_keeps_every_accepted_collider_inside_the_padded_capsule_aabb():
    """Touching capsules built at the very distance r from boxes and spheres: whatever the predicates accept has a world AABB that touches the
    capsule's c -+ (|a_k| + r) -- the box the walk prunes by, before its padding."""
    rng = np.random.default_rng(59)
    o, d, q, r, hh, p, qb, hb = _random_cases(rng, 4000, long=True)
    n = len(p)
    # centres at about the touching distance from the collider, in random directions
    dirn = rng.normal(size=(n, 3))
    dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
    c = (p + dirn * (np.linalg.norm(hb, axis=1) + r + hh)[:, None] * rng.uniform(0.3, 1.2, size=(n, 1))).astype(np.float32)
    accepted = 0
    for i in range(n):
        a = H.capsule_axis(q[i], hh[i]).astype(np.float64)
        e = np.abs(a) + r[i]
        lo, hi = c[i] - e, c[i] + e
        pad = np.abs(np.concatenate([lo, hi])).max() * 2.0 ** -18
        for box in (True, False):
            ok = H.overlap_capsule_box(c[i], q[i], r[i], hh[i], p[i], qb[i], hb[i]) if box else H.overlap_capsule_sphere(c[i], q[i], r[i], hh[i], p[i], hb[i, 0])
            if not ok:
                continue
            accepted += 1
            eb = np.abs(_mat(qb[i])) @ hb[i] if box else np.full(3, float(hb[i, 0]))
            assert (p[i] - eb <= hi + pad).all() and (lo - pad <= p[i] + eb).all(), (i, box)
    assert accepted > 1000


# ---- start overlaps, invalid casts, missing bodies ------------------------------------------------------------------------------------------
def test_a_start_overlap_under_the_overlap_predicates_hits_at_zero():
    rng = np.random.default_rng(60)
    o, d, q, r, hh, p, qb, hb = _random_cases(rng, 3000)
    c = (p + rng.normal(scale=1.5, size=(len(p), 3))).astype(np.float32)
    starts = 0
    for i in range(len(c)):
        inside = _inside(d[i])
        if H.overlap_capsule_box(c[i], q[i], r[i], hh[i], p[i], qb[i], hb[i]):
            t, nn, hit = H.sweep_capsule_box(c[i], d[i], q[i], r[i], hh[i], p[i], qb[i], hb[i])
            assert hit and t == 0.0 and np.array_equal(nn, inside), i
            starts += 1
        if H.overlap_capsule_sphere(c[i], q[i], r[i], hh[i], p[i], hb[i, 0]):
            t, nn, hit = H.sweep_capsule_sphere(c[i], d[i], q[i], r[i], hh[i], p[i], hb[i, 0])
            assert hit and t == 0.0 and np.array_equal(nn, inside), i
            starts += 1
    assert starts > 500


def test_invalid_casts_are_nan_misses_and_missing_bodies_are_never_hit():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 5)], spheres=[((0, 0, 3), 1.0, 5)], bodies=2)
    assert _cast(w, (0, 0, -5), (0, 0, 1), 0.5, 1.0)["shape"] == NONE
    assert _cast(w, (0, 0, -0.5), (0, 0, 1), 0.5, 1.0)["shape"] == NONE
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 1)])
    assert _cast(w, (0, 0, -5), (0, 0, 1), 0.5, 1.0)["t"] == 3.5
    nanq = np.float32([np.nan, 0, 0, 1])
    for o, d, r, hh, q in (((np.nan, 0, -5), (0, 0, 1), 0.5, 1.0, IDENTITY), ((0, 0, -5), (0, np.inf, 1), 0.5, 1.0, IDENTITY),
                           ((0, 0, -5), (0, 0, 1), np.inf, 1.0, IDENTITY), ((0, 0, -5), (0, 0, 1), 0.5, np.nan, IDENTITY),
                           ((0, 0, -5), (0, 0, 1), -0.25, 1.0, IDENTITY), ((0, 0, -5), (0, 0, 1), 0.5, -1.0, IDENTITY),
                           ((0, 0, -5), (0, 0, 1), 0.5, 1.0, nanq), ((0, 0, -5), (0, 0, 1), 0.5, np.inf, IDENTITY)):
        h = _cast(w, o, d, r, hh, q)
        assert h["shape"] == NONE and np.isnan(h["t"]) and h["body"] == NONE and h["collider"] == NONE, (o, d, r, hh)
    h = _cast(w, (0, 0, -5), (0, 0, 1), 0.5, 0.0, nanq)                # hh = 0 does not read the rotation
    assert h["shape"] == E.NH_SHAPE_BOX and h["t"] == 3.5


def test_ties_ignore_body_and_max_t():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 2), ((0, 0, 0), (1, 1, 1), 1)], spheres=[((0, 0, 0), 1.0, 3)])
    h = _cast(w, (0, 5, 0), (0, -1, 0), 0.5, 1.0)
    assert h["shape"] == E.NH_SHAPE_BOX and h["collider"] == 0 and h["t"] == 2.5
    h = _cast(w, (0, 5, 0), (0, -1, 0), 0.5, 1.0, ignore=2)
    assert h["collider"] == 1 and h["body"] == 1
    h = _cast(w, (0, 5, 0), (0, -1, 0), 0.5, 1.0, max_t=2.0)
    assert h["shape"] == NONE and h["t"] == 2.0
    w = _world(spheres=[((0, 0, 0), 1.0, 1)])
    h = _cast(w, (0, 5, 0), (0, -1, 0), 0.5, 1.0)
    assert h["shape"] == E.NH_SHAPE_SPHERE and h["t"] == 2.5 and np.array_equal(h["normal"], np.float32([0, 1, 0]))
    h = _cast(w, (5, 0, 0), (-1, 0, 0), 0.5, 1.0)                      # the side of the cylinder
    assert h["t"] == 3.5 and np.array_equal(h["normal"], np.float32([1, 0, 0]))
    h = _cast(w, (0, 1.0, 0), (1, 0, 0), 0.5, 1.0)                      # a start overlap
    assert h["t"] == 0.0 and np.array_equal(h["normal"], np.float32([-1, 0, 0]))


def test_capsule_overlap_brute_force_matches_the_sphere_and_box_oracle_for_other_shapes():
    """hostcapsule's nh_overlap brute force is hostoverlap's for sphere and box queries, and hh = 0 capsules give the sphere query's records."""
    scene = S.pile(200, 100, seed=7)
    rec = Q.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    rng = np.random.default_rng(61)
    n = 2000
    qs = np.zeros(n, dtype=E.OVERLAP_QUERY)
    qs["center"] = rng.uniform((-10, -1, -10), (10, 25, 10), size=(n, 3))
    qs["shape"] = rng.choice([E.NH_SHAPE_SPHERE, E.NH_SHAPE_BOX], size=n)
    qs["rotation"] = _unit_quats(rng, n)
    qs["size"] = rng.uniform(0.1, 2.0, size=(n, 3))
    qs["ignore_body"] = np.where(rng.random(n) < 0.2, rng.integers(0, 64, size=n), NONE)
    a, b = H.overlap(rec, nbox, qs), O.overlap(rec, nbox, qs)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] > 100
    caps = qs.copy()
    caps["shape"] = E.NH_SHAPE_CAPSULE
    caps["size"][:, 1] = 0.0
    caps["rotation"][::2] = np.nan
    sph = qs.copy()
    sph["shape"] = E.NH_SHAPE_SPHERE
    a, b = H.overlap(rec, nbox, caps), O.overlap(rec, nbox, sph)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
