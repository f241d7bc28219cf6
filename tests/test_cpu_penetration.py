"""Penetration queries on the host (no GPU): the six pair functions of nudge_amd/csrc/nh_query.h ("penetration") -- built for the host by
tests/hostpen_util.py, the device's bits -- against an independent float64 oracle by support functions, against the library's own overlap
predicates (the push separates, a shorter one does not), their exact special cases, and the brute-force nh_penetration against the brute-force
nh_overlap on whole worlds.

THE ORACLE.  For a unit direction u, the query shape A translated by g(u) u just touches the collider B, with
    g(u) = h_B(u) + h_A(-u) - u . (c_A - c_B),
h the support function about the centre: a box sum_k h_k |u . axis_k|, a sphere R, a capsule |u . a| + r.  The penetration depth is min_u g(u).
Nothing of it is shared with the code under test: no clamp, no separating axes, no closest points.

THE TOLERANCE is relative to the pair's scale (every half extent, radius and half height, plus the centre distance).  MEASURED on the seeded inputs
below with the host build (the worst deviation of |g(n) - depth| and of depth - min g(u), as a share of the scale):
    sphere/sphere 6.0e-08   sphere/box 1.1e-07   box/sphere 1.1e-07   capsule/sphere 6.4e-07   box/box 3.7e-06   capsule/box 9.2e-07
(box / box carries the 2^-20 of its radii: four to six terms of 2^-20 of a size on one axis, an edge axis' over the length of its cross product; the
rest is rounding).  TOL is set at twice the worst, 7.5e-6, below the 2^-16 = 1.5e-5 of the scale that this arithmetic allows."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostcapsule_util as HC               # noqa: E402
import hostpen_util as H                    # noqa: E402
import hostquery_util as Q                  # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

NONE = 0xFFFFFFFF
IDENT = (0.0, 0.0, 0.0, 1.0)
TOL = 7.5e-6                  # of the pair's scale: twice the measured worst (the docstring), and below 2^-16
KINDS = ("sphere/sphere", "sphere/box", "box/sphere", "capsule/sphere", "box/box", "capsule/box")
N_PAIRS = 1500                # per kind, world and rotation mode
N_DIRS = 4096


def test_the_tolerance_is_below_what_the_arithmetic_allows():
    assert TOL < 2.0 ** -16


def test_penetration_records_match_the_header(tmp_path):
    """nh_PenetrationHit: size and every member offset as gcc lays them out, against the ctypes mirror and the numpy records; its last 16 bytes are
    nh_OverlapHit's members in nh_OverlapHit's order."""
    ms = ("normal", "depth", "body", "collider", "shape", "tag")
    body = "".join(f'  printf("%zu %zu\\n", sizeof(nh_PenetrationHit), offsetof(nh_PenetrationHit, {m}));\n' for m in ms)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nudge_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    for k, m in enumerate(ms):
        size, off = (int(v) for v in lines[k].split())
        assert ctypes.sizeof(E.PenetrationHit) == size == E.PENETRATION_HIT.itemsize == H.HIT.itemsize == 32
        assert getattr(E.PenetrationHit, m).offset == off == E.PENETRATION_HIT.fields[m][1] == H.HIT.fields[m][1], (m, off)
    for m in ("body", "collider", "shape", "tag"):
        assert E.PENETRATION_HIT.fields[m][1] == 16 + E.OVERLAP_HIT.fields[m][1]
    assert "nh_penetration" in E.EXPORTS


# ---- seeded pairs --------------------------------------------------------------------------------------------------------------------------
def _quats(rng, n, identity):
    if identity:
        return np.tile(np.float32(IDENT), (n, 1))
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def _pairs(kind, n, seed, world, identity):
    """n pairs of one kind: the query records, the collider records and the box flags.  Sizes 0.05 to 4; the collider's centre within 2 of `world`;
    the query's centre = the collider's plus a uniform offset of up to the sum of both extents per axis (a box's extent its half extents, a sphere's
    its radius, a capsule's its radius, plus its half height on y)."""
    rng = np.random.default_rng(seed)
    qs, cs = kind.split("/")
    q = np.zeros(n, dtype=E.OVERLAP_QUERY)
    r = np.zeros(n, dtype=Q.REC)
    size = lambda *shape: rng.uniform(0.05, 4.0, size=shape).astype(np.float32)          # noqa: E731
    q["ignore_body"], q["rotation"] = NONE, _quats(rng, n, identity)
    if qs == "sphere":
        q["shape"] = E.NH_SHAPE_SPHERE
        q["size"][:, 0] = size(n)
        ea = np.repeat(q["size"][:, :1], 3, axis=1)
    elif qs == "box":
        q["shape"] = E.NH_SHAPE_BOX
        q["size"] = size(n, 3)
        ea = q["size"].copy()
    else:
        q["shape"] = E.NH_SHAPE_CAPSULE
        q["size"][:, :2] = size(n, 2)
        ea = np.repeat(q["size"][:, :1], 3, axis=1)
        ea[:, 1] += q["size"][:, 1]
    r["q"] = _quats(rng, n, identity)
    if cs == "box":
        r["h"] = size(n, 3)
    else:
        r["h"] = np.repeat(size(n, 1), 3, axis=1)
    r["p"] = (np.asarray(world, np.float64) + rng.uniform(-2, 2, size=(n, 3))).astype(np.float32)
    reach = ea.astype(np.float64) + r["h"]
    q["center"] = (r["p"] + rng.uniform(-1, 1, size=(n, 3)) * reach).astype(np.float32)
    return q, r, np.full(n, cs == "box")


# ---- the float64 oracle ----------------------------------------------------------------------------------------------------------------------
def _mats(q):
    x, y, z, s = (q[:, k].astype(np.float64) for k in range(4))
    m = np.empty((len(q), 3, 3))
    m[:, 0, 0], m[:, 0, 1], m[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y)
    m[:, 1, 0], m[:, 1, 1], m[:, 1, 2] = 2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)
    m[:, 2, 0], m[:, 2, 1], m[:, 2, 2] = 2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)
    return m


def _shapes(q, r, box):
    """Both shapes as (axes (n, 3, 3), extents along them (n, 3), radius (n,)): every support function is sum_k ext_k |u . axis_k| + radius."""
    n = len(q)
    A, B = _mats(q["rotation"]), _mats(r["q"])
    ea, ra = np.zeros((n, 3)), np.zeros(n)
    sph, cap, bx = q["shape"] == E.NH_SHAPE_SPHERE, q["shape"] == E.NH_SHAPE_CAPSULE, q["shape"] == E.NH_SHAPE_BOX
    ra[sph | cap] = q["size"][sph | cap, 0]
    ea[cap, 1] = q["size"][cap, 1]
    ea[bx] = q["size"][bx]
    eb = np.where(box[:, None], r["h"].astype(np.float64), 0.0)
    rb = np.where(box, 0.0, r["h"][:, 0].astype(np.float64))
    return (A, ea, ra), (B, eb, rb)


def _g(q, r, box, U):
    """g(u) of every pair (rows) for its own directions U (n, m, 3)."""
    (A, ea, ra), (B, eb, rb) = _shapes(q, r, box)
    d = q["center"].astype(np.float64) - r["p"].astype(np.float64)
    ha = (np.abs(np.einsum("nik,nmi->nmk", A, U)) * ea[:, None, :]).sum(axis=2) + ra[:, None]
    hb = (np.abs(np.einsum("nik,nmi->nmk", B, U)) * eb[:, None, :]).sum(axis=2) + rb[:, None]
    return ha + hb - np.einsum("nmi,ni->nm", U, d)


def _scale(q, r, box):
    (A, ea, ra), (B, eb, rb) = _shapes(q, r, box)
    d = q["center"].astype(np.float64) - r["p"].astype(np.float64)
    return ea.sum(axis=1) + ra + eb.sum(axis=1) + rb + np.linalg.norm(d, axis=1)


def _segment_meets_box(q, r):
    """float64: does the capsule's segment meet the box?  (the clip of its parameter against the three slabs)"""
    A, B = _mats(q["rotation"]), _mats(r["q"])
    a = A[:, :, 1] * q["size"][:, 1:2].astype(np.float64)
    ol = np.einsum("nik,ni->nk", B, q["center"].astype(np.float64) - r["p"])
    al = np.einsum("nik,ni->nk", B, a)
    h = r["h"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (-h - ol) / al, (h - ol) / al
    lo, hi = np.minimum(t0, t1), np.maximum(t0, t1)
    flat = al == 0
    lo[flat] = np.where(np.abs(ol[flat]) <= h[flat], -np.inf, np.inf)
    hi[flat] = np.where(np.abs(ol[flat]) <= h[flat], np.inf, -np.inf)
    return np.maximum(lo.max(axis=1), -1.0) <= np.minimum(hi.min(axis=1), 1.0)


def _on_an_edge_axis(q, r, n):
    """float64: is the box / box normal a face normal of neither box?"""
    A, B = _mats(q["rotation"]), _mats(r["q"])
    c = np.maximum(np.abs(np.einsum("nik,ni->nk", A, n)).max(axis=1), np.abs(np.einsum("nik,ni->nk", B, n)).max(axis=1))
    return c < 1.0 - 1e-6


CONFIGS = [(kind, world, identity) for kind in KINDS for world in ((0.0, 0.0, 0.0), (1000.0, 0.0, 0.0)) for identity in (False, True)]


def _accepted(kind, world, identity):
    seed = 7000 + CONFIGS.index((kind, world, identity))
    q, r, box = _pairs(kind, N_PAIRS, seed, world, identity)
    ok, n, depth = H.pairs(q, r, box)
    return q[ok], r[ok], box[ok], n[ok].astype(np.float64), depth[ok].astype(np.float64), seed


def deviations(kind, world, identity):
    """(|g(n) - depth|, max over the directions of depth - g(u), both as a share of the pair's scale; q, r, n) of the accepted pairs of one config."""
    q, r, box, n, depth, seed = _accepted(kind, world, identity)
    rng = np.random.default_rng(seed + 500)
    U = rng.normal(size=(N_DIRS, 3))
    U /= np.linalg.norm(U, axis=1, keepdims=True)
    # every pair gets the common random directions, turned by its own normal's sign pattern so that no two pairs see the same set, and its own normal
    nn = n / np.linalg.norm(n, axis=1, keepdims=True)
    flip = np.where(nn < 0, -1.0, 1.0)
    dirs = np.concatenate([nn[:, None, :], U[None, :, :] * flip[:, None, :]], axis=1)
    g = _g(q, r, box, dirs)
    s = _scale(q, r, box)
    return np.abs(g[:, 0] - depth) / s, (depth[:, None] - g).max(axis=1) / s, (q, r, n)


@pytest.mark.parametrize("kind", KINDS)
def test_depth_and_normal_against_the_support_function_oracle(kind):
    deep = shallow = edge = total = 0
    for k, world, identity in CONFIGS:
        if k != kind:
            continue
        at, below, (q, r, n) = deviations(kind, world, identity)
        what = (kind, world, identity)
        assert len(at) > N_PAIRS // 10, (what, len(at))                        # enough pairs were accepted
        assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-5, what
        print(f"{kind} world {world[0]:g} identity {identity}: {len(at)} pairs, worst |g(n) - depth| {at.max():.3g}, worst depth - g(u) {below.max():.3g} of the scale")
        assert at.max() <= TOL, (what, float(at.max()), int(at.argmax()))       # the push along the normal just separates
        assert below.max() <= TOL, (what, float(below.max()), int(below.argmax()))  # no direction of 4097 separates with less
        total += len(at)
        if kind == "capsule/box":
            m = _segment_meets_box(q, r)
            deep += int(m.sum()); shallow += int((~m).sum())
        if kind == "box/box" and not identity:
            edge += int(_on_an_edge_axis(q, r, n).sum())
    if kind == "capsule/box":
        assert deep >= 0.10 * total and shallow >= 0.10 * total, (deep, shallow, total)
    if kind == "box/box":
        assert edge >= 0.05 * total, (edge, total)


@pytest.mark.parametrize("kind", KINDS)
def test_the_push_separates_under_the_librarys_own_predicates(kind):
    """The query moved by (depth + 2 tol) n is rejected by nh_overlap's predicate; moved by (depth - 2 tol) n it is still accepted, wherever
    depth > 4 tol.  (tol = TOL of the pair's scale, and no less than the float32 grid of the moved centre's coordinates, which the move is rounded to.)"""
    kept = total = 0
    for k, world, identity in CONFIGS:
        if k != kind:
            continue
        q, r, box, n, depth, _ = _accepted(kind, world, identity)
        c = q["center"].astype(np.float64)
        tol = np.maximum(TOL * _scale(q, r, box), np.spacing(np.abs(c).max(axis=1).astype(np.float32)).astype(np.float64))
        out, back = q.copy(), q.copy()
        out["center"] = (c + (depth + 2 * tol)[:, None] * n).astype(np.float32)
        back["center"] = (c + (depth - 2 * tol)[:, None] * n).astype(np.float32)
        still = H.pairs(out, r, box)[0]
        assert not still.any(), (kind, world, identity, int(still.sum()), int(still.argmax()))
        far = depth > 4 * tol
        gone = ~H.pairs(back, r, box)[0] & far
        assert not gone.any(), (kind, world, identity, int(gone.sum()), int(gone.argmax()))
        kept += int(far.sum()); total += len(far)
    assert kept >= 0.8 * total, (kind, kept, total)


# ---- exactness of the special cases ----------------------------------------------------------------------------------------------------------
def _query(shape, center, size, rotation=IDENT, ignore=NONE):
    q = np.zeros(1, dtype=E.OVERLAP_QUERY)
    q["shape"], q["center"], q["rotation"], q["ignore_body"] = shape, center, rotation, ignore
    q["size"][0, :len(size)] = size
    return q


def _world_queries(rec, rng, n):
    """Mixed sphere, box and capsule queries around the colliders of a world: some touch several colliders, some none."""
    live = rec["p"][np.isfinite(rec["p"]).all(axis=1)].astype(np.float64)
    q = np.zeros(n, dtype=E.OVERLAP_QUERY)
    q["shape"] = rng.choice([E.NH_SHAPE_SPHERE, E.NH_SHAPE_BOX, E.NH_SHAPE_CAPSULE], size=n)
    q["center"] = live[rng.integers(0, len(live), size=n)] + rng.normal(scale=0.6, size=(n, 3))
    q["center"][::7] += rng.normal(scale=30.0, size=(len(q[::7]), 3))
    r = rng.normal(size=(n, 4))
    q["rotation"] = r / np.linalg.norm(r, axis=1, keepdims=True)
    q["size"] = rng.uniform(0.05, 3.0, size=(n, 3))
    q["size"][::5, 1] = np.where(q["shape"][::5] == E.NH_SHAPE_CAPSULE, 0.0, q["size"][::5, 1])          # capsules of half height 0
    q["ignore_body"] = NONE
    q["ignore_body"][::3] = rng.integers(0, 32, size=len(q[::3]))
    return q


def test_a_capsule_of_half_height_zero_gives_the_sphere_querys_bytes():
    scene = S.pile(40, 30, seed=2)
    rec = H.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    rng = np.random.default_rng(71)
    sph = _world_queries(rec, rng, 512)
    sph["shape"] = E.NH_SHAPE_SPHERE
    cap = sph.copy()
    cap["shape"] = E.NH_SHAPE_CAPSULE
    cap["size"][:, 1] = 0.0
    cap["rotation"] = np.nan                                                   # not read
    cap["size"][:, 2] = np.nan
    o0, h0, t0 = H.penetration(rec, nbox, sph)
    o1, h1, t1 = H.penetration(rec, nbox, cap)
    assert t0 == t1 > 256 and o0.tobytes() == o1.tobytes() and h0.tobytes() == h1.tobytes()
    # and the pair functions themselves
    for k in range(64):
        c, p = rng.uniform(-1, 1, size=3), rng.uniform(-1, 1, size=3)
        n0, d0 = H.pen_capsule_sphere(c, (np.nan,) * 4, 0.7, 0.0, p, 0.9)
        n1, d1 = H.pen_sphere_sphere(c, 0.7, p, 0.9)
        assert n0.tobytes() == n1.tobytes() and d0.tobytes() == d1.tobytes()
        qb = _quats(rng, 1, False)[0]
        n0, d0 = H.pen_capsule_box(c, (np.nan,) * 4, 0.7, 0.0, p, qb, (0.5, 0.8, 0.3))
        n1, d1 = H.pen_sphere_box(c, 0.7, p, qb, (0.5, 0.8, 0.3))
        assert n0.tobytes() == n1.tobytes() and d0.tobytes() == d1.tobytes()


def test_sphere_against_box_is_the_radius_less_the_point_distance_to_the_bit():
    rng = np.random.default_rng(72)
    inside = 0
    for k in range(512):
        p = rng.uniform(-3, 3, size=3).astype(np.float32)
        qb = _quats(rng, 1, k % 4 == 0)[0]
        h = rng.uniform(0.05, 2.0, size=3).astype(np.float32)
        c = (p + rng.uniform(-1, 1, size=3) * (h + 1.0)).astype(np.float32)
        r = np.float32(rng.uniform(0.0, 2.0))
        d = H.point_box_distance(c, p, qb, h)
        n, depth = H.pen_sphere_box(c, r, p, qb, h)
        want = np.float32(r - d)
        want = want if want > 0 else np.float32(0.0)
        assert depth.tobytes() == want.tobytes(), (k, depth, want)
        inside += d < 0
        if d < 0:
            assert depth > r                                                   # the centre inside the box: r + the face depth
    assert inside > 50


def _positive_zero(x):
    return np.float32(x).tobytes() == np.float32(0.0).tobytes()


def test_a_touching_pair_has_depth_plus_zero():
    cube = (1.0, 1.0, 1.0)
    # tangent spheres (3-4-5: every square exact)
    n, d = H.pen_sphere_sphere((3, 4, 0), 2.0, (0, 0, 0), 3.0)
    assert _positive_zero(d) and np.array_equal(n, np.float32([0.6, 0.8, 0.0]))
    # a ball on a box face, on an edge (0.375, 0.5 from it: 0.625 away)
    n, d = H.pen_sphere_box((1.5, 0.25, -0.5), 0.5, (0, 0, 0), IDENT, cube)
    assert _positive_zero(d) and np.array_equal(n, np.float32([1, 0, 0]))
    n, d = H.pen_sphere_box((1.375, 1.5, 0.0), 0.625, (0, 0, 0), IDENT, cube)
    assert _positive_zero(d) and np.array_equal(n, np.float32([0.6, 0.8, 0.0]))
    # a box face on a sphere: the normal points from the sphere to the box
    n, d = H.pen_box_sphere((0, 0, 0), IDENT, cube, (0, -1.75, 0), 0.75)
    assert _positive_zero(d) and np.array_equal(n, np.float32([0, 1, 0]))
    # an upright capsule beside a sphere, and with its cap on a box; a flat one lying on a box
    n, d = H.pen_capsule_sphere((2, 0.5, 0), IDENT, 0.5, 1.0, (0, 0, 0), 1.5)
    assert _positive_zero(d) and np.array_equal(n, np.float32([1, 0, 0]))
    n, d = H.pen_capsule_box((0.25, 2.75, 0), IDENT, 0.75, 1.0, (0, 0, 0), IDENT, cube)
    assert _positive_zero(d) and np.array_equal(n, np.float32([0, 1, 0]))
    quarter = (0.0, 0.0, np.float32(np.sqrt(0.5)), np.float32(np.sqrt(0.5)))   # the axis turned to x
    n, d = H.pen_capsule_box((0.25, 1.5, 0), quarter, 0.5, 3.0, (0, 0, 0), IDENT, cube)
    assert d >= 0 and not np.signbit(d) and d < 1e-6 and n[1] > 0.999999
    # box faces in contact: the 2^-20 of the radii is all the depth there is
    n, d = H.pen_box_box((2, 0, 0), IDENT, cube, (0, 0, 0), IDENT, cube)
    assert 0 <= d <= 6 * 2.0 ** -20 and not np.signbit(d) and np.array_equal(n, np.float32([1, 0, 0]))
    # pairs that do not overlap at all: the clamp, never a negative depth or -0
    for n, d in (H.pen_sphere_sphere((9, 0, 0), 1.0, (0, 0, 0), 1.0), H.pen_sphere_box((9, 0, 0), 1.0, (0, 0, 0), IDENT, cube),
                 H.pen_box_sphere((9, 0, 0), IDENT, cube, (0, 0, 0), 1.0), H.pen_capsule_sphere((9, 0, 0), IDENT, 1.0, 1.0, (0, 0, 0), 1.0),
                 H.pen_box_box((9, 0, 0), IDENT, cube, (0, 0, 0), IDENT, cube), H.pen_capsule_box((9, 0, 0), IDENT, 1.0, 1.0, (0, 0, 0), IDENT, cube)):
        assert _positive_zero(d)


def test_named_depths():
    cube = (1.0, 1.0, 1.0)
    # coincident centres: +y for spheres; a ball centred in a box leaves by the nearest face, the lowest axis on equality
    n, d = H.pen_sphere_sphere((1, 2, 3), 0.5, (1, 2, 3), 0.25)
    assert d == 0.75 and np.array_equal(n, np.float32([0, 1, 0]))
    n, d = H.pen_sphere_box((0, 0, 0), 0.5, (0, 0, 0), IDENT, cube)
    assert d == 1.5 and np.array_equal(n, np.float32([1, 0, 0]))
    n, d = H.pen_sphere_box((0.25, -0.5, 0), 0.5, (0, 0, 0), IDENT, (1.0, 1.0, 2.0))
    assert d == 1.0 and np.array_equal(n, np.float32([0, -1, 0]))
    # a capsule whose segment passes through a sphere's centre: a stated perpendicular of the axis
    n, d = H.pen_capsule_sphere((0, 0.5, 0), IDENT, 0.5, 1.0, (0, 0, 0), 0.25)
    assert d == 0.75 and np.array_equal(np.abs(n), np.float32([0, 0, 1]))
    # an upright capsule sunk into the ground slab: out through the top, radius and all
    n, d = H.pen_capsule_box((0.5, 1.25, 0.25), IDENT, 0.5, 1.0, (0, -1, 0), IDENT, (10.0, 1.0, 10.0))
    assert d == 0.25 and np.array_equal(n, np.float32([0, 1, 0]))              # shallow: the lower end point is 0.25 above the slab
    n, d = H.pen_capsule_box((0.5, 0.5, 0.25), IDENT, 0.5, 1.0, (0, -1, 0), IDENT, (10.0, 1.0, 10.0))
    assert d == 1.0 and np.array_equal(n, np.float32([0, 1, 0]))               # deep: the segment reaches 0.5 into the slab
    # a crate pushed 0.25 into a wall
    n, d = H.pen_box_box((1.75, 0, 0), IDENT, cube, (0, 0, 0), IDENT, cube)
    assert abs(d - 0.25) <= 6 * 2.0 ** -20 and np.array_equal(n, np.float32([1, 0, 0]))
    # coincident boxes: the first axis, its + side
    n, d = H.pen_box_box((0, 0, 0), IDENT, (1.0, 2.0, 3.0), (0, 0, 0), IDENT, (1.0, 2.0, 3.0))
    assert abs(d - 2.0) <= 12 * 2.0 ** -20 and np.array_equal(n, np.float32([1, 0, 0]))


# ---- whole worlds on the host ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pile", "compound"])
def test_the_brute_force_penetration_is_the_brute_force_overlap_with_a_richer_record(name):
    scene = S.pile(40, 30, seed=2) if name == "pile" else S.compound(12, seed=6)
    rec = H.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    q = _world_queries(rec, np.random.default_rng(73), 2048)
    q[:4]["shape"] = 7                                                         # invalid queries count 0
    off, hits, total = H.penetration(rec, nbox, q)
    ooff, ohits, ototal = HC.overlap(rec, nbox, q)
    assert total == ototal > 1024 and off.tobytes() == ooff.tobytes()
    assert hits.view(np.uint8).reshape(-1, 32)[:total, 16:].tobytes() == ohits.view(np.uint8).reshape(-1, 16)[:total].tobytes()
    counts = np.diff(off.astype(np.int64))
    assert (counts > 1).mean() > 0.1 and (counts == 0).mean() > 0.05 and not counts[:4].any()
    d, n = hits["depth"][:total], hits["normal"][:total]
    assert (d >= 0).all() and not np.signbit(d).any() and np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-5
    # every record is the pair function of its query and its collider
    query = np.repeat(np.arange(len(q)), counts)
    comb = hits["collider"][:total].astype(np.int64) + np.where(hits["shape"][:total] == E.NH_SHAPE_BOX, 0, nbox)
    ok, pn, pd = H.pairs(q[query], rec[comb], comb < nbox)
    assert ok.all() and pn.tobytes() == n.tobytes() and pd.tobytes() == d.tobytes()
    # the capacity rule with 32-byte records: a prefix of whole segments, every byte behind it untouched
    sentinel = np.frombuffer(b"\xa5" * 32 * total, dtype=H.HIT)
    for cap in (0, int(off[len(q) // 2]), int(off[len(q) // 2]) + 1, total - 1, total):
        written = int(off[np.searchsorted(off, cap, side="right") - 1])
        got = sentinel.copy()
        o2, got, t2 = H.penetration(rec, nbox, q, capacity=cap, hits=got)
        assert o2.tobytes() == off.tobytes() and t2 == total
        assert got[:written].tobytes() == hits[:written].tobytes() and got[written:].tobytes() == sentinel[written:].tobytes(), cap
