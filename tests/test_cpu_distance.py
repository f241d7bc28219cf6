"""Distance queries on the host (no GPU): nh_distance's declaration, exports and wrappers; the six pair functions of nudge_amd/csrc/nh_query.h
("distance") -- built for the host by tests/hostdistance_util.py, the device's bits -- against independent float64 values, their witnesses, the existing
cast oracles, and the brute-force oracle of the GPU tests on hand-made worlds.

THE FLOAT64 VALUES share nothing with the code under test:
    sphere/sphere   |c - p| - R - r
    sphere/box      the length of the centre minus its clamp to the box, - r;  box/sphere likewise from the query box, - R
    capsule/sphere  the distance from p to the segment (closed form), - R - r
    capsule/box     the distance from the segment to the box, - r: dist(ol + u al, box)^2 is convex and piecewise quadratic in u, with breakpoints where a
                    coordinate crosses -+h, so its minimum is the least of the closed-form minima of its (at most 7) pieces
    box/box         a SANDWICH: the 15-axis SAT gap (a lower bound of the distance: every axis separates by at most the distance) and the distance of the
                    two points that alternating projections (clamp into A, clamp into B, iterated) end on (an upper bound: both points are in the boxes)

THE TOLERANCES are relative to the pair's scale (every half extent, radius and half height, plus the centre distance).  MEASURED on the seeded inputs
below with the host build, the worst deviation of the float32 result from the float64 value (for box / box: beyond either end of the sandwich), as
distance / the collider's witness / the query shape's witness / |normal| - 1:
    sphere/sphere   1.09e-07  5.95e-08  8.77e-08  1.12e-07        capsule/sphere  1.23e-07  6.65e-08  1.22e-07  1.20e-07
    sphere/box      1.71e-07  9.28e-08  3.25e-07  2.25e-07        capsule/box     1.90e-07  1.43e-07  2.92e-07  3.01e-07
    box/sphere      1.98e-07  5.69e-08  3.03e-07  2.55e-07        box/box         2.24e-07  2.58e-07  3.62e-07  3.20e-07
MEASURED_PAIR = 2.24e-7 is the worst deviation of the distance; the witnesses and |normal| are held to the same tolerance, 4 x that, which their own worst
(3.62e-7) meets.  Against the casts along -normal, the worst |t - distance|: sphere casts 1.79e-07, capsule casts 3.20e-07,
box casts 7.07e-07 (their radii carry 2^-20): MEASURED_CAST = 7.07e-7.  The tests assert 4 x the measured worst: rounding differs between seeds, and the
margin has to absorb that."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostcapsule_util as HC               # noqa: E402
import hostcast_util as CAST                 # noqa: E402
import hostdistance_util as D               # noqa: E402
import hostpoint_util as HP                 # noqa: E402
import hostquery_util as Q                  # noqa: E402
from volume_records import distance_bases, distance_lists      # noqa: E402
from nudge_amd import engine as E           # noqa: E402

NONE = 0xFFFFFFFF
IDENT = (0.0, 0.0, 0.0, 1.0)
MEASURED_PAIR = 2.24e-7
MEASURED_CAST = 7.07e-7
TOL = 4 * MEASURED_PAIR
TOL_CAST = 4 * MEASURED_CAST
KINDS = ("sphere/sphere", "sphere/box", "box/sphere", "capsule/sphere", "capsule/box", "box/box")
N_PAIRS = 1200


# ---- 1. the declaration ----------------------------------------------------------------------------------------------------------------------
def test_the_call_is_declared_exported_and_wrapped(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "nudge_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "int nh_distance(nh_context* ctx, const nh_DistanceQuery* queries, uint32_t count, nh_PointHit* hits, uint32_t flags );" in flat
    assert "nh_distance" in E.EXPORTS
    syms = subprocess.check_output(["nm", "-D", "--defined-only", E._LIB_PATH], text=True)
    assert re.search(r"\bT nh_distance$", syms, flags=re.M)
    assert list(inspect.signature(E.World.distance_records).parameters) == ["self", "queries", "hits"]
    assert list(inspect.signature(E.World.distance).parameters) == ["self", "centres", "radii", "half_extents", "rotations", "half_heights", "max_distance",
                                                                    "ignore_body", "synchronize"]
    sig = inspect.signature(E.World.distance).parameters
    assert sig["max_distance"].default == float("inf") and sig["synchronize"].default is False and sig["radii"].default is None
    # the sentences that named the gap are gone
    assert "(GJK)" not in hdr
    # nh_DistanceQuery: 64 bytes whose first 48 are an nh_OverlapQuery, as gcc lays it out and as the numpy record has it
    ms = ("center", "shape", "rotation", "size", "ignore_body", "max_distance", "reserved")
    body = "".join(f'  printf("%zu %zu\\n", sizeof(nh_DistanceQuery), offsetof(nh_DistanceQuery, {m}));\n' for m in ms)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nudge_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    for k, m in enumerate(ms):
        size, off = (int(v) for v in lines[k].split())
        assert size == E.DISTANCE_QUERY.itemsize == 64
        assert off == E.DISTANCE_QUERY.fields[m][1], (m, off)
        if m in E.OVERLAP_QUERY.fields:
            assert off == E.OVERLAP_QUERY.fields[m][1]


# ---- seeded pairs --------------------------------------------------------------------------------------------------------------------------
def _quats(rng, n, identity=False):
    if identity:
        return np.tile(np.float32(IDENT), (n, 1))
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def _empty(kind, n):
    qs, cs = kind.split("/")
    q = np.zeros(n, dtype=E.DISTANCE_QUERY)
    q["shape"] = {"sphere": E.NH_SHAPE_SPHERE, "box": E.NH_SHAPE_BOX, "capsule": E.NH_SHAPE_CAPSULE}[qs]
    q["ignore_body"], q["max_distance"] = NONE, np.inf
    return q, np.zeros(n, dtype=Q.REC), np.full(n, cs == "box")


def _random_pairs(kind, n, seed, world=(0.0, 0.0, 0.0), identity=False):
    """n pairs of one kind.  Sizes 0.05 to 4; the collider's centre within 0.5 of `world`; the query's centre = the collider's plus a random direction
    times 0 .. 3 of the sum of both bounding radii -- so some overlap, some touch nearly, most are apart."""
    rng = np.random.default_rng(seed)
    qs, cs = kind.split("/")
    q, r, box = _empty(kind, n)
    size = lambda *shape: rng.uniform(0.05, 4.0, size=shape).astype(np.float32)          # noqa: E731
    q["rotation"], r["q"] = _quats(rng, n, identity), _quats(rng, n, identity)
    if qs == "box":
        q["size"] = size(n, 3)
    else:
        q["size"][:, 0] = size(n)
        if qs == "capsule":
            q["size"][:, 1] = size(n)
    r["h"] = size(n, 3) if cs == "box" else np.repeat(size(n, 1), 3, axis=1)
    r["p"] = (np.asarray(world, np.float64) + rng.uniform(-0.5, 0.5, size=(n, 3))).astype(np.float32)
    ra = np.linalg.norm(q["size"], axis=1) if qs == "box" else q["size"][:, 0] + q["size"][:, 1]
    rb = np.linalg.norm(r["h"], axis=1) if cs == "box" else r["h"][:, 0]
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    q["center"] = (r["p"] + u * (rng.uniform(0, 3, size=n) * (ra + rb))[:, None]).astype(np.float32)
    return q, r, box


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.float32(np.append(axis * np.sin(angle / 2), np.cos(angle / 2)))


def _crafted_boxes(seed):
    """Box / box pairs with known closest features, each at gaps from 1e-4 to 1e3 and touching (gap 0): faces parallel, face over face; crossing edges;
    vertex against vertex; vertex against edge; edges within 1e-3 rad of parallel; a flat box (one half extent 0) on either side; sizes 1 : 1000."""
    rng = np.random.default_rng(seed)
    gaps = [0.0] + list(10.0 ** np.arange(-4, 4))
    rows = []

    def add(ca, qa, ha, cb, qb, hb):
        rows.append((np.float32(ca), np.float32(qa), np.float32(ha), np.float32(cb), np.float32(qb), np.float32(hb)))

    s2, s3 = np.sqrt(2.0), np.sqrt(3.0)
    # the rotation that turns the body diagonal (1, 1, 1) to -y: a vertex points down
    diag = np.array([1.0, 1.0, 1.0]) / s3
    ax = np.cross(diag, [0.0, -1.0, 0.0])
    down = _rot(ax, np.arccos(np.clip(np.dot(diag, [0.0, -1.0, 0.0]), -1, 1)))
    for g in gaps:
        for _ in range(6):
            ha, hb = rng.uniform(0.05, 4.0, size=3), rng.uniform(0.05, 4.0, size=3)
            cb = rng.uniform(-0.2, 0.2, size=3)
            slide = rng.uniform(-0.5, 0.5, size=3)
            # faces parallel, face over face (on a random axis), the query box slid along the face
            k = rng.integers(0, 3)
            off = slide * np.minimum(ha, hb)
            off[k] = ha[k] + hb[k] + g
            add(cb + off, IDENT, ha, cb, IDENT, hb)
            # crossing edges: a cube turned 45 degrees about x over a cube turned 45 degrees about z
            a, b = rng.uniform(0.05, 4.0), rng.uniform(0.05, 4.0)
            add(cb + [0.1 * a * slide[0], (a + b) * s2 + g, 0.1 * b * slide[2]], _rot([1, 0, 0], np.pi / 4), [a, a, a], cb, _rot([0, 0, 1], np.pi / 4), [b, b, b])
            # vertex against vertex: two upright boxes apart on all three axes
            add(cb + ha + hb + g / s3, IDENT, ha, cb, IDENT, hb)
            # vertex against edge: a cube on its vertex over the top edge of a cube turned 45 degrees about z
            add(cb + [0.0, b * s2 + g + a * s3, 0.2 * b * slide[2]], down, [a, a, a], cb, _rot([0, 0, 1], np.pi / 4), [b, b, b])
            # edges within 1e-3 rad of parallel: upright boxes apart on x and y, the query turned by a small angle about a random axis
            add(cb + [ha[0] + hb[0] + g / s2, ha[1] + hb[1] + g / s2, 0.3 * slide[2]], _rot(rng.normal(size=3), rng.uniform(0, 1e-3)), ha, cb, IDENT, hb)
            # a flat box on either side, at random rotations
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            flat = ha.copy()
            flat[rng.integers(0, 3)] = 0.0
            reach = np.linalg.norm(flat) + np.linalg.norm(hb)
            add(cb + u * (0.6 * reach + g), _quats(rng, 1)[0], flat, cb, _quats(rng, 1)[0], hb)
            add(cb + u * (0.6 * reach + g), _quats(rng, 1)[0], hb, cb, _quats(rng, 1)[0], flat)
            # sizes 1 : 1000, either way round
            add(cb + u * (0.7 * np.linalg.norm(hb) + g), _quats(rng, 1)[0], ha * 1e-3, cb, _quats(rng, 1)[0], hb)
            add(cb + u * (0.7 * np.linalg.norm(hb) + g), _quats(rng, 1)[0], hb, cb, _quats(rng, 1)[0], ha * 1e-3)
    q, r, box = _empty("box/box", len(rows))
    for i, (ca, qa, ha, cb, qb, hb) in enumerate(rows):
        q["center"][i], q["rotation"][i], q["size"][i], r["p"][i], r["q"][i], r["h"][i] = ca, qa, ha, cb, qb, hb
    return q, r, box


def _crafted_round(kind, seed):
    """The sphere and capsule pairs at gaps from 1e-4 to 1e3 and touching, and with sizes 1 : 1000."""
    rng = np.random.default_rng(seed)
    q, r, box = _random_pairs(kind, 9 * 40, seed)
    gaps = np.repeat([0.0] + list(10.0 ** np.arange(-4, 4)), 40)
    small = rng.random(len(q)) < 0.3
    q["size"][small] *= np.float32(1e-3)
    r["p"] *= np.float32(0.02)
    # a sphere collider, or a sphere query: place the pair at the gap along a random direction from the other shape's surface point
    qs, cs = kind.split("/")
    u = rng.normal(size=(len(q), 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    if cs == "sphere" and qs == "sphere":
        q["center"] = (r["p"] + u * (r["h"][:, 0] + q["size"][:, 0] + gaps)[:, None]).astype(np.float32)
    elif qs == "sphere":
        # over a face of the box: along the box's own x axis
        m = _mats(r["q"])
        q["center"] = (r["p"] + m[:, :, 0] * (r["h"][:, 0] + q["size"][:, 0] + gaps)[:, None]).astype(np.float32)
    elif cs == "sphere" and qs == "box":
        m = _mats(q["rotation"])
        q["center"] = (r["p"] + m[:, :, 1] * (r["h"][:, 0] + q["size"][:, 1] + gaps)[:, None]).astype(np.float32)
    elif cs == "sphere":
        # beside the capsule's axis (local x is perpendicular to it)
        m = _mats(q["rotation"])
        q["center"] = (r["p"] + m[:, :, 0] * (r["h"][:, 0] + q["size"][:, 0] + gaps)[:, None]).astype(np.float32)
    else:
        # a capsule lying along the box's z axis over its +x face
        q["rotation"] = _qmul(r["q"], np.tile(_rot([1, 0, 0], np.pi / 2), (len(q), 1)))
        m = _mats(r["q"])
        q["center"] = (r["p"] + m[:, :, 0] * (r["h"][:, 0] + q["size"][:, 0] + gaps)[:, None]).astype(np.float32)
    return q, r, box


def _qmul(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    av, bv = a[:, :3], b[:, :3]
    v = a[:, 3:] * bv + b[:, 3:] * av + np.cross(av, bv)
    s = a[:, 3] * b[:, 3] - (av * bv).sum(axis=1)
    return np.concatenate([v, s[:, None]], axis=1).astype(np.float32)


def _inputs(kind):
    """Every seeded input of a kind: random pairs near the origin, at random rotations and upright, the crafted ones -- and N_PAIRS random pairs far from the origin; the fourth
    array returned says which pairs those are.  A witness is a position in the world and is written on the float grid of its coordinates (2^-24 of 300 is 1.8e-5, whatever
    the pair's scale), so the far pairs check the distance, which is formed from differences, and not the witnesses."""
    sets = [_random_pairs(kind, N_PAIRS, 11 + 7 * KINDS.index(kind)), _random_pairs(kind, N_PAIRS // 2, 13 + 7 * KINDS.index(kind), identity=True)]
    sets.append(_crafted_boxes(99) if kind == "box/box" else _crafted_round(kind, 98))
    far = [np.zeros(len(s[0]), dtype=bool) for s in sets] + [np.ones(N_PAIRS, dtype=bool)]
    sets.append(_random_pairs(kind, N_PAIRS, 12 + 7 * KINDS.index(kind), world=(300.0, -40.0, 120.0)))
    return tuple(np.concatenate([s[k] for s in sets]) for k in range(3)) + (np.concatenate(far),)


# ---- the float64 side ------------------------------------------------------------------------------------------------------------------------
def _mats(q):
    x, y, z, s = (q[:, k].astype(np.float64) for k in range(4))
    m = np.empty((len(q), 3, 3))
    m[:, 0, 0], m[:, 0, 1], m[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y)
    m[:, 1, 0], m[:, 1, 1], m[:, 1, 2] = 2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)
    m[:, 2, 0], m[:, 2, 1], m[:, 2, 2] = 2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)
    return m


def _to_frame(m, c, x):
    return np.einsum("nji,nj->ni", m, x - c)


def _box_sdf(m, c, h, x):
    """The signed distance of x from the box (m, c, h): negative inside."""
    l = np.abs(_to_frame(m, c, x)) - h
    return np.linalg.norm(np.maximum(l, 0.0), axis=1) + np.minimum(l.max(axis=1), 0.0)


def _segment_point(c, a, x):
    aa = (a * a).sum(axis=1)
    u = np.clip(np.where(aa > 0, ((x - c) * a).sum(axis=1) / np.where(aa > 0, aa, 1.0), 0.0), -1.0, 1.0)
    return np.linalg.norm(c + u[:, None] * a - x, axis=1)


def _segment_box(ol, al, h):
    """The distance from the segment ol + u al, u in [-1, 1], to the box [-h, h]: the least closed-form minimum over the pieces of u."""
    n = len(ol)
    with np.errstate(divide="ignore", invalid="ignore"):
        cuts = np.concatenate([(s * h - ol) / al for s in (-1.0, 1.0)], axis=1)
    cuts = np.where(np.isfinite(cuts), np.clip(cuts, -1.0, 1.0), 1.0)
    cuts = np.sort(np.concatenate([np.full((n, 1), -1.0), cuts, np.full((n, 1), 1.0)], axis=1), axis=1)
    best = np.full(n, np.inf)
    for k in range(cuts.shape[1] - 1):
        lo, hi = cuts[:, k], cuts[:, k + 1]
        x = ol + (0.5 * (lo + hi))[:, None] * al
        s = np.where(x > h, 1.0, np.where(x < -h, -1.0, 0.0))          # which side of which slab this piece is on
        o = (ol - s * h) * (s != 0)
        a = al * (s != 0)
        aa = (a * a).sum(axis=1)
        u = np.clip(np.where(aa > 0, -(o * a).sum(axis=1) / np.where(aa > 0, aa, 1.0), lo), lo, hi)
        best = np.minimum(best, np.linalg.norm(o + u[:, None] * a, axis=1))
    return best


def _sat_gap(A, ca, ha, B, cb, hb):
    """The largest separation over the 15 axes (negative where none separates): a lower bound of the distance of two boxes."""
    d = cb - ca
    axes = [A[:, :, k] for k in range(3)] + [B[:, :, k] for k in range(3)] + [np.cross(A[:, :, i], B[:, :, j]) for i in range(3) for j in range(3)]
    best = np.full(len(d), -np.inf)
    for L in axes:
        ln = np.linalg.norm(L, axis=1)
        ok = ln > 1e-9
        Ln = L / np.where(ok, ln, 1.0)[:, None]
        ra = (np.abs(np.einsum("nik,ni->nk", A, Ln)) * ha).sum(axis=1)
        rb = (np.abs(np.einsum("nik,ni->nk", B, Ln)) * hb).sum(axis=1)
        gap = np.abs((d * Ln).sum(axis=1)) - ra - rb
        best = np.where(ok, np.maximum(best, gap), best)
    return best


def _alternating(A, ca, ha, B, cb, hb, rounds=400):
    """The distance of the two points alternating projections end on: x in A, y in B -- an upper bound of the distance of the boxes."""
    def into(m, c, h, x):
        return c + np.einsum("nij,nj->ni", m, np.clip(_to_frame(m, c, x), -h, h))
    x = into(A, ca, ha, cb)
    for _ in range(rounds):
        y = into(B, cb, hb, x)
        x = into(A, ca, ha, y)
    return np.linalg.norm(x - into(B, cb, hb, x), axis=1)


def _f64(q, r):
    return (q["center"].astype(np.float64), _mats(q["rotation"]), q["size"].astype(np.float64), r["p"].astype(np.float64), _mats(r["q"]),
            r["h"].astype(np.float64))


def _bounds(kind, q, r):
    """(lower, upper) float64 bounds of the separation of every pair: equal but for box / box."""
    ca, A, sa, cb, B, hb = _f64(q, r)
    qs, cs = kind.split("/")
    a = A[:, :, 1] * sa[:, 1:2]                                  # a capsule's half axis: its local y
    if kind == "sphere/sphere":
        d = np.linalg.norm(ca - cb, axis=1) - hb[:, 0] - sa[:, 0]
    elif kind == "sphere/box":
        d = _box_sdf(B, cb, hb, ca) - sa[:, 0]
    elif kind == "box/sphere":
        d = _box_sdf(A, ca, sa, cb) - hb[:, 0]
    elif kind == "capsule/sphere":
        d = _segment_point(ca, a, cb) - hb[:, 0] - sa[:, 0]
    elif kind == "capsule/box":
        d = _segment_box(_to_frame(B, cb, ca), np.einsum("nji,nj->ni", B, a), hb) - sa[:, 0]
    else:
        return _sat_gap(A, ca, sa, B, cb, hb), _alternating(A, ca, sa, B, cb, hb)
    return d, d


def _scale(kind, q, r):
    qs, cs = kind.split("/")
    sa = q["size"].astype(np.float64)
    s = sa.sum(axis=1) if qs == "box" else sa[:, 0] + (sa[:, 1] if qs == "capsule" else 0.0)
    s = s + (r["h"].astype(np.float64).sum(axis=1) if cs == "box" else r["h"][:, 0].astype(np.float64))
    return s + np.linalg.norm(q["center"].astype(np.float64) - r["p"].astype(np.float64), axis=1)


def _query_sdf(kind, q, x):
    """The signed distance of the points x from the query shapes."""
    ca, A, sa = q["center"].astype(np.float64), _mats(q["rotation"]), q["size"].astype(np.float64)
    qs = kind.split("/")[0]
    if qs == "sphere":
        return np.linalg.norm(x - ca, axis=1) - sa[:, 0]
    if qs == "box":
        return _box_sdf(A, ca, sa, x)
    return _segment_point(ca, A[:, :, 1] * sa[:, 1:2], x) - sa[:, 0]


def _collider_sdf(kind, r, x):
    cb, B, hb = r["p"].astype(np.float64), _mats(r["q"]), r["h"].astype(np.float64)
    return _box_sdf(B, cb, hb, x) if kind.endswith("/box") else np.linalg.norm(x - cb, axis=1) - hb[:, 0]


# ---- 2. and 3. the pair functions and their witnesses against float64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_the_pair_function_and_its_witnesses_match_float64(kind):
    q, r, box, far = _inputs(kind)
    d, n, x = D.pairs(q, r, box)
    lo, hi = _bounds(kind, q, r)
    scale = _scale(kind, q, r)
    apart = d > 0
    assert apart.mean() > 0.3 and (~apart).mean() > 0.05, "the inputs hold both kinds of record"
    # the overlap record: distance 0, normal = point = 0, never a negative or NaN value; and a unit normal iff the record is a separated one
    assert np.all(d >= 0) and not np.any(np.signbit(d))
    assert np.all(n[~apart] == 0) and np.all(x[~apart] == 0)
    nn = np.linalg.norm(n[apart].astype(np.float64), axis=1)
    # the distance: within the float64 bounds (an overlap record claims a separation <= 0)
    dev = np.where(apart, np.maximum(np.maximum(lo - d, d - hi), 0.0), np.maximum(lo, 0.0)) / scale
    # the witnesses: `point` on the collider's surface, point + distance normal on the query shape's
    xa = x.astype(np.float64) + d.astype(np.float64)[:, None] * n.astype(np.float64)
    near = apart & ~far
    wb = np.abs(_collider_sdf(kind, r, x.astype(np.float64)))[near] / scale[near]
    wa = np.abs(_query_sdf(kind, q, xa))[near] / scale[near]
    print(f"{kind}: {len(q)} pairs, {int(apart.sum())} apart; worst deviation of the distance {dev.max():.2e}, of the collider witness {wb.max():.2e}, "
          f"of the query witness {wa.max():.2e}, of |normal| - 1 {np.abs(nn - 1).max():.2e} (of the scale; asserted below {TOL:.1e})")
    assert dev.max() <= TOL, int(np.argmax(dev))
    assert wb.max() <= TOL and wa.max() <= TOL
    assert np.abs(nn - 1).max() <= TOL


# ---- 4. agreement with the casts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_cast_along_the_normal_arrives_after_the_distance(kind):
    """The query shape cast along -normal through the existing cast oracles reaches that collider at t = distance: no direction gets there sooner (the
    distance of convex shapes is 1-Lipschitz in a translation), and along the witnesses' direction it gets there exactly then."""
    q, r, box = _random_pairs(kind, 400, 500 + KINDS.index(kind))
    d, n, x = D.pairs(q, r, box)
    scale = _scale(kind, q, r)
    qs, cs = kind.split("/")
    worst, seen = 0.0, 0
    for i in np.nonzero(d > 0)[0]:
        o, dirn = q["center"][i], -n[i]
        if qs == "sphere":
            t, _, hit = (CAST.sweep_box(o, dirn, q["size"][i, 0], r["p"][i], r["q"][i], r["h"][i]) if box[i] else
                         CAST.sweep_sphere(o, dirn, q["size"][i, 0], r["p"][i], r["h"][i, 0]))
        elif qs == "box":
            t, _, hit = (CAST.sweep_box_box(o, dirn, q["rotation"][i], q["size"][i], r["p"][i], r["q"][i], r["h"][i]) if box[i] else
                         CAST.sweep_box_sphere(o, dirn, q["rotation"][i], q["size"][i], r["p"][i], r["h"][i, 0]))
        else:
            t, _, hit = (HC.sweep_capsule_box(o, dirn, q["rotation"][i], q["size"][i, 0], q["size"][i, 1], r["p"][i], r["q"][i], r["h"][i]) if box[i] else
                         HC.sweep_capsule_sphere(o, dirn, q["rotation"][i], q["size"][i, 0], q["size"][i, 1], r["p"][i], r["h"][i, 0]))
        assert hit, (kind, int(i))
        worst = max(worst, abs(float(t) - float(d[i])) / scale[i])
        seen += 1
    print(f"{kind}: {seen} casts along -normal; worst |t - distance| {worst:.2e} of the scale (asserted below {TOL_CAST:.1e})")
    assert seen > 100 and worst <= TOL_CAST


# ---- 5. the oracle's rules on hand-made worlds --------------------------------------------------------------------------------------------------
def _world(colliders):
    """Records of hand-made colliders, boxes first: ("box" | "sphere", position, half extents | radius, body, rotation=identity)."""
    colliders = sorted(colliders, key=lambda c: c[0] != "box")
    rec = np.zeros(len(colliders), dtype=Q.REC)
    for i, c in enumerate(colliders):
        rec["p"][i], rec["body"][i], rec["tag"][i] = c[1], c[3], 100 + i
        rec["h"][i] = c[2] if c[0] == "box" else (c[2], c[2], c[2])
        rec["q"][i] = c[4] if len(c) > 4 else IDENT
    return rec, sum(c[0] == "box" for c in colliders)


def _miss(h, distance):
    assert h["shape"] == NONE and h["body"] == NONE and h["collider"] == NONE and h["tag"] == NONE and h["reserved"] == 0
    assert np.all(h["normal"] == 0) and np.all(h["point"] == 0)
    assert (np.isnan(h["distance"]) and np.isnan(distance)) or h["distance"] == np.float32(distance)


def test_ties_go_to_the_lower_combined_index():
    # two equal spheres at mirrored places: the first; a box and a sphere at the same distance: the box
    rec, nbox = _world([("sphere", (3, 0, 0), 1.0, 1), ("sphere", (-3, 0, 0), 1.0, 2)])
    for qq in (D.queries([(0, 0, 0)], radii=0.5), D.queries([(0, 0, 0)], half_extents=(0.5, 0.5, 0.5)), D.queries([(0, 0, 0)], radii=0.5, half_heights=0.25)):
        h = D.distance(rec, nbox, qq)[0]
        assert h["distance"] == 1.5 and h["collider"] == 0 and h["shape"] == E.NH_SHAPE_SPHERE and h["body"] == 1 and h["tag"] == 100
        assert D.distance(rec[::-1].copy(), nbox, qq)[0]["body"] == 2
    rec, nbox = _world([("sphere", (3, 0, 0), 1.0, 1), ("box", (-3, 0, 0), (1, 1, 1), 2)])
    h = D.distance(rec, nbox, D.queries([(0, 0, 0)], radii=0.5))[0]
    assert h["distance"] == 1.5 and h["shape"] == E.NH_SHAPE_BOX and h["body"] == 2 and tuple(h["normal"]) == (1, 0, 0) and tuple(h["point"]) == (-2, 0, 0)


def test_max_distance_cuts_at_the_key_exactly():
    rec, nbox = _world([("box", (5, 0.3, -0.2), (1, 2, 3), 1, _rot([1, 2, 3], 0.7)), ("sphere", (-40, 0, 0), 1.0, 2)])
    for shape in (dict(radii=0.5), dict(half_extents=(0.3, 0.4, 0.5), rotations=_rot([3, 1, 2], 1.1)), dict(radii=0.25, half_heights=0.75, rotations=_rot([0, 0, 1], 0.4))):
        key = D.distance(rec, nbox, D.queries([(0, 0, 0)], **shape))[0]["distance"]
        assert 1.0 < key < 5.0
        below = np.nextafter(key, np.float32(0))
        at = D.distance(rec, nbox, D.queries([(0, 0, 0)], max_distance=key, **shape))[0]
        assert at["distance"] == key and at["body"] == 1
        _miss(D.distance(rec, nbox, D.queries([(0, 0, 0)], max_distance=below, **shape))[0], below)
        above = D.distance(rec, nbox, D.queries([(0, 0, 0)], max_distance=np.nextafter(key, np.float32(np.inf)), **shape))[0]
        assert above.tobytes() == at.tobytes()
        # +inf finds the far sphere when the box is ignored; 0 finds only what the shape touches
        far = D.distance(rec, nbox, D.queries([(0, 0, 0)], ignore_body=1, **shape))[0]
        assert far["body"] == 2 and far["distance"] > 30
        _miss(D.distance(rec, nbox, D.queries([(0, 0, 0)], max_distance=0.0, **shape))[0], 0.0)
        touch = D.distance(rec, nbox, D.queries([(4.2, 0.3, -0.2)], max_distance=0.0, **shape))[0]
        assert touch["distance"] == 0 and touch["body"] == 1 and np.all(touch["normal"] == 0) and np.all(touch["point"] == 0)


def test_the_overlap_record_and_what_is_never_reported():
    nan = np.float32(np.nan)
    rec, nbox = _world([("box", (0, 0, 0), (1, 1, 1), 1), ("box", (nan, nan, nan), (1, 1, 1), 9, (nan, nan, nan, nan)), ("sphere", (6, 0, 0), 1.0, 2),
                        ("sphere", (nan, nan, nan), 1.0, 9)])
    for shape in (dict(radii=0.5), dict(half_extents=(0.5, 0.5, 0.5)), dict(radii=0.5, half_heights=0.5)):
        # inside the box, over its face and touching the sphere: the overlap record, with the identity of the lowest index that overlaps
        for c, body in (((0.2, 0.1, 0), 1), ((1.4, 0, 0), 1), ((6, 1.5, 0), 2)):
            h = D.distance(rec, nbox, D.queries([c], **shape))[0]
            assert h["distance"] == 0 and not np.signbit(h["distance"]) and np.all(h["normal"] == 0) and np.all(h["point"] == 0)
            assert h["body"] == body and h["reserved"] == 0 and h["tag"] in (100, 102)
        # a collider of a NaN pose is never reported: alone in the world it is a miss
        _miss(D.distance(rec[[1, 3]].copy(), 1, D.queries([(0, 0, 0)], **shape))[0], np.inf)
        # ignore_body: the box ignored, the sphere is what is left
        h = D.distance(rec, nbox, D.queries([(0.2, 0.1, 0)], ignore_body=1, **shape))[0]
        assert h["body"] == 2 and h["distance"] > 3 and abs(np.linalg.norm(h["normal"]) - 1) < 1e-6
        # the empty world
        _miss(D.distance(rec[:0], 0, D.queries([(0, 0, 0)], max_distance=7.0, **shape))[0], 7.0)


def test_every_kind_of_invalid_query_writes_the_nan_miss():
    rec, nbox = _world([("box", (0, 0, 0), (1, 1, 1), 1), ("sphere", (6, 0, 0), 1.0, 2)])
    for base in distance_bases():
        assert D.distance(rec, nbox, base)[0]["body"] in (1, 2)
    bad, ok = distance_lists()
    assert len(bad) == 3 * 8 + 2 * 3 + 1
    for qq in bad:
        _miss(D.distance(rec, nbox, qq)[0], np.nan)
    # what is not read does not spoil: a sphere's rotation and size[1..2], a capsule's size[2], reserved
    assert len(ok) == 2
    for qq, base in ok:
        assert D.distance(rec, nbox, qq).tobytes() == D.distance(rec, nbox, base).tobytes()


def _random_world(seed, n=300):
    rng = np.random.default_rng(seed)
    nbox = n // 2
    rec = np.zeros(n, dtype=Q.REC)
    rec["p"], rec["q"] = rng.uniform(-10, 10, size=(n, 3)), _quats(rng, n)
    rec["h"][:nbox] = rng.uniform(0.1, 1.5, size=(nbox, 3))
    rec["h"][nbox:] = rng.uniform(0.1, 1.5, size=(n - nbox, 1))
    rec["body"], rec["tag"] = np.arange(n) // 2, rng.integers(0, 1 << 30, size=n)
    return rec, nbox, rng


def test_identity_a_capsule_of_half_height_0_is_the_sphere_query():
    rec, nbox, rng = _random_world(31)
    c = rng.uniform(-12, 12, size=(2000, 3))
    radii = rng.uniform(0, 1.0, size=2000)
    for md in (np.inf, 1.0):
        sph = D.distance(rec, nbox, D.queries(c, radii=radii, max_distance=md))
        cap = D.queries(c, radii=radii, half_heights=0.0, max_distance=md)
        cap["rotation"] = np.nan                                   # (not read)
        assert D.distance(rec, nbox, cap).tobytes() == sph.tobytes()
    assert (sph["shape"] == NONE).any() and (sph["distance"] == 0).any() and ((sph["distance"] > 0) & (sph["shape"] != NONE)).any()


def test_identity_a_sphere_of_radius_0_is_nh_closest_where_that_is_positive():
    rec, nbox, rng = _random_world(32)
    c = rng.uniform(-12, 12, size=(4000, 3)).astype(np.float32)
    ignore = np.where(rng.random(4000) < 0.3, rng.integers(0, 150, size=4000), NONE).astype(np.uint32)
    for md in (np.inf, 1.5):
        pq = np.zeros(4000, dtype=E.POINT_QUERY)
        pq["point"], pq["max_distance"], pq["ignore_body"] = c, md, ignore
        near = HP.closest(rec, nbox, pq)
        got = D.distance(rec, nbox, D.queries(c, radii=0.0, max_distance=md, ignore_body=ignore))
        pos = near["distance"] > 0
        assert pos.sum() > 1000 and (~pos).sum() > 100
        assert got[pos].tobytes() == near[pos].tobytes()
        # inside a collider nh_closest is negative and nh_distance writes the overlap record of the lowest index that contains the point
        inside = near["distance"] < 0
        assert np.all(got["distance"][inside] == 0) and np.all(got["normal"][inside] == 0)


def test_the_brute_force_is_the_least_key_of_the_single_collider_answers():
    """hd_distance over a world against hd_distance of every collider alone (`only`): the least key, the lowest index among equals."""
    rec, nbox, rng = _random_world(33, n=40)
    c = rng.uniform(-12, 12, size=(60, 3))
    for qq in (D.queries(c, radii=rng.uniform(0, 1, 60)), D.queries(c, half_extents=rng.uniform(0.1, 1, (60, 3)), rotations=_quats(rng, 60)),
               D.queries(c, radii=rng.uniform(0, 1, 60), half_heights=rng.uniform(0, 1, 60), rotations=_quats(rng, 60), max_distance=4.0)):
        whole = D.distance(rec, nbox, qq)
        alone = np.stack([D.distance(rec, nbox, qq, only=k) for k in range(len(rec))])          # (collider, query)
        keys = np.where(alone["shape"] == NONE, np.inf, alone["distance"])
        first = keys.argmin(axis=0)
        for i in range(len(qq)):
            want = alone[first[i], i] if np.isfinite(keys[first[i], i]) else alone[0, i]
            assert whole[i].tobytes() == want.tobytes(), i
