"""Scene queries on the host (no GPU): the ABI records of include/nudge_hip.h against their Python mirrors, and the per-item arithmetic of
nudge_amd/csrc/nh_query.h -- built for the host by tests/hostquery_util.py, the same bits as the device -- against float64 closed forms and the
named cases of its exact semantics (ties, zero direction components, max_t, ignore_body, inside origins, non-unit directions)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostcast_util as CAST                 # noqa: E402
import hostquery_util as Q                   # noqa: E402
from query_util import unit_quats as _unit_quats      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

NONE = 0xFFFFFFFF


def test_ray_records_match_the_header(tmp_path):
    """nh_Ray / nh_RayHit: size and every member offset as gcc lays them out, against the ctypes mirrors and the numpy records."""
    members = {"nh_Ray": ("origin", "max_t", "direction", "ignore_body"), "nh_RayHit": ("t", "normal", "body", "collider", "shape", "tag")}
    body = "".join(f'  printf("%zu %zu\\n", sizeof({c}), offsetof({c}, {m}));\n' for c, ms in members.items() for m in ms)
    body += '  printf("%u %u %u %u\\n", (unsigned)NH_SHAPE_BOX, (unsigned)NH_SHAPE_SPHERE, (unsigned)NH_SHAPE_NONE, (unsigned)NH_RAY_ANY_HIT);\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nudge_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    k = 0
    for cname, ms in members.items():
        mirror, rec = (E.Ray, E.RAY) if cname == "nh_Ray" else (E.RayHit, E.RAY_HIT)
        for m in ms:
            size, off = (int(v) for v in lines[k].split())
            k += 1
            assert ctypes.sizeof(mirror) == size == rec.itemsize == 32, (cname, size)
            assert getattr(mirror, m).offset == off == rec.fields[m][1], (cname, m, off)
    assert [int(v) for v in lines[k].split()] == [E.NH_SHAPE_BOX, E.NH_SHAPE_SPHERE, E.NH_SHAPE_NONE, E.NH_RAY_ANY_HIT]
    assert {"nh_query_build", "nh_raycast"} <= set(E.EXPORTS)


# ---- float64 closed forms ----------------------------------------------------------------------------------------------------------------
def _mat(q):
    x, y, z, s = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y)],
                     [2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)],
                     [2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)]])


def _box64(o, d, p, R, h):
    """(hit, t, normal, entering axis) of the exact box semantics in float64 (R: world-from-local)."""
    ol, dl = R.T @ (o - p), R.T @ d
    if np.all(np.abs(ol) <= h):
        return True, 0.0, -d / np.linalg.norm(d), -1
    t0, t1, ax = -np.inf, np.inf, -1
    for k in range(3):
        if dl[k] == 0.0:
            if abs(ol[k]) > h[k]:
                return False, 0.0, None, -1
            continue
        a, b = (-h[k] - ol[k]) / dl[k], (h[k] - ol[k]) / dl[k]
        lo, hi = min(a, b), max(a, b)
        if lo > t0:
            t0, ax = lo, k
        t1 = min(t1, hi)
    if not (t0 <= t1 and t0 >= 0.0):
        return False, 0.0, None, -1
    nl = np.zeros(3)
    nl[ax] = -1.0 if dl[ax] > 0 else 1.0
    return True, t0, R @ nl, ax


def _sphere64(o, d, c, r):
    m = o - c
    if m @ m <= r * r:
        return True, 0.0, -d / np.linalg.norm(d)
    a, b = d @ d, m @ d
    disc = b * b - a * (m @ m - r * r)
    if disc < 0:
        return False, 0.0, None
    t = (-b - np.sqrt(disc)) / a
    if t < 0:
        return False, 0.0, None
    return True, t, (o + t * d - c) / r


def _rays_at(rng, n, centres):
    o = rng.uniform(-10.0, 10.0, size=(n, 3)).astype(np.float32)
    aim = centres + rng.normal(scale=1.5, size=(n, 3))
    d = aim - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, size=(n, 1))
    return o, d.astype(np.float32)


EDGE = 1e-5      # rays within this (relative) of an edge or a silhouette are not compared: float32 and float64 may disagree about them


def _close(t32, n32, t64, n64, lever=1.0):
    """t within 1e-5 relative, the normal within 1e-5 -- times `lever` for a sphere's normal, (hit point - centre) / r: the point carries the error of t
    times |d|, so a ray that travels far to a small sphere turns the same relative error of t into a larger one of the normal."""
    return abs(t32 - t64) <= 1e-5 * max(abs(t64), 1.0) and np.abs(n32 - n64).max() <= 1e-5 * lever


def test_box_and_sphere_against_float64_closed_forms():
    rng = np.random.default_rng(7)
    n = 4000
    ctr = rng.uniform(-5.0, 5.0, size=(n, 3)).astype(np.float32)
    q = _unit_quats(rng, n)
    h = rng.uniform(0.2, 2.0, size=(n, 3)).astype(np.float32)
    o, d = _rays_at(rng, n, ctr)
    compared = hits = 0
    for i in range(n):
        o64, d64, p64, R = o[i].astype(np.float64), d[i].astype(np.float64), ctr[i].astype(np.float64), _mat(q[i])
        ref = _box64(o64, d64, p64, R, h[i].astype(np.float64))
        lo = _box64(o64, d64, p64, R, h[i] * (1.0 - EDGE))
        hi = _box64(o64, d64, p64, R, h[i] * (1.0 + EDGE))
        if not (ref[0] == lo[0] == hi[0] and ref[3] == lo[3] == hi[3]):
            continue
        t, nn, hit = Q.ray_box(o[i], d[i], ctr[i], q[i], h[i])
        compared += 1
        assert hit == ref[0], (i, hit, ref)
        if hit:
            hits += 1
            assert _close(t, nn, ref[1], ref[2]), (i, t, ref[1], nn, ref[2])
    assert compared > 0.99 * n and hits > 0.3 * n, (compared, hits)

    r = rng.uniform(0.2, 2.0, size=n).astype(np.float32)
    compared = hits = 0
    for i in range(n):
        o64, d64, c64 = o[i].astype(np.float64), d[i].astype(np.float64), ctr[i].astype(np.float64)
        ref = _sphere64(o64, d64, c64, float(r[i]))
        if not (ref[0] == _sphere64(o64, d64, c64, float(r[i]) * (1 - EDGE))[0] == _sphere64(o64, d64, c64, float(r[i]) * (1 + EDGE))[0]):
            continue
        # (near a silhouette t rests on the root of a small discriminant, which float32 rounding of its terms moves by ~sqrt(eps): rays within 1e-5 of it are
        # compared for hit / miss only)
        m = o64 - c64
        a, b = d64 @ d64, m @ d64
        disc = b * b - a * (m @ m - float(r[i]) ** 2)
        t, nn, hit = Q.ray_sphere(o[i], d[i], ctr[i], float(r[i]))
        compared += 1
        assert hit == ref[0], (i, hit, ref)
        if hit:
            hits += 1
            if ref[1] > 0 and disc < 1e-3 * b * b:
                continue
            assert _close(t, nn, ref[1], ref[2], lever=max(1.0, ref[1] * np.sqrt(a) / float(r[i]))), (i, t, ref[1], nn, ref[2])
    assert compared > 0.99 * n and hits > 0.2 * n, (compared, hits)


def test_compound_collider_pose_and_hits():
    """A collider on a rotated body with a local transform of its own: the pose is the composition k_xform computes, the hit that of the composed box."""
    rng = np.random.default_rng(8)
    n = 1000
    bq, lq = _unit_quats(rng, n), _unit_quats(rng, n)
    bp = rng.uniform(-4.0, 4.0, size=(n, 3)).astype(np.float32)
    lp = rng.uniform(-1.5, 1.5, size=(n, 3)).astype(np.float32)
    h = rng.uniform(0.2, 1.5, size=(n, 3)).astype(np.float32)
    compared = 0
    for i in range(n):
        p, q = Q.pose(bp[i], bq[i], lp[i], lq[i])
        Rb, Rl = _mat(bq[i]), _mat(lq[i])
        p64 = Rb @ lp[i].astype(np.float64) + bp[i]
        assert np.abs(p - p64).max() <= 1e-5 * max(1.0, np.abs(p64).max())
        assert np.abs(_mat(q) - Rb @ Rl).max() <= 1e-5
        o, d = _rays_at(rng, 1, p64[None, :])
        ref = _box64(o[0].astype(np.float64), d[0].astype(np.float64), p64, Rb @ Rl, h[i].astype(np.float64))
        lo = _box64(o[0].astype(np.float64), d[0].astype(np.float64), p64, Rb @ Rl, h[i] * (1.0 - 1e-4))
        hi = _box64(o[0].astype(np.float64), d[0].astype(np.float64), p64, Rb @ Rl, h[i] * (1.0 + 1e-4))
        if not (ref[0] == lo[0] == hi[0] and ref[3] == lo[3] == hi[3]):
            continue        # (the composed pose itself carries float32 rounding: the margin is that of the pose, not of the ray test)
        t, nn, hit = Q.ray_box(o[0], d[0], p, q, h[i])
        compared += 1
        assert hit == ref[0]
        if hit:
            assert abs(t - ref[1]) <= 1e-4 * max(ref[1], 1.0) and np.abs(nn - ref[2]).max() <= 1e-4, (i, t, ref)
    assert compared > 0.95 * n


# ---- named cases, through the brute force the GPU tests use as their oracle ---------------------------------------------------------------------
def _world(boxes=(), spheres=(), bodies=None):
    """boxes: (position, half extents, body), spheres: (position, radius, body); bodies at identity, collider transforms carry the positions."""
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


def _ray(o, d, max_t=np.inf, ignore=NONE):
    r = np.zeros(1, dtype=E.RAY)
    r["origin"], r["direction"], r["max_t"], r["ignore_body"] = o, d, max_t, ignore
    return r


def _cast(world, o, d, **kw):
    rec, nbox = world
    return CAST.cast(CAST.RAY, rec, nbox, _ray(o, d, **kw))[0]


def test_origin_inside_a_box_and_inside_a_sphere_hits_at_zero():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 1)], spheres=[((10, 0, 0), 2.0, 2)])
    h = _cast(w, (0.5, 0.2, -0.3), (0, 0, 2))
    assert h["t"] == 0.0 and h["shape"] == E.NH_SHAPE_BOX and h["collider"] == 0 and h["body"] == 1 and h["tag"] == 100
    assert np.array_equal(h["normal"], np.float32([0, 0, -1]))
    h = _cast(w, (10.5, 1.0, 0.0), (3, 0, 4))
    assert h["t"] == 0.0 and h["shape"] == E.NH_SHAPE_SPHERE and h["collider"] == 0 and h["body"] == 2 and h["tag"] == 200
    assert np.array_equal(h["normal"], np.float32([-0.6, 0, -0.8]))


def test_a_zero_direction_component_with_the_origin_on_a_face_plane():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 1)])
    h = _cast(w, (1.0, 0.0, -5.0), (0.0, 0.0, 1.0))          # on the plane x = +1: the x slab holds it, all or nothing
    assert h["shape"] == E.NH_SHAPE_BOX and h["t"] == 4.0 and np.array_equal(h["normal"], np.float32([0, 0, -1]))
    h = _cast(w, (-1.0, 1.0, -5.0), (0.0, 0.0, 1.0))         # on an edge
    assert h["shape"] == E.NH_SHAPE_BOX and h["t"] == 4.0
    h = _cast(w, (np.nextafter(np.float32(1), np.float32(2)), 0.0, -5.0), (0.0, 0.0, 1.0))
    assert h["shape"] == E.NH_SHAPE_NONE
    h = _cast(w, (1.0, 0.0, -5.0), (0.0, -0.0, 1.0))         # (negative zero: the same)
    assert h["shape"] == E.NH_SHAPE_BOX and h["t"] == 4.0


def test_max_t_zero_and_infinite():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 1)])
    h = _cast(w, (0, 0, -5), (0, 0, 1), max_t=0.0)
    assert h["shape"] == E.NH_SHAPE_NONE and h["t"] == 0.0 and h["body"] == NONE and h["collider"] == NONE and h["tag"] == NONE
    assert np.array_equal(h["normal"], np.zeros(3, np.float32))
    h = _cast(w, (0, 0, 0.5), (0, 0, 1), max_t=0.0)         # inside: t = 0 <= max_t
    assert h["shape"] == E.NH_SHAPE_BOX and h["t"] == 0.0
    h = _cast(w, (0, 0, -5), (0, 0, 1), max_t=4.0)          # t == max_t counts
    assert h["shape"] == E.NH_SHAPE_BOX and h["t"] == 4.0
    h = _cast(w, (0, 0, -5), (0, 0, 1), max_t=np.nextafter(np.float32(4), np.float32(0)))
    assert h["shape"] == E.NH_SHAPE_NONE and h["t"] == np.nextafter(np.float32(4), np.float32(0))
    far = _world(boxes=[((0, 0, 3e30), (1, 1, 1), 1)])
    h = _cast(far, (0, 0, 0), (0, 0, 1), max_t=np.inf)
    assert h["shape"] == E.NH_SHAPE_BOX and h["t"] == np.float32(3e30) - 1
    h = _cast(w, (0, 0, -5), (0, 0, -1), max_t=np.inf)      # behind the origin
    assert h["shape"] == E.NH_SHAPE_NONE and h["t"] == np.inf


def test_ignore_body_skips_every_collider_of_that_body():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 1), ((0, 0, 3), (0.5, 0.5, 0.5), 1), ((0, 0, 6), (1, 1, 1), 2)], spheres=[((0, 0, 1.5), 0.2, 1)])
    assert _cast(w, (0, 0, -5), (0, 0, 1))["body"] == 1
    h = _cast(w, (0, 0, -5), (0, 0, 1), ignore=1)
    assert h["body"] == 2 and h["collider"] == 2 and h["t"] == 10.0
    assert _cast(w, (0, 0, -5), (0, 0, 1), ignore=2)["collider"] == 0
    assert _cast(w, (0, 0, -5), (0, 0, 1), ignore=7)["collider"] == 0


def test_coincident_colliders_the_lower_index_wins():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 3), ((0, 0, 0), (1, 1, 1), 2), ((0, 0, 0), (1, 1, 1), 1)])
    h = _cast(w, (0, 0, -5), (0, 0, 1))
    assert h["collider"] == 0 and h["body"] == 3
    assert _cast(w, (0, 0, -5), (0, 0, 1), ignore=3)["collider"] == 1
    # a box and a sphere with the same t: the box (shape 0) wins
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 2)], spheres=[((0, 0, 0), 1.0, 1)])
    assert Q.ray_sphere((0, 0, -5), (0, 0, 1), (0, 0, 0), 1.0)[0] == 4.0
    h = _cast(w, (0, 0, -5), (0, 0, 1))
    assert h["shape"] == E.NH_SHAPE_BOX and h["t"] == 4.0
    assert _cast(w, (0, 0, -5), (0, 0, 1), ignore=2)["shape"] == E.NH_SHAPE_SPHERE


def test_a_non_unit_direction_scales_t():
    rng = np.random.default_rng(9)
    w = _world(boxes=[((0.3, -0.2, 0.1), (1, 0.7, 1.3), 1)], spheres=[((4, 1, 0), 1.1, 2)])
    for _ in range(200):
        o = rng.uniform(-6, 6, size=3).astype(np.float32)
        d = (rng.choice([(0.3, -0.2, 0.1), (4, 1, 0)]) + rng.normal(scale=0.3, size=3) - o).astype(np.float32)
        a, b = _cast(w, o, d), _cast(w, o, (d * np.float32(2)).astype(np.float32))
        assert a["shape"] == b["shape"] and a["collider"] == b["collider"]
        if a["shape"] != E.NH_SHAPE_NONE:
            assert b["t"] == a["t"] / 2 and np.array_equal(a["normal"], b["normal"])      # (a power of two: exactly)
            c = _cast(w, o, (d * np.float32(3)).astype(np.float32))
            assert c["collider"] == a["collider"] and abs(c["t"] * 3 - a["t"]) <= 1e-5 * max(a["t"], 1.0)


def test_non_finite_rays_are_written_as_misses_with_nan():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 1)])
    for o, d in (((np.nan, 0, -5), (0, 0, 1)), ((0, 0, -5), (0, np.inf, 1))):
        h = _cast(w, o, d)
        assert h["shape"] == E.NH_SHAPE_NONE and np.isnan(h["t"]) and h["body"] == NONE


def test_collider_of_a_missing_body_is_never_hit():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 5)], bodies=2)
    assert _cast(w, (0, 0, -5), (0, 0, 1))["shape"] == E.NH_SHAPE_NONE
