"""Sphere casts on the host (no GPU): the nh_SphereCast record of include/nudge_hip.h against its Python mirrors, and the sweep arithmetic of
nudge_amd/csrc/nh_query.h -- built for the host by tests/hostcast_util.py, the same bits as the device -- against float64 closed forms, the named
cases of its exact semantics, the ray predicates at radius 0 and the overlap predicates at t = 0."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostcast_util as CAST                 # noqa: E402
import hostoverlap_util as O                 # noqa: E402
import hostquery_util as Q                   # noqa: E402
from cast_util import ball64 as _ball64, sweep_box64 as _sweep_box64      # noqa: E402
from query_util import mat as _mat, unit_quats as _unit_quats      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

NONE = 0xFFFFFFFF


def test_sphere_cast_record_matches_the_header(tmp_path):
    """nh_SphereCast: 48 bytes, every member offset as gcc lays it out, the ctypes mirror and the numpy record; its first 32 bytes are nh_Ray's."""
    members = ("origin", "max_t", "direction", "ignore_body", "radius", "reserved")
    body = "".join(f'  printf("%zu %zu\\n", sizeof(nh_SphereCast), offsetof(nh_SphereCast, {m}));\n' for m in members)
    body += "".join(f'  printf("%zu\\n", offsetof(nh_Ray, {m}));\n' for m in members[:4])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nudge_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    for k, m in enumerate(members):
        size, off = (int(v) for v in lines[k].split())
        assert ctypes.sizeof(E.SphereCast) == size == E.SPHERE_CAST.itemsize == 48, size
        assert getattr(E.SphereCast, m).offset == off == E.SPHERE_CAST.fields[m][1], (m, off)
        if k < 4:
            assert int(lines[len(members) + k]) == off == E.RAY.fields[m][1] == getattr(E.Ray, m).offset, m
    assert "nh_spherecast" in E.EXPORTS


# ---- float64 closed forms ----------------------------------------------------------------------------------------------------------------
def _casts_at(rng, n, centres):
    o = rng.uniform(-10.0, 10.0, size=(n, 3)).astype(np.float32)
    aim = centres + rng.normal(scale=1.5, size=(n, 3))
    d = aim - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, size=(n, 1))
    return o, d.astype(np.float32)


EDGE = 1e-5      # casts whose float64 answer changes when the sizes move by this (relative) are not compared: float32 and float64 may disagree about them


def _close(t32, n32, t64, n64, lever=1.0):
    """t within 1e-5 relative, the normal within 1e-5 -- times `lever` where the normal is (centre - closest point) / r: it carries the error of t times
    |d| / r."""
    return abs(t32 - t64) <= 1e-5 * max(abs(t64), 1.0) and np.abs(n32 - n64).max() <= 1e-5 * lever


def test_box_and_sphere_sweeps_against_float64_closed_forms():
    rng = np.random.default_rng(11)
    n = 3000
    ctr = rng.uniform(-5.0, 5.0, size=(n, 3)).astype(np.float32)
    q = _unit_quats(rng, n)
    h = rng.uniform(0.2, 2.0, size=(n, 3)).astype(np.float32)
    r = rng.uniform(0.05, 1.5, size=n).astype(np.float32)
    o, d = _casts_at(rng, n, ctr)
    compared, feats = 0, {}
    for i in range(n):
        o64, d64, p64, R = o[i].astype(np.float64), d[i].astype(np.float64), ctr[i].astype(np.float64), _mat(q[i])
        h64, r64 = h[i].astype(np.float64), float(r[i])
        ref = _sweep_box64(o64, d64, r64, p64, R, h64)
        lo = _sweep_box64(o64, d64, r64 * (1 - EDGE), p64, R, h64 * (1 - EDGE))
        hi = _sweep_box64(o64, d64, r64 * (1 + EDGE), p64, R, h64 * (1 + EDGE))
        if not (ref[0] == lo[0] == hi[0] and ref[3] == lo[3] == hi[3]):
            continue
        if ref[0] and max(abs(lo[1] - ref[1]), abs(hi[1] - ref[1])) > 1e-3 * max(ref[1], 1.0):
            continue            # (a grazing touch: t rests on a near-zero discriminant)
        t, nn, hit = CAST.sweep_box(o[i], d[i], r[i], ctr[i], q[i], h[i])
        compared += 1
        assert hit == ref[0], (i, hit, ref)
        if hit:
            feats[ref[3]] = feats.get(ref[3], 0) + 1
            lever = 1.0 if ref[3] in ("face", "start") else max(1.0, ref[1] * np.linalg.norm(d64) / r64)
            assert _close(t, nn, ref[1], ref[2], lever), (i, ref[3], t, ref[1], nn, ref[2])
            assert abs(np.linalg.norm(nn.astype(np.float64)) - 1.0) <= 1e-6
    assert compared > 0.97 * n, compared
    assert all(feats.get(k, 0) > 30 for k in ("face", "edge", "corner")) and feats.get("start", 0) > 5, feats

    R_ = rng.uniform(0.2, 2.0, size=n).astype(np.float32)
    compared = hits = 0
    for i in range(n):
        o64, d64, c64 = o[i].astype(np.float64), d[i].astype(np.float64), ctr[i].astype(np.float64)
        rho = float(R_[i]) + float(r[i])
        ref_t = 0.0 if (o64 - c64) @ (o64 - c64) <= rho * rho else _ball64(o64, d64, c64, rho)
        edge = [_ball64(o64, d64, c64, rho * (1 + s)) for s in (-EDGE, EDGE)]
        if not ((ref_t < np.inf) == (edge[0] < np.inf) == (edge[1] < np.inf)) or (ref_t < np.inf and abs(edge[0] - edge[1]) > 1e-3 * max(ref_t, 1)):
            continue
        t, nn, hit = CAST.sweep_sphere(o[i], d[i], r[i], ctr[i], R_[i])
        compared += 1
        assert hit == (ref_t < np.inf), i
        if hit:
            hits += 1
            # (nh_q_ray_sphere's t near a silhouette rests on the root of a small discriminant, as in test_cpu_query: hit / miss only there)
            m = o64 - c64
            a, b = d64 @ d64, m @ d64
            if ref_t > 0 and b * b - a * (m @ m - rho * rho) < 1e-3 * b * b:
                continue
            n64 = -d64 / np.linalg.norm(d64) if ref_t == 0.0 else (o64 + ref_t * d64 - c64) / rho
            assert _close(t, nn, ref_t, n64, lever=max(1.0, ref_t * np.linalg.norm(d64) / rho)), (i, t, ref_t)
    assert compared > 0.97 * n and hits > 0.3 * n, (compared, hits)


def test_radius_zero_is_the_ray_predicate_bit_for_bit():
    rng = np.random.default_rng(12)
    n = 3000
    ctr = rng.uniform(-5.0, 5.0, size=(n, 3)).astype(np.float32)
    q = _unit_quats(rng, n)
    h = rng.uniform(0.2, 2.0, size=(n, 3)).astype(np.float32)
    o, d = _casts_at(rng, n, ctr)
    d[: n // 10, rng.integers(0, 3)] = 0.0          # (zero direction components, the slab's all-or-nothing rule)
    hits = 0
    for i in range(n):
        for r0 in (0.0, -0.0):
            a, b = CAST.sweep_box(o[i], d[i], r0, ctr[i], q[i], h[i]), Q.ray_box(o[i], d[i], ctr[i], q[i], h[i])
            assert a[2] == b[2] and np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes() and a[1].tobytes() == b[1].tobytes(), i
            a, b = CAST.sweep_sphere(o[i], d[i], r0, ctr[i], h[i, 0]), Q.ray_sphere(o[i], d[i], ctr[i], h[i, 0])
            assert a[2] == b[2] and np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes() and a[1].tobytes() == b[1].tobytes(), i
            hits += a[2]
    assert hits > 0.2 * n
    # the same through the brute force: a cast of radius 0 writes the ray cast's bytes
    rec, nbox = _world(boxes=[(tuple(ctr[i]), tuple(h[i]), 1 + i % 5) for i in range(40)], spheres=[(tuple(ctr[40 + i]), float(h[40 + i, 0]), 2) for i in range(20)])
    rays = np.zeros(n, dtype=E.RAY)
    rays["origin"], rays["direction"], rays["max_t"], rays["ignore_body"] = o, d, np.inf, NONE
    rays["max_t"][::3] = 6.0
    rays["ignore_body"][::7] = 3
    casts = np.zeros(n, dtype=E.SPHERE_CAST)
    for k in ("origin", "direction", "max_t", "ignore_body"):
        casts[k] = rays[k]
    assert CAST.cast(CAST.SPHERE, rec, nbox, casts).tobytes() == CAST.cast(CAST.RAY, rec, nbox, rays).tobytes()


def test_a_start_overlap_under_the_overlap_predicates_hits_at_zero():
    rng = np.random.default_rng(13)
    n = 4000
    ctr = rng.uniform(-2.0, 2.0, size=(n, 3)).astype(np.float32)
    q = _unit_quats(rng, n)
    h = rng.uniform(0.2, 2.0, size=(n, 3)).astype(np.float32)
    r = rng.uniform(0.01, 1.5, size=n).astype(np.float32)
    o = rng.uniform(-4.0, 4.0, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    boxes = spheres = 0
    for i in range(n):
        inside = -d[i] / np.float32(np.sqrt(np.float32(d[i] @ d[i])))
        if O.sphere_box(o[i], r[i], ctr[i], q[i], h[i]):
            boxes += 1
            t, nn, hit = CAST.sweep_box(o[i], d[i], r[i], ctr[i], q[i], h[i])
            assert hit and t == 0.0 and np.allclose(nn, inside, atol=1e-6), i
        if O.sphere_sphere(o[i], r[i], ctr[i], h[i, 0]):
            spheres += 1
            t, nn, hit = CAST.sweep_sphere(o[i], d[i], r[i], ctr[i], h[i, 0])
            assert hit and t == 0.0 and np.allclose(nn, inside, atol=1e-6), i
    assert boxes > 300 and spheres > 300, (boxes, spheres)


# ---- named cases, through the brute force the GPU tests use as their oracle ---------------------------------------------------------------------
def _world(boxes=(), spheres=(), bodies=None, rotations=None):
    """boxes: (position, half extents, body), spheres: (position, radius, body); bodies at identity, collider transforms carry the positions."""
    nb = 1 + max([b for *_, b in list(boxes) + list(spheres)] + [0]) if bodies is None else bodies
    bt = np.zeros(nb, dtype=S.TRANSFORM)
    bt["rotation"][:, 3] = 1.0
    xt = np.zeros(len(boxes), dtype=S.TRANSFORM)
    xd = np.zeros(len(boxes), dtype=S.BOX)
    for i, (p, h, b) in enumerate(boxes):
        xt[i]["position"], xt[i]["body"], xt[i]["rotation"] = p, b, (0, 0, 0, 1) if rotations is None else rotations[i]
        xd[i]["size"] = h
    st = np.zeros(len(spheres), dtype=S.TRANSFORM)
    sd = np.zeros(len(spheres), dtype=S.SPHERE)
    for i, (p, r, b) in enumerate(spheres):
        st[i]["position"], st[i]["body"], st[i]["rotation"] = p, b, (0, 0, 0, 1)
        sd[i]["radius"] = r
    scene = dict(box_transforms=xt, box_data=xd, box_tags=np.arange(len(boxes), dtype=np.uint32) + 100,
                 sphere_transforms=st, sphere_data=sd, sphere_tags=np.arange(len(spheres), dtype=np.uint32) + 200)
    return Q.records(bt, scene), len(boxes)


def _cast(world, o, d, r, max_t=np.inf, ignore=NONE):
    rec, nbox = world
    c = np.zeros(1, dtype=E.SPHERE_CAST)
    c["origin"], c["direction"], c["radius"], c["max_t"], c["ignore_body"] = o, d, r, max_t, ignore
    return CAST.cast(CAST.SPHERE, rec, nbox, c)[0]


def test_head_on_edge_and_corner_hits():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 1)])
    h = _cast(w, (0, 0, -5), (0, 0, 1), 0.5)                 # a face: the ball touches at z = -1.5
    assert h["shape"] == E.NH_SHAPE_BOX and h["t"] == 3.5 and np.array_equal(h["normal"], np.float32([0, 0, -1])) and h["tag"] == 100
    s = np.float32(np.sqrt(0.5))
    h = _cast(w, (5, 5, 0), (-1, -1, 0), 0.5)                # an edge at 45 degrees: centre at (1 + r s, 1 + r s, 0)
    assert abs(h["t"] - (4.0 - 0.5 * s)) <= 1e-6 and np.allclose(h["normal"], (s, s, 0), atol=1e-6)
    h = _cast(w, (-4, -4, -4), (1, 1, 1), 0.75)              # a corner along the diagonal: centre at (-1, -1, -1) - r / sqrt(3)
    k = 1.0 / np.sqrt(3.0)
    assert abs(h["t"] - (3.0 - 0.75 * k)) <= 1e-6 and np.allclose(h["normal"], (-k, -k, -k), atol=1e-6)
    x = np.float32(-4) + np.float32(h["t"]) - np.float32(0.75) * h["normal"]
    assert np.allclose(x, (-1, -1, -1), atol=1e-6)           # the contact point o + t d - r n is the corner


def test_a_ball_grazing_a_face_at_exactly_r_touches():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 1)])
    h = _cast(w, (-5, 1.5, 0), (1, 0, 0), 0.5)               # sliding along the top face at distance r
    assert h["shape"] == E.NH_SHAPE_BOX and h["t"] == 4.0 and np.array_equal(h["normal"], np.float32([0, 1, 0]))      # (at the edge x = -1)
    h = _cast(w, (-5, np.nextafter(np.float32(1.5), np.float32(2)), 0), (1, 0, 0), 0.5)
    assert h["shape"] == E.NH_SHAPE_NONE


def test_a_gap_narrower_than_the_ball_blocks_it_and_a_wider_one_lets_it_pass():
    w = _world(boxes=[((-2, 0, 0), (1, 1, 1), 1), ((2, 0, 0), (1, 1, 1), 2)])          # faces at x = -1 and x = +1: a gap of 2
    h = _cast(w, (0, 10, 0), (0, -1, 0), 1.25)                                          # 2 r = 2.5 > 2
    assert h["shape"] == E.NH_SHAPE_BOX and h["t"] > 8.0 and h["t"] < 9.0
    h = _cast(w, (0, 10, 0), (0, -1, 0), 0.75)                                          # 2 r = 1.5 < 2
    assert h["shape"] == E.NH_SHAPE_NONE and h["t"] == np.inf


def test_start_overlap_max_t_and_ignore_body():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 1), ((0, 0, 6), (1, 1, 1), 2)], spheres=[((0, 0, 3), 0.5, 1)])
    h = _cast(w, (0, 0, -1.25), (0, 0, 2), 0.5)                                         # overlapping at t = 0
    assert h["t"] == 0.0 and h["collider"] == 0 and np.array_equal(h["normal"], np.float32([0, 0, -1]))
    h = _cast(w, (0, 0, -5), (0, 0, 1), 0.5, max_t=0.0)
    assert h["shape"] == E.NH_SHAPE_NONE and h["t"] == 0.0 and h["body"] == NONE and np.array_equal(h["normal"], np.zeros(3, np.float32))
    assert _cast(w, (0, 0, -5), (0, 0, 1), 0.5, max_t=3.5)["t"] == 3.5                  # t == max_t counts
    assert _cast(w, (0, 0, -5), (0, 0, 1), 0.5, max_t=np.nextafter(np.float32(3.5), np.float32(0)))["shape"] == E.NH_SHAPE_NONE
    assert _cast(w, (0, 0, -5), (0, 0, -1), 0.5)["t"] == np.inf                        # moving away
    h = _cast(w, (0, 0, -5), (0, 0, 1), 0.5, ignore=1)                                  # the first box and the sphere are body 1's
    assert h["body"] == 2 and h["collider"] == 1 and h["t"] == 9.5


def test_coincident_colliders_the_lower_index_wins():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 3), ((0, 0, 0), (1, 1, 1), 2), ((0, 0, 0), (1, 1, 1), 1)])
    h = _cast(w, (0.3, 0.2, -5), (0, 0, 1), 0.5)
    assert h["collider"] == 0 and h["body"] == 3
    assert _cast(w, (0.3, 0.2, -5), (0, 0, 1), 0.5, ignore=3)["collider"] == 1
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 2)], spheres=[((0, 0, 0), 1.0, 1)])       # a box and a sphere with the same t: the box wins
    h = _cast(w, (0, 0, -5), (0, 0, 1), 0.5)
    assert h["shape"] == E.NH_SHAPE_BOX and h["t"] == 3.5
    assert _cast(w, (0, 0, -5), (0, 0, 1), 0.5, ignore=2)["shape"] == E.NH_SHAPE_SPHERE


def test_a_non_unit_direction_scales_t():
    rng = np.random.default_rng(14)
    s2 = np.float32(np.sqrt(0.5))
    w = _world(boxes=[((0.3, -0.2, 0.1), (1, 0.7, 1.3), 1), ((-3, 2, 1), (0.5, 0.5, 0.5), 3)], spheres=[((4, 1, 0), 1.1, 2)],
               rotations=[(0, 0, 0, 1), (s2, 0, 0, s2)])
    hits = 0
    for _ in range(300):
        o = rng.uniform(-6, 6, size=3).astype(np.float32)
        aim = np.asarray([(0.3, -0.2, 0.1), (4, 1, 0), (-3, 2, 1)][rng.integers(0, 3)])
        d = (aim + rng.normal(scale=0.8, size=3) - o).astype(np.float32)
        r = np.float32(rng.uniform(0.05, 1.0))
        a, b = _cast(w, o, d, r), _cast(w, o, (d * np.float32(2)).astype(np.float32), r)
        assert a["shape"] == b["shape"] and a["collider"] == b["collider"]
        if a["shape"] != E.NH_SHAPE_NONE:
            hits += 1
            assert abs(b["t"] * 2 - a["t"]) <= 1e-5 * max(a["t"], 1.0) and np.allclose(a["normal"], b["normal"], atol=1e-5)
    assert hits > 50


def test_a_collider_of_a_missing_body_is_never_hit_and_invalid_casts_are_nan_misses():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 5)], spheres=[((0, 0, 3), 1.0, 5)], bodies=2)
    assert _cast(w, (0, 0, -5), (0, 0, 1), 0.5)["shape"] == E.NH_SHAPE_NONE
    assert _cast(w, (0, 0, -0.5), (0, 0, 1), 0.5)["shape"] == E.NH_SHAPE_NONE
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 1)])
    for o, d, r in (((np.nan, 0, -5), (0, 0, 1), 0.5), ((0, 0, -5), (0, np.inf, 1), 0.5), ((0, 0, -5), (0, 0, 1), np.inf), ((0, 0, -5), (0, 0, 1), np.nan),
                    ((0, 0, -5), (0, 0, 1), -0.25)):
        h = _cast(w, o, d, r)
        assert h["shape"] == E.NH_SHAPE_NONE and np.isnan(h["t"]) and h["body"] == NONE and h["collider"] == NONE, (o, d, r)


def test_a_zero_direction_touches_at_zero_or_misses():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 1)], spheres=[((5, 0, 0), 1.0, 2)])
    h = _cast(w, (0, 0, -1.25), (0, 0, 0), 0.5)
    assert h["t"] == 0.0 and h["shape"] == E.NH_SHAPE_BOX and np.isnan(h["normal"]).all()
    h = _cast(w, (5, 0, -1.25), (0, 0, 0), 0.5)
    assert h["t"] == 0.0 and h["shape"] == E.NH_SHAPE_SPHERE and np.isnan(h["normal"]).all()
    assert _cast(w, (0, 0, -3), (0, 0, 0), 0.5)["shape"] == E.NH_SHAPE_NONE
    assert _cast(w, (1.4, 1.4, 0), (0, 0, 0), 0.5)["shape"] == E.NH_SHAPE_NONE      # (inside the grown box, beyond the rounded edge)
