"""Closest-point queries on the host (no GPU): the nh_PointQuery / nh_PointHit records of include/nudge_hip.h against their Python mirrors, and the
closest-point arithmetic of nudge_amd/csrc/nh_query.h -- built for the host by tests/hostpoint_util.py, the same bits as the device -- against an
independent float64 model, named cases, the max_distance boundaries, invalid queries, the reach rule's monotonicity (what makes the GPU walk's pruning
exact) and the sphere-overlap oracle."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostoverlap_util as O                 # noqa: E402
import hostpoint_util as H                   # noqa: E402
import hostquery_util as Q                   # noqa: E402
from query_util import unit_quats as _unit_quats      # noqa: E402
from nudge_amd import engine as E           # noqa: E402

NONE = 0xFFFFFFFF
IDENTITY = np.float32([0, 0, 0, 1])


def test_point_records_match_the_header(tmp_path):
    """nh_PointQuery (32 B) and nh_PointHit (48 B): every member offset as gcc lays it out, the ctypes mirrors and the numpy records."""
    layouts = (("nh_PointQuery", E.PointQuery, E.POINT_QUERY, 32, ("point", "max_distance", "ignore_body", "reserved")),
               ("nh_PointHit", E.PointHit, E.POINT_HIT, 48, ("distance", "normal", "point", "body", "collider", "shape", "tag", "reserved")))
    body = ""
    for name, _, _, _, members in layouts:
        body += "".join(f'  printf("%zu %zu\\n", sizeof({name}), offsetof({name}, {m}));\n' for m in members)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nudge_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = iter(subprocess.check_output([str(exe)], text=True).split("\n"))
    for name, cs, dt, size, members in layouts:
        for m in members:
            sz, off = (int(v) for v in next(lines).split())
            assert ctypes.sizeof(cs) == sz == dt.itemsize == size, name
            assert getattr(cs, m).offset == off == dt.fields[m][1], (name, m, off)
    assert "nh_closest" in E.EXPORTS


# ---- the float64 model ------------------------------------------------------------------------------------------------------------------------
def _mat(q):
    x, y, z, s = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y)],
                     [2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)],
                     [2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)]])


def _model_box(p, c, q, h):
    """Signed distance of p from the box (c, q, h) in float64, and the signed distance of a point x from its surface (for `point on the surface`)."""
    R = _mat(q)
    h = np.asarray(h, np.float64)
    l = R.T @ (np.asarray(p, np.float64) - np.asarray(c, np.float64))
    e = np.abs(l) - h
    return (np.linalg.norm(np.maximum(e, 0.0)) if (e > 0).any() else float(e.max())), (lambda x: float((np.abs(R.T @ (np.asarray(x, np.float64) - c)) - h).max()))


def test_predicates_agree_with_a_float64_model():
    rng = np.random.default_rng(1)
    qs = _unit_quats(rng, 4000)
    for i in range(4000):
        c = rng.uniform(-50, 50, size=3).astype(np.float32)
        h = rng.uniform(0.05, 3.0, size=3).astype(np.float32)
        p = (c + rng.normal(scale=rng.choice([0.3, 2.0, 10.0]), size=3)).astype(np.float32)
        scale = float(np.abs(c).max() + np.abs(p - c).max() + h.max())
        tol = 3e-6 * scale
        d, n, x = H.point_box(p, c, qs[i], h)
        d64, surf = _model_box(p, c, qs[i], h)
        assert abs(float(d) - d64) <= tol, (i, d, d64)
        assert abs(surf(x)) <= tol, (i, surf(x))                                    # on the surface
        assert abs(np.linalg.norm(n.astype(np.float64)) - 1.0) < 1e-5
        assert np.abs(x.astype(np.float64) + float(d) * n - p).max() <= 2 * tol, i   # p = point + distance normal
        R = float(rng.uniform(0.05, 3.0))
        d, n, x = H.point_sphere(p, c, R)
        d64 = np.linalg.norm(p.astype(np.float64) - c) - R
        assert abs(float(d) - d64) <= tol, (i, d, d64)
        assert abs(np.linalg.norm(x.astype(np.float64) - c) - R) <= tol
        assert np.abs(x.astype(np.float64) + float(d) * n - p).max() <= 2 * tol, i


def test_named_cases():
    c, h = np.float32([1.0, 2.0, 3.0]), np.float32([1.0, 1.0, 1.0])
    # a point on a face: +0, never -0, the face's normal, the point itself
    d, n, x = H.point_box(c + np.float32([1.0, 0.25, -0.5]), c, IDENTITY, h)
    assert np.float32(d).view(np.uint32) == 0 and np.array_equal(n, [1, 0, 0]) and np.array_equal(x, c + np.float32([1.0, 0.25, -0.5]))
    d, n, x = H.point_box(c + np.float32([0.1, -1.0, 0.2]), c, IDENTITY, h)
    assert np.float32(d).view(np.uint32) == 0 and np.array_equal(n, [0, -1, 0])
    # on an edge and at a vertex (surface: +0, the lowest axis of the faces that meet there)
    d, n, x = H.point_box(c + np.float32([1.0, 1.0, 0.0]), c, IDENTITY, h)
    assert np.float32(d).view(np.uint32) == 0 and np.array_equal(n, [1, 0, 0])
    d, n, x = H.point_box(c + np.float32([-1.0, -1.0, -1.0]), c, IDENTITY, h)
    assert np.float32(d).view(np.uint32) == 0 and np.array_equal(n, [-1, 0, 0]) and np.array_equal(x, c - 1)
    # outside an edge and a vertex: the distance to them, the normal along the diagonal
    d, n, x = H.point_box(c + np.float32([2.0, 2.0, 0.0]), c, IDENTITY, h)
    assert abs(d - np.sqrt(2)) < 1e-6 and np.allclose(n, [np.sqrt(0.5), np.sqrt(0.5), 0]) and np.array_equal(x, c + np.float32([1, 1, 0]))
    d, n, x = H.point_box(c - np.float32([2.0, 2.0, 2.0]), c, IDENTITY, h)
    assert abs(d - np.sqrt(3)) < 1e-6 and np.allclose(n, -np.ones(3) / np.sqrt(3)) and np.array_equal(x, c - 1)
    # at a cube's centre: every face is as deep, axis 0 wins, + side
    d, n, x = H.point_box(c, c, IDENTITY, h)
    assert d == -1.0 and np.array_equal(n, [1, 0, 0]) and np.array_equal(x, c + np.float32([1, 0, 0]))
    # a turned box: the normal and point turn with it
    q = np.float32([0, 0, np.sin(np.pi / 8), np.cos(np.pi / 8)])                        # 45 degrees about z
    d, n, x = H.point_box(c, c, q, np.float32([2.0, 1.0, 3.0]))
    assert d == -1.0 and np.allclose(n, [-np.sqrt(0.5), np.sqrt(0.5), 0], atol=1e-6)   # the thin y axis, turned
    # at a sphere's centre: +y
    d, n, x = H.point_sphere(c, c, 2.0)
    assert d == -2.0 and np.array_equal(n, [0, 1, 0]) and np.array_equal(x, c + np.float32([0, 2, 0]))
    d, n, x = H.point_sphere(c + np.float32([0, 0, 5]), c, 2.0)
    assert d == 3.0 and np.array_equal(n, [0, 0, 1]) and np.array_equal(x, c + np.float32([0, 0, 2]))


def _rec(colliders):
    """Records of (kind, position, rotation, size, body): boxes first, as the build numbers them."""
    rec = np.zeros(len(colliders), dtype=Q.REC)
    for i, (kind, p, q, h, body) in enumerate(colliders):
        rec[i]["p"], rec[i]["q"], rec[i]["body"], rec[i]["tag"] = p, q, body, 100 + i
        rec[i]["h"] = h if kind == "box" else (h, h, h)
    return rec, sum(1 for k in colliders if k[0] == "box")


def _query(points, max_distance=np.inf, ignore_body=NONE):
    q = np.zeros(len(points), dtype=E.POINT_QUERY)
    q["point"], q["max_distance"], q["ignore_body"] = points, max_distance, ignore_body
    return q


def test_the_deepest_collider_wins_and_ties_go_to_the_lower_shape_and_index():
    rec, nbox = _rec([("box", (0, 0, 0), IDENTITY, (1, 1, 1), 1), ("sphere", (0, 0, 0), IDENTITY, 2.0, 2)])
    hit = H.closest(rec, nbox, _query([(0.5, 0, 0)]))[0]
    assert hit["shape"] == E.NH_SHAPE_SPHERE and hit["distance"] == -1.5 and hit["body"] == 2 and hit["tag"] == 101
    # equal distances: the box (shape 0) before the sphere, then the lower index
    rec, nbox = _rec([("box", (0, 0, 0), IDENTITY, (1, 1, 1), 1), ("sphere", (0, 0, 0), IDENTITY, 1.0, 2)])
    hit = H.closest(rec, nbox, _query([(3, 0, 0)]))[0]
    assert hit["shape"] == E.NH_SHAPE_BOX and hit["collider"] == 0 and hit["distance"] == 2.0
    rec, nbox = _rec([("box", (0, 0, 0), IDENTITY, (1, 1, 1), 3)] * 3 + [("sphere", (5, 0, 0), IDENTITY, 1.0, 4)] * 2)
    hits = H.closest(rec, nbox, _query([(0.2, 0.1, 0), (5, 0, 0), (5, 3, 0)]))
    assert list(hits["collider"]) == [0, 0, 0] and list(hits["shape"]) == [0, 1, 1]
    # ignore_body skips every collider of that body
    hit = H.closest(rec, nbox, _query([(0.2, 0.1, 0)], ignore_body=3))[0]
    assert hit["shape"] == E.NH_SHAPE_SPHERE and hit["body"] == 4


def test_max_distance_boundaries():
    rec, nbox = _rec([("sphere", (0, 0, 0), IDENTITY, 1.0, 1)])
    at = H.closest(rec, nbox, _query([(3, 0, 0)], max_distance=2.0))[0]
    assert at["shape"] == E.NH_SHAPE_SPHERE and at["distance"] == 2.0                   # exactly at max_distance: counts
    below = np.nextafter(np.float32(2.0), np.float32(0))
    miss = H.closest(rec, nbox, _query([(3, 0, 0)], max_distance=below))[0]
    assert miss["shape"] == NONE and miss["distance"] == below                           # a float beyond: a miss, distance = max_distance
    assert not miss["normal"].any() and not miss["point"].any() and miss["body"] == miss["collider"] == miss["tag"] == NONE and miss["reserved"] == 0
    # max_distance 0: only colliders that contain or touch p
    rec, nbox = _rec([("box", (0, 0, 0), IDENTITY, (1, 1, 1), 1)])
    hits = H.closest(rec, nbox, _query([(1, 0.5, 0), (0.5, 0, 0), (1.0001, 0, 0)], max_distance=0.0))
    assert list(hits["shape"]) == [0, 0, NONE] and hits["distance"][0] == 0 and hits["distance"][1] == -0.5
    # +inf: the nearest anywhere
    hit = H.closest(rec, nbox, _query([(1e6, -3e5, 2e5)]))[0]
    assert hit["shape"] == E.NH_SHAPE_BOX and abs(hit["distance"] - np.linalg.norm([1e6 - 1, -3e5 + 1, 2e5 - 1])) < 0.2


def test_invalid_queries_and_nan_poses():
    rec, nbox = _rec([("box", (0, 0, 0), IDENTITY, (1, 1, 1), 1), ("sphere", (0, 0, 0), IDENTITY, 1.0, 2)])
    pts = np.float32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0, 0, 0], [0, 0, 0]])
    q = _query(pts)
    q["max_distance"][3], q["max_distance"][4] = np.nan, -1.0
    hits = H.closest(rec, nbox, q)
    assert np.isnan(hits["distance"]).all() and (hits["shape"] == NONE).all() and not hits["normal"].any() and not hits["point"].any()
    # a collider of a body that does not exist has a NaN pose: never reported, even at max_distance +inf
    rec["p"][1] = np.nan
    rec["q"][1] = np.nan
    hits = H.closest(rec, nbox, _query([(0, 0, 0), (5, 5, 5), (0, 9, 0)]))
    assert (hits["shape"] == E.NH_SHAPE_BOX).all()
    rec["p"][0] = np.nan
    hits = H.closest(rec, nbox, _query([(0, 0, 0), (5, 5, 5)]))
    assert (hits["shape"] == NONE).all() and np.isinf(hits["distance"]).all()


def test_the_node_bound_never_exceeds_the_leaf_key():
    """The reach rule's lemma: for a box that contains the leaf box, nh_q_point_node is never larger than the leaf's -- so sqrtf of it never exceeds
    the key of any collider below, and the walk's strict test cannot prune the brute force's winner."""
    rng = np.random.default_rng(2)
    qs = _unit_quats(rng, 3000)
    for i in range(3000):
        c = rng.uniform(-1e3, 1e3, size=3).astype(np.float32) * np.float32(rng.choice([1e-3, 1.0, 30.0]))
        box = bool(i % 2)
        h = rng.uniform(0.01, 2.0, size=3).astype(np.float32)
        lo, hi = H.leaf_box(c, qs[i], h, box)
        p = (c + rng.normal(scale=rng.choice([0.5, 5.0, 500.0]), size=3)).astype(np.float32)
        leaf = H.point_node(lo, hi, p)
        d = H.point_box(p, c, qs[i], h)[0] if box else H.point_sphere(p, c, h[0])[0]
        key = H.point_key(d, leaf)
        assert key >= d and (leaf == 0 or key >= np.sqrt(np.float32(leaf)))
        for _ in range(3):
            olo = (lo - rng.choice([0, 1e-6, 0.1, 10.0], size=3)).astype(np.float32)
            ohi = (hi + rng.choice([0, 1e-6, 0.1, 10.0], size=3)).astype(np.float32)
            node = H.point_node(olo, ohi, p)
            assert node <= leaf, (i, node, leaf)
            assert node == 0 or np.sqrt(node) <= key


def test_a_hit_within_r_exists_iff_the_sphere_overlap_of_radius_r_is_not_empty():
    rng = np.random.default_rng(3)
    n = 300
    colliders = [("box", rng.uniform(-10, 10, size=3), q, rng.uniform(0.2, 1.5, size=3), 1 + i) for i, q in enumerate(_unit_quats(rng, n))]
    colliders += [("sphere", rng.uniform(-10, 10, size=3), IDENTITY, float(rng.uniform(0.2, 1.5)), 1 + n + i) for i in range(n // 2)]
    rec, nbox = _rec(colliders)
    m = 4000
    pts = rng.uniform(-12, 12, size=(m, 3)).astype(np.float32)
    r = rng.choice(np.float32([0.0, 0.1, 0.5, 1.0, 3.0]), size=m)
    hits = H.closest(rec, nbox, _query(pts, max_distance=r))
    # the distance of the nearest anywhere decides which queries are close to touching
    nearest = H.closest(rec, nbox, _query(pts))["distance"].astype(np.float64)
    ov = np.zeros(m, dtype=E.OVERLAP_QUERY)
    ov["center"], ov["shape"], ov["ignore_body"] = pts, E.NH_SHAPE_SPHERE, NONE
    ov["size"][:, 0] = r
    offsets, _, _ = O.overlap(rec, nbox, ov, capacity=0)
    count = np.diff(offsets.astype(np.int64))
    clear = np.abs(nearest - r) > 1e-5 * np.maximum(1.0, r)
    assert clear.mean() > 0.95
    assert np.array_equal((hits["shape"] != NONE)[clear], (count > 0)[clear])
    assert (count[clear] > 0).mean() > 0.2 and (count[clear] == 0).mean() > 0.2
