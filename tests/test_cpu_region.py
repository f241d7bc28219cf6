"""nh_region on the host (no GPU): the declaration, the per-plane predicates of nudge_amd/csrc/nh_query.h ("region") through tests/hostoracle/hostregion.cpp,
the brute-force oracle's own semantics (validity, touching, capacity), the kernel's node test against the predicates, and engine.frustum_planes.

The predicate model is float64: a plane (n, d) keeps a collider iff its support distance n.p + d + r is >= 0, r = R |n| for a sphere and
sum_i h_i |n . A_i| for a box (A the rotation matrix of the float32 quaternion, evaluated in float64).  The float32 predicate must agree wherever the
float64 value lies outside a band of 1e-6 * (|n| (|p| + |h|) + |d|); the band may leave out at most 1 % of the cases."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostlib as H                          # noqa: E402
import hostregion_util as R                  # noqa: E402
from query_util import unit_quats            # noqa: E402
from nudge_amd import engine as E           # noqa: E402

NONE = 0xFFFFFFFF
SENTINEL = 0xA5
IDENT = (0.0, 0.0, 0.0, 1.0)


# ---- the declaration ------------------------------------------------------------------------------------------------------------------------
def test_the_call_is_declared_exported_and_wrapped(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "nudge_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert ("int nh_region(nh_context* ctx, const nh_Region* regions, uint32_t count, uint32_t* offsets , nh_OverlapHit* hits, uint32_t capacity, "
            "uint32_t flags );") in flat
    assert "#define NH_REGION_MAX_PLANES 8u" in hdr and E.NH_REGION_MAX_PLANES == 8
    assert "nh_region" in E.EXPORTS
    syms = subprocess.check_output(["nm", "-D", "--defined-only", E._LIB_PATH], text=True)
    assert re.search(r"\bT nh_region$", syms, flags=re.M)
    assert list(inspect.signature(E.World.region_records).parameters) == ["self", "regions", "offsets", "hits", "capacity"]
    assert list(inspect.signature(E.World.region).parameters) == ["self", "planes", "plane_counts", "ignore_body", "capacity", "synchronize"]
    # nh_Region: 144 bytes, as gcc lays it out and as the numpy record has it
    ms = ("planes", "plane_count", "ignore_body", "reserved")
    body = "".join(f'  printf("%zu %zu\\n", sizeof(nh_Region), offsetof(nh_Region, {m}));\n' for m in ms)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nudge_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    for k, m in enumerate(ms):
        size, off = (int(v) for v in lines[k].split())
        assert size == E.REGION.itemsize == 144
        assert off == E.REGION.fields[m][1], (m, off)


# ---- the predicates against float64 -----------------------------------------------------------------------------------------------------------
def _matrix64(q):
    """The columns of nh_matrix(q) in float64, for (n, 4) float32 quaternions (x, y, z, s)."""
    x, y, z, s = (q[:, k].astype(np.float64) for k in range(4))
    c0 = np.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y + 2 * s * z, 2 * x * z - 2 * s * y], axis=1)
    c1 = np.stack([2 * x * y - 2 * s * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z + 2 * s * x], axis=1)
    c2 = np.stack([2 * x * z + 2 * s * y, 2 * y * z - 2 * s * x, 1 - 2 * x * x - 2 * y * y], axis=1)
    return c0, c1, c2


def _reach64(n, q, h, box):
    n = n.astype(np.float64)
    if not box:
        return h[:, 0].astype(np.float64) * np.linalg.norm(n, axis=1)
    return sum(h[:, k].astype(np.float64) * np.abs((n * c).sum(axis=1)) for k, c in enumerate(_matrix64(q)))


def _pairs(rng, count, box):
    p = rng.uniform(-100.0, 100.0, size=(count, 3)).astype(np.float32)
    q = unit_quats(rng, count)
    h = rng.uniform(0.05, 2.0, size=(count, 3)).astype(np.float32)
    if not box:
        h[:, 1:] = h[:, :1]
    n = rng.normal(size=(count, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True) * np.exp(rng.uniform(-3.0, 3.0, size=(count, 1)))).astype(np.float32)
    norm = np.linalg.norm(n.astype(np.float64), axis=1)
    # d places the plane within +-3 |n| of tangency
    d = (-(n.astype(np.float64) * p).sum(axis=1) - _reach64(n, q, h, box) + rng.uniform(-3.0, 3.0, size=count) * norm).astype(np.float32)
    return n, d, p, q, h


def _agreement(box, seed, count=100000):
    rng = np.random.default_rng(seed)
    n, d, p, q, h = _pairs(rng, count, box)
    got = R.keeps(np.concatenate([n, d[:, None]], axis=1), p, q, h, box)
    value = (n.astype(np.float64) * p).sum(axis=1) + d.astype(np.float64) + _reach64(n, q, h, box)
    size = np.linalg.norm(h.astype(np.float64), axis=1) if box else h[:, 0].astype(np.float64)
    scale = np.linalg.norm(n.astype(np.float64), axis=1) * (np.linalg.norm(p.astype(np.float64), axis=1) + size) + np.abs(d.astype(np.float64))
    clear = np.abs(value) > 1e-6 * scale
    print(f"{'boxes' if box else 'spheres'}: {int((~clear).sum())} of {count} inside the band; kept {int(got.sum())}; "
          f"worst disagreement {float(np.max(np.where(got != (value >= 0), np.abs(value) / scale, 0.0))):.3g} of the scale")
    assert (~clear).mean() <= 0.01
    assert 0.2 < got.mean() < 0.8                                      # both answers occur
    assert np.array_equal(got[clear], (value >= 0)[clear])


def test_the_box_predicate_agrees_with_float64_outside_the_band():
    _agreement(True, 31)


def test_the_sphere_predicate_agrees_with_float64_outside_the_band():
    _agreement(False, 32)


# ---- the oracle's semantics ------------------------------------------------------------------------------------------------------------------
def _lattice(count=16, spheres=0):
    """`count` unit boxes at integer centres (k, 0, 0), identity rotation, half extents 0.5, body k + 1; then `spheres` spheres of radius 0.5 at (k, 2, 0)."""
    rec = np.zeros(count + spheres, dtype=H.REC)
    rec["q"] = IDENT
    rec["h"] = 0.5
    rec["p"][:count, 0] = np.arange(count)
    rec["p"][count:, 0] = np.arange(spheres)
    rec["p"][count:, 1] = 2.0
    rec["body"] = np.arange(count + spheres) + 1
    rec["tag"] = np.arange(count + spheres) + 100
    return rec


def test_a_plane_that_touches_a_face_exactly_keeps_the_box():
    rec = _lattice()
    for k in range(14):
        touching = R.regions([[(-1.0, 0.0, 0.0, k + 0.5)]])
        short = R.regions([[(-1.0, 0.0, 0.0, k + 0.25)]])
        off, hits, total = R.region(rec, 16, touching)
        assert total == k + 2 and list(hits["collider"][:total]) == list(range(k + 2))         # the box centred at k + 1: s + r == 0
        off, hits, total = R.region(rec, 16, short)
        assert total == k + 1 and list(hits["collider"][:total]) == list(range(k + 1))
    # the per-plane function itself, on the box centred at 5
    one = lambda d: bool(R.keeps(np.float32([[-1, 0, 0, d]]), np.float32([[5, 0, 0]]), np.float32([IDENT]), np.float32([[0.5, 0.5, 0.5]]), True)[0])   # noqa: E731
    assert one(4.5) and not one(np.nextafter(np.float32(4.5), np.float32(0)))


def test_records_order_identity_and_ignore_body():
    rec = _lattice(8, 8)
    slab = R.regions([[(1.0, 0.0, 0.0, -1.5), (-1.0, 0.0, 0.0, 4.5)]])            # 1.5 <= x <= 4.5, reaching: centres 1 .. 5
    off, hits, total = R.region(rec, 8, slab)
    assert list(off) == [0, 10] and total == 10
    assert list(hits["collider"]) == [1, 2, 3, 4, 5] * 2 and list(hits["shape"]) == [E.NH_SHAPE_BOX] * 5 + [E.NH_SHAPE_SPHERE] * 5
    assert list(hits["body"]) == [2, 3, 4, 5, 6, 10, 11, 12, 13, 14] and list(hits["tag"]) == [101, 102, 103, 104, 105, 109, 110, 111, 112, 113]
    slab["ignore_body"] = 4
    off, hits, total = R.region(rec, 8, slab)
    assert total == 9 and 4 not in hits["body"][:total]
    # planes behind plane_count are not read
    slab["ignore_body"] = NONE
    slab["plane_count"] = 1
    slab["planes"][0, 2:] = np.nan
    assert R.region(rec, 8, slab)[2] == 14                                          # x >= 1.5 alone: centres 1 .. 7 of both shapes
    # a NaN pose is never listed
    rec["p"][3] = np.nan
    assert R.region(rec, 8, slab)[2] == 13


def _invalid_regions():
    """The invalid kinds: plane counts 0 and 9, a NaN, an infinity, a zero normal, a normal whose square overflows."""
    keep_all = (0.0, 1.0, 0.0, 1e6)
    out = R.regions(np.tile(np.float32([keep_all, keep_all]), (6, 1, 1)))
    out["plane_count"][0] = 0
    out["plane_count"][1] = 9
    out["planes"][2, 1, 3] = np.nan
    out["planes"][3, 0, 0] = np.inf
    out["planes"][4, 1, :3] = 0.0
    out["planes"][5, 0, 1] = 1e20
    return out


def test_invalid_regions_list_nothing():
    rec = _lattice(8, 8)
    bad = _invalid_regions()
    good = R.regions([[(0.0, 1.0, 0.0, 1e6)] * 2])
    assert R.valid(good[0]) and R.region(rec, 8, good)[2] == 16
    for k in range(len(bad)):
        assert not R.valid(bad[k]), k
    off, _, total = R.region(rec, 8, np.concatenate([bad[:3], good, bad[3:]]))
    assert total == 16 and list(np.diff(off.astype(np.int64))) == [0, 0, 0, 16, 0, 0, 0]
    # a NaN behind plane_count does not make a region invalid
    ok = good.copy()
    ok["plane_count"] = 1
    ok["planes"][0, 1] = np.nan
    ok["reserved"] = 0xFFFFFFFF
    assert R.valid(ok[0]) and R.region(rec, 8, ok)[2] == 16


def test_the_capacity_prefix_leaves_the_sentinel_behind_it():
    rec = _lattice(8, 8)
    regs = R.regions([[(-1.0, 0.0, 0.0, 2.0)], [(-1.0, 0.0, 0.0, 0.0)], [(-1.0, 0.0, 0.0, 5.0)]])      # 6, 2 and 12 records
    full_off, full, total = R.region(rec, 8, regs)
    assert list(full_off) == [0, 6, 8, 20] and total == 20
    for cap, written in ((20, 20), (19, 8), (8, 8), (7, 6), (5, 0), (0, 0)):
        hits = np.frombuffer(bytes([SENTINEL]) * 16 * 20, dtype=E.OVERLAP_HIT).copy()
        off, hits, t = R.region(rec, 8, regs, capacity=cap, hits=hits)
        assert off.tobytes() == full_off.tobytes() and t == 20
        assert hits[:written].tobytes() == full[:written].tobytes() and set(hits[written:].tobytes()) <= {SENTINEL}, cap


# ---- the kernel's node test never prunes what the predicates keep ----------------------------------------------------------------------------
def test_the_node_test_is_conservative_against_the_predicates():
    rng = np.random.default_rng(33)
    pruned_far = 0
    for box in (True, False):
        n, d, p, q, h = _pairs(rng, 20000, box)
        # half of them a hair around tangency, where rounding decides
        norm = np.linalg.norm(n.astype(np.float64), axis=1)
        tight = np.arange(len(d)) % 2 == 0
        d64 = -(n.astype(np.float64) * p).sum(axis=1) - _reach64(n, q, h, box)
        d = np.where(tight, d64 + rng.uniform(-1e-5, 1e-5, size=len(d)) * norm, d).astype(np.float32)
        planes = np.concatenate([n, d[:, None]], axis=1)
        kept = R.keeps(planes, p, q, h, box)
        for k in range(len(d)):
            lo, hi = R.leaf_box(p[k], q[k], h[k], box)
            out = R.node_outside(planes[k], lo, hi)
            assert not (kept[k] and out), (box, k)
            # an ancestor's box contains the leaf's
            grown = R.node_outside(planes[k], lo - np.float32(3.0), hi + np.float32(7.0))
            assert not (out is False and grown), (box, k)
            pruned_far += out and not tight[k]
    assert pruned_far > 5000                                           # the test does prune: it is not conservative by never saying "outside"
    nan = np.float32([np.nan] * 3)
    assert not R.node_outside(np.float32([1, 0, 0, -1e9]), nan, nan)  # only a comparison that is true prunes


# ---- engine.frustum_planes ------------------------------------------------------------------------------------------------------------------
def _camera(rng):
    """A perspective x look-at clip matrix for column vectors (float64), and point(ndc_x, ndc_y, depth): the world point at that depth along the view
    direction whose clip x / w and y / w are the two given."""
    eye = rng.uniform(-20, 20, size=3)
    fwd = rng.normal(size=3)
    fwd /= np.linalg.norm(fwd)
    up = np.cross(np.cross(fwd, rng.normal(size=3)), fwd)
    up /= np.linalg.norm(up)
    right = np.cross(fwd, up)
    view = np.eye(4)
    view[0, :3], view[1, :3], view[2, :3] = right, up, -fwd
    view[:3, 3] = -view[:3, :3] @ eye
    f, aspect, near, far = 1.0 / np.tan(np.radians(rng.uniform(30, 90)) / 2), rng.uniform(1.0, 2.0), 0.5, rng.uniform(50, 200)
    proj = np.array([[f / aspect, 0, 0, 0], [0, f, 0, 0], [0, 0, (far + near) / (near - far), 2 * far * near / (near - far)], [0, 0, -1, 0]])

    def point(ndc_x, ndc_y, depth):
        return eye + np.outer(ndc_x * depth * aspect / f, right) + np.outer(ndc_y * depth / f, up) + np.outer(depth, fwd)

    return proj @ view, point, near, far


def test_frustum_planes_face_inwards_and_each_bounds_its_own_face():
    rng = np.random.default_rng(34)
    k = 500
    for _ in range(8):
        m, point, near, far = _camera(rng)
        planes = E.frustum_planes(m)
        assert planes.shape == (6, 4) and planes.dtype == np.float32

        def check(x, face):
            """Every point has clip coordinates strictly inside the cube but for `face` (None: none), and the planes say the same."""
            clip = np.concatenate([x, np.ones((len(x), 1))], axis=1) @ m.T
            w = clip[:, 3:]
            cube = np.stack([w[:, 0] + clip[:, 0], w[:, 0] - clip[:, 0], w[:, 0] + clip[:, 1], w[:, 0] - clip[:, 1], w[:, 0] + clip[:, 2], w[:, 0] - clip[:, 2]], axis=1)
            value = x @ planes[:, :3].astype(np.float64).T + planes[:, 3].astype(np.float64)
            for g in range(6):
                assert ((cube[:, g] < 0) if g == face else (cube[:, g] > 0)).all(), (face, g)
                assert ((value[:, g] < 0) if g == face else (value[:, g] > 0)).all(), (face, g)

        inner = lambda: rng.uniform(-0.9, 0.9, size=k)      # noqa: E731
        outer = lambda: rng.uniform(1.1, 2.0, size=k)       # noqa: E731
        depth = lambda: rng.uniform(1.2 * near, 0.9 * far, size=k)      # noqa: E731
        check(point(inner(), inner(), depth()), None)
        check(point(-outer(), inner(), depth()), 0)          # left, right, bottom, top, near, far: rows 0, 1, 2 of m added to, subtracted from the last
        check(point(outer(), inner(), depth()), 1)
        check(point(inner(), -outer(), depth()), 2)
        check(point(inner(), outer(), depth()), 3)
        check(point(inner(), inner(), rng.uniform(0.1 * near, 0.9 * near, size=k)), 4)
        check(point(inner(), inner(), rng.uniform(1.1 * far, 2.0 * far, size=k)), 5)
