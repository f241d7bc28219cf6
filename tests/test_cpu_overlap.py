"""Overlap queries on the host (no GPU): the ABI records of nh_overlap (include/nudge_hip.h) against their Python mirrors, the three overlap
predicates of nudge_amd/csrc/nh_query.h -- built for the host by tests/hostoverlap_util.py, the device's answers -- against float64 closed forms
and named touching cases, and the brute-force oracle's semantics (ignore_body, missing bodies, order, invalid queries, capacity) on hand-built
worlds."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostoverlap_util as O                 # noqa: E402
from query_util import unit_quats as _quats  # noqa: E402
from volume_records import overlap_lists, overlap_query      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

NONE = 0xFFFFFFFF
IDENT = (0.0, 0.0, 0.0, 1.0)
DELTA = 1e-5                  # the float64 margin (relative) beyond which the float32 predicates must agree with the closed forms


def test_overlap_records_match_the_header(tmp_path):
    """nh_OverlapQuery / nh_OverlapHit: size and every member offset as gcc lays them out, against the ctypes mirrors and the numpy records."""
    members = {"nh_OverlapQuery": ("center", "shape", "rotation", "size", "ignore_body"), "nh_OverlapHit": ("body", "collider", "shape", "tag")}
    body = "".join(f'  printf("%zu %zu\\n", sizeof({c}), offsetof({c}, {m}));\n' for c, ms in members.items() for m in ms)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nudge_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    k = 0
    for cname, ms in members.items():
        mirror, rec, size_ = (E.OverlapQuery, E.OVERLAP_QUERY, 48) if cname == "nh_OverlapQuery" else (E.OverlapHit, E.OVERLAP_HIT, 16)
        for m in ms:
            size, off = (int(v) for v in lines[k].split())
            k += 1
            assert ctypes.sizeof(mirror) == size == rec.itemsize == size_, (cname, size)
            assert getattr(mirror, m).offset == off == rec.fields[m][1], (cname, m, off)
    assert "nh_overlap" in E.EXPORTS


# ---- float64 closed forms ----------------------------------------------------------------------------------------------------------------
def _mat(q):
    x, y, z, s = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y)],
                     [2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)],
                     [2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)]])


def _ss64(c, r, p, R):
    m = np.asarray(c, np.float64) - np.asarray(p, np.float64)
    return m @ m <= (r + R) ** 2


def _sb64(c, r, p, q, h):
    l = _mat(q).T @ (np.asarray(c, np.float64) - np.asarray(p, np.float64))
    d = np.maximum(np.abs(l) - np.asarray(h, np.float64), 0.0)
    return d @ d <= r * r


def _bb64(ca, qa, ha, cb, qb, hb):
    """The separating-axis theorem with unit axes; (nearly) degenerate edge-cross axes are skipped -- the face axes decide there."""
    A, B = _mat(qa), _mat(qb)
    ha, hb = np.asarray(ha, np.float64), np.asarray(hb, np.float64)
    t = np.asarray(cb, np.float64) - np.asarray(ca, np.float64)
    axes = [A[:, i] for i in range(3)] + [B[:, j] for j in range(3)]
    for i in range(3):
        for j in range(3):
            L = np.cross(A[:, i], B[:, j])
            n = np.linalg.norm(L)
            if n > 1e-9:
                axes.append(L / n)
    for L in axes:
        ra = np.abs(A.T @ L) @ ha
        rb = np.abs(B.T @ L) @ hb
        if abs(t @ L) > ra + rb:
            return False
    return True


def _clear(f):
    """The float64 answer where it does not change when every size grows or shrinks by DELTA (relative), else None."""
    lo, hi = f(1.0 - DELTA), f(1.0 + DELTA)
    return lo if lo == hi else None


def test_predicates_agree_with_float64_closed_forms_on_random_poses():
    rng = np.random.default_rng(1)
    n = 3000
    checked = {"ss": [0, 0], "sb": [0, 0], "bb": [0, 0]}
    qa, qb = _quats(rng, n), _quats(rng, n)
    for k in range(n):
        c = rng.uniform(-3, 3, size=3).astype(np.float32)
        p = rng.uniform(-3, 3, size=3).astype(np.float32)
        r, R = np.float32(rng.uniform(0.0, 2.5)), np.float32(rng.uniform(0.0, 2.5))
        ha = rng.uniform(0.05, 2.0, size=3).astype(np.float32)
        hb = rng.uniform(0.05, 2.0, size=3).astype(np.float32)
        want = _clear(lambda s: _ss64(c, float(r) * s, p, float(R) * s))
        if want is not None:
            assert O.sphere_sphere(c, r, p, R) == want, (k, "sphere-sphere")
            checked["ss"][int(want)] += 1
        want = _clear(lambda s: _sb64(c, float(r) * s, p, qb[k], hb.astype(np.float64) * s))
        if want is not None:
            assert O.sphere_box(c, r, p, qb[k], hb) == want, (k, "sphere-box")
            checked["sb"][int(want)] += 1
        want = _clear(lambda s: _bb64(c, qa[k], ha.astype(np.float64) * s, p, qb[k], hb.astype(np.float64) * s))
        if want is not None:
            assert O.box_box(c, qa[k], ha, p, qb[k], hb) == want, (k, "box-box")
            checked["bb"][int(want)] += 1
    for key, (miss, hit) in checked.items():          # both answers were exercised, and nearly every pose was clear of the margin
        assert miss > n // 10 and hit > n // 10 and miss + hit > 0.99 * n, (key, miss, hit)


def test_touching_counts():
    # tangent spheres (3-4-5: every square exact)
    assert O.sphere_sphere((0, 0, 0), 2.0, (3, 4, 0), 3.0)
    assert not O.sphere_sphere((0, 0, 0), 2.0, (3, 4, 0), 2.9990)
    # a box face on a sphere
    h = (1.0, 2.0, 3.0)
    assert O.sphere_box((1.5, 0.3, -0.2), 0.5, (0, 0, 0), IDENT, h)
    assert O.sphere_box((0.25, -2.75, 1.0), 0.75, (0, 0, 0), IDENT, h)
    assert not O.sphere_box((1.5, 0.3, -0.2), 0.4999, (0, 0, 0), IDENT, h)
    # a sphere on a box edge: (0.375, 0.5) from it, 0.625 away -- every square exact
    assert O.sphere_box((1.375, 2.5, 0.0), 0.625, (0, 0, 0), IDENT, h)
    assert not O.sphere_box((1.375, 2.5, 0.0), 0.6249, (0, 0, 0), IDENT, h)
    # the same box turned half a turn about y (an exact quaternion) and moved
    assert O.sphere_box((6.0, 0.0, 0.0), 1.0, (4.0, 0, 0), (0.0, 1.0, 0.0, 0.0), h)
    # coincident box faces: side by side, stacked, and with the collider turned a half turn
    assert O.box_box((0, 0, 0), IDENT, (1, 1, 1), (2, 0, 0), IDENT, (1, 1, 1))
    assert O.box_box((0, 0, 0), IDENT, (1, 2, 1), (0.5, 3, 0.25), IDENT, (1, 1, 1))
    assert O.box_box((0, 0, 0), IDENT, (1, 1, 1), (0, 0, 2.5), (1.0, 0.0, 0.0, 0.0), (0.5, 0.5, 1.5))
    assert not O.box_box((0, 0, 0), IDENT, (1, 1, 1), (2.001, 0, 0), IDENT, (1, 1, 1))
    # edge on edge at 45 degrees: a turned 45 degrees about x (top edge along x), b turned 45 degrees about z (bottom edge along z), the two edges
    # crossing at one point; both exact only up to rounding of sin / cos 22.5 degrees, which the radii's epsilon covers
    s, co = np.float32(np.sin(np.pi / 8)), np.float32(np.cos(np.pi / 8))
    qx, qz = (s, 0.0, 0.0, co), (0.0, 0.0, s, co)
    top = np.float32(np.sqrt(2.0))
    assert O.box_box((0, 0, 0), qx, (1, 1, 1), (0, 2 * top, 0), qz, (1, 1, 1))
    assert O.box_box((0, 0, 0), qz, (1, 1, 1), (0, 2 * top, 0), qx, (1, 1, 1))
    assert not O.box_box((0, 0, 0), qx, (1, 1, 1), (0, 2 * top + 1e-3, 0), qz, (1, 1, 1))
    # a zero-radius sphere (a point) on a box face, on an edge, inside; and a point on a sphere
    assert O.sphere_box((1.0, 0.5, 0.5), 0.0, (0, 0, 0), IDENT, h)
    assert O.sphere_box((1.0, 2.0, 0.5), 0.0, (0, 0, 0), IDENT, h)
    assert O.sphere_box((0.0, 0.0, 0.0), 0.0, (0, 0, 0), IDENT, h)
    assert not O.sphere_box((1.0001, 0.5, 0.5), 0.0, (0, 0, 0), IDENT, h)
    assert O.sphere_sphere((0, 0, 0), 0.0, (3, 4, 0), 5.0)
    # a point query on a point collider at the same spot
    assert O.sphere_sphere((1, 2, 3), 0.0, (1, 2, 3), 0.0)


def test_nan_anywhere_gives_no_overlap():
    base = {
        "ss": ([(0, 0, 0), 1.0, (0.5, 0, 0), 1.0], O.sphere_sphere),
        "sb": ([(0, 0, 0), 1.0, (0.5, 0, 0), IDENT, (1, 1, 1)], O.sphere_box),
        "bb": ([(0, 0, 0), IDENT, (1, 1, 1), (0.5, 0, 0), IDENT, (1, 1, 1)], O.box_box),
    }
    for key, (args, f) in base.items():
        assert f(*args), key
        for a, v in enumerate(args):
            if np.ndim(v) == 0:
                bad = list(args)
                bad[a] = float("nan")
                assert not f(*bad), (key, a)
            else:
                for j in range(len(v)):
                    w = np.array(v, np.float32)
                    w[j] = np.nan
                    bad = list(args)
                    bad[a] = w
                    assert not f(*bad), (key, a, j)


# ---- the brute force's semantics on hand-built worlds ------------------------------------------------------------------------------------------
_query = overlap_query


def _everything(ignore=NONE):
    return _query(E.NH_SHAPE_SPHERE, (0, 0, 0), (1e5,), ignore=ignore)


def _combined(hits, nbox):
    return hits["collider"].astype(np.int64) + np.where(hits["shape"] == E.NH_SHAPE_BOX, 0, nbox)


def test_ignore_body_drops_every_collider_of_a_compound_body():
    scene = S.compound(12, seed=6)
    rec = O.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    off, hits, total = O.overlap(rec, nbox, _everything())
    assert total == len(rec) and np.array_equal(_combined(hits, nbox), np.arange(len(rec)))
    body = 5
    mine = np.nonzero(rec["body"] == body)[0]
    assert len(mine) == 3                                        # two boxes and a sphere
    off, hits, total = O.overlap(rec, nbox, _everything(ignore=body))
    assert total == len(rec) - 3 and not (hits["body"][:total] == body).any()
    assert np.array_equal(_combined(hits, nbox), np.setdiff1d(np.arange(len(rec)), mine))
    # a point on one of the body's colliders, with and without ignoring it
    c = rec["p"][mine[2]]
    assert body in O.overlap(rec, nbox, _query(E.NH_SHAPE_SPHERE, c, (0.0,)))[1]["body"]
    assert body not in O.overlap(rec, nbox, _query(E.NH_SHAPE_SPHERE, c, (0.0,), ignore=body))[1]["body"]


def test_the_collider_of_a_missing_body_never_appears():
    scene = S.pile(8, 4, seed=3)
    scene["box_transforms"]["body"][3] = 10000
    scene["sphere_transforms"]["body"][1] = 20000
    nbox = len(scene["box_tags"])
    rec = O.records(scene["body_transforms"], scene)
    assert np.isnan(rec["p"][3]).all() and np.isnan(rec["p"][nbox + 1]).all()
    off, hits, total = O.overlap(rec, nbox, _everything())
    assert total == len(rec) - 2
    comb = _combined(hits, nbox)
    assert 3 not in comb and nbox + 1 not in comb
    # a box query over everything, at any rotation, does not find them either
    box = _query(E.NH_SHAPE_BOX, (0, 0, 0), (1e5, 1e5, 1e5), rotation=(0.0, 0.6, 0.0, 0.8))
    assert O.overlap(rec, nbox, box)[2] == len(rec) - 2


def test_records_come_in_combined_index_order_with_boxes_first():
    scene = S.pile(40, 30, seed=2)
    rec = O.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    qs = np.concatenate([_everything(), _query(E.NH_SHAPE_BOX, (0, 150, 0), (6, 160, 6), rotation=(0.0, 0.0, 0.0, 1.0)),
                         _query(E.NH_SHAPE_SPHERE, (0, 150, 0), (80.0,))])
    off, hits, total = O.overlap(rec, nbox, qs)
    for i in range(len(qs)):
        seg = hits[off[i]:off[i + 1]]
        comb = _combined(seg, nbox)
        assert len(seg) > 10 and (np.diff(comb) > 0).all(), i
        assert np.array_equal(seg["shape"], np.where(comb < nbox, E.NH_SHAPE_BOX, E.NH_SHAPE_SPHERE))
        assert np.array_equal(seg["tag"], rec["tag"][comb]) and np.array_equal(seg["body"], rec["body"][comb])
    assert (_combined(hits[:off[1]], nbox) == np.arange(len(rec))).all()


def test_invalid_queries_count_zero():
    scene = S.pile(16, 8, seed=2)
    rec = O.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    invalid, valid = overlap_lists()
    off, hits, total = O.overlap(rec, nbox, np.concatenate(invalid))
    assert total == 0 and not off.any()
    off, hits, total = O.overlap(rec, nbox, np.concatenate(valid))
    counts = np.diff(off.astype(np.int64))
    assert counts[0] == len(rec) and counts[2] == len(rec) and counts[1] >= 0


def test_capacity_writes_a_prefix_of_whole_segments():
    scene = S.pile(16, 8, seed=2)
    rec = O.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    n = len(rec)
    qs = np.concatenate([_everything(), _query(2, (0, 0, 0), (1.0,)), _everything(ignore=0), _everything()])
    full_off, full, total = O.overlap(rec, nbox, qs)
    assert list(full_off) == [0, n, n, 2 * n - 1, 3 * n - 1] and total == 3 * n - 1
    sentinel = np.frombuffer(b"\xa5" * 16 * total, dtype=E.OVERLAP_HIT)
    for cap, written in ((0, 0), (n - 1, 0), (n, n), (n + 1, n), (2 * n - 2, n), (2 * n - 1, 2 * n - 1), (total - 1, 2 * n - 1), (total, total)):
        hits = sentinel.copy()
        off, hits, t = O.overlap(rec, nbox, qs, capacity=cap, hits=hits)
        assert off.tobytes() == full_off.tobytes() and t == total, cap
        assert hits[:written].tobytes() == full[:written].tobytes(), cap
        assert hits[written:].tobytes() == sentinel[written:].tobytes(), cap
