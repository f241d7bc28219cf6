"""k-nearest closest-point queries on the host (no GPU): nh_closest_k's declaration and exports, the bounded ordered list the kernel keeps per lane
(nh_q_nearest_insert, nudge_amd/csrc/nh_query.h, driven through tests/hostnearest_util.py) against a plain sort, and the brute-force oracle of the GPU
tests (hn_closest_k: sort everything, take k) against the single-collider oracle of nh_closest and on hand-made worlds."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostnearest_util as N                 # noqa: E402
import hostpoint_util as H                   # noqa: E402
import hostquery_util as Q                   # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

NONE = 0xFFFFFFFF
IDENTITY = np.float32([0, 0, 0, 1])


def test_the_call_is_declared_exported_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "nudge_hip.h")).read()
    assert re.search(r"#define\s+NH_CLOSEST_K_MAX\s+32u\b", hdr)
    flat = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("int nh_closest_k(nh_context* ctx, const nh_PointQuery* queries, uint32_t count, uint32_t k, uint32_t* counts , nh_PointHit* hits , "
            "uint32_t flags );") in flat, "nh_closest_k's declaration"
    assert "nh_closest_k" in E.EXPORTS
    syms = subprocess.check_output(["nm", "-D", "--defined-only", E._LIB_PATH], text=True)
    assert re.search(r"\bT nh_closest_k$", syms, flags=re.M)
    assert list(inspect.signature(E.World.closest_k).parameters) == ["self", "points", "k", "max_distance", "ignore_body", "synchronize"]
    assert list(inspect.signature(E.World.closest_k_records).parameters) == ["self", "queries", "k", "counts", "hits"]
    # the sentence that named the gap is gone
    assert "Not built: the distance of a shape from the world (GJK), the k nearest colliders" not in hdr


# ---- the list ---------------------------------------------------------------------------------------------------------------------------------
def _first_k(keys, idx, k, max_d):
    """The first k of the sorted unique candidates with key <= max_d: (key, index) ascending."""
    keys, idx = np.asarray(keys, np.float32), np.asarray(idx, np.uint32)
    ok = keys <= np.float32(max_d)                                 # (NaN: False)
    pairs = sorted(set(zip(keys[ok].tolist(), idx[ok].tolist())))
    return np.float32([p[0] for p in pairs[:k]]), np.uint32([p[1] for p in pairs[:k]])


def _stream(rng, n, flavour):
    """A candidate stream: `plain` random keys; `ties` few distinct keys under many indices; `repeats` candidates offered again later (still held
    or long evicted); `wild` keys above any max_d, NaN and negative (inside a collider) keys mixed in."""
    if flavour == "ties":
        keys = rng.choice(np.float32([-0.5, 0.0, 0.25, 0.25, 1.0, 3.0]), size=n)
    else:
        keys = rng.uniform(-1.0, 4.0, size=n).astype(np.float32)
    idx = rng.integers(0, max(4 * n, 8), size=n).astype(np.uint32)
    if flavour == "ties":
        idx = rng.integers(0, 40, size=n).astype(np.uint32)
    if flavour == "repeats" and n > 1:
        for _ in range(n):
            a, b = sorted(rng.integers(0, n, size=2))
            keys[b], idx[b] = keys[a], idx[a]
    if flavour == "wild" and n:
        where = rng.random(n)
        keys[where < 0.15] = np.nan
        keys[(where >= 0.15) & (where < 0.3)] = np.inf
        keys[(where >= 0.3) & (where < 0.4)] = 1e30
    return keys, idx


@pytest.mark.parametrize("stride", [1, 64])
def test_the_list_holds_the_first_k_of_the_sorted_unique_candidates(stride):
    rng = np.random.default_rng(700 + stride)
    N.lib()
    for k in range(1, 33):
        for flavour in ("plain", "ties", "repeats", "wild"):
            for n in (0, 1, 2, k - 1, k, k + 1, int(rng.integers(0, 201)), 200):
                keys, idx = _stream(rng, max(n, 0), flavour)
                for max_d in (np.inf, 0.0, 1.0):
                    lk, li, changed = N.insert(keys, idx, k, stride=stride, max_d=max_d)
                    rk, ri = _first_k(keys, idx, k, max_d)
                    assert np.array_equal(lk.view(np.uint32), rk.view(np.uint32)) and np.array_equal(li, ri), (k, flavour, n, max_d)
                    # a refused candidate changed nothing: NaN keys, keys above max_d
                    assert not changed[~(keys <= np.float32(max_d))].any()


def test_a_repeat_is_dropped_whether_it_is_still_held_or_was_evicted():
    # (1.0, 7) is held and offered again: one entry.  Then four nearer candidates evict it from a list of 4; offered again it stays out.
    keys = np.float32([1.0, 2.0, 1.0, 0.1, 0.2, 0.3, 0.4, 1.0])
    idx = np.uint32([7, 3, 7, 10, 11, 12, 13, 7])
    lk, li, changed = N.insert(keys, idx, 4)
    assert list(changed) == [True, True, False, True, True, True, True, False]
    assert list(li) == [10, 11, 12, 13] and list(lk) == list(np.float32([0.1, 0.2, 0.3, 0.4]))
    # equal keys: strictly by index, and an equal key with a HIGHER index than the last does not enter a full list
    lk, li, changed = N.insert(np.float32([0.5] * 6), np.uint32([9, 4, 6, 4, 2, 8]), 3)
    assert list(li) == [2, 4, 6] and list(changed) == [True, True, True, False, True, False]
    # k = 1 is nh_closest's rule
    lk, li, _ = N.insert(np.float32([3, 1, 1, 2]), np.uint32([0, 5, 4, 1]), 1)
    assert list(li) == [4] and lk[0] == 1.0
    # exactly max_d counts, the next float above does not
    lk, li, _ = N.insert(np.float32([2.0, np.nextafter(np.float32(2.0), np.float32(3.0))]), np.uint32([1, 0]), 4, max_d=2.0)
    assert list(li) == [1]


# ---- the oracle against nh_closest's ----------------------------------------------------------------------------------------------------------------
SCENES = {"pile": lambda: S.pile(256, 64, seed=1), "compound": lambda: S.compound(150, seed=6), "ball_pit": lambda: S.ball_pit(6, 6, 6, seed=4)}


def _query(points, max_distance=np.inf, ignore_body=NONE):
    q = np.zeros(len(points), dtype=E.POINT_QUERY)
    q["point"], q["max_distance"], q["ignore_body"] = points, max_distance, ignore_body
    return q


def _combined(hits, nbox):
    return np.where(hits["shape"] == E.NH_SHAPE_SPHERE, hits["collider"].astype(np.int64) + nbox, hits["collider"].astype(np.int64))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_oracle_agrees_with_the_single_collider_oracle(name):
    scene = SCENES[name]()
    rec = Q.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    rng = np.random.default_rng(710 + sorted(SCENES).index(name))
    live = rec["p"].astype(np.float64)
    n = 600
    pts = np.concatenate([live[rng.integers(0, len(live), size=n // 2)] + rng.normal(scale=0.4, size=(n // 2, 3)),
                          rng.uniform(live.min(axis=0) - 2, live.max(axis=0) + 2, size=(n // 2, 3))])
    q = _query(pts, max_distance=rng.choice(np.float32([np.inf, 0.0, 0.5, 2.0]), size=n))
    q["ignore_body"][::4] = rng.integers(0, len(scene["body_transforms"]), size=len(q[::4]))
    # k = 1: nh_closest's bytes
    c1, h1 = N.closest_k(rec, nbox, q, 1)
    ref = H.closest(rec, nbox, q)
    assert h1[:, 0].tobytes() == ref.tobytes() and np.array_equal(c1, (ref["shape"] != NONE).astype(np.uint32))
    # prefix: k = 3 against k = 8
    c3, h3 = N.closest_k(rec, nbox, q, 3)
    c8, h8 = N.closest_k(rec, nbox, q, 8)
    assert h8[:, :3].tobytes() == h3.tobytes() and np.array_equal(c3, np.minimum(c8, 3))
    assert (c8 == 8).any() and (c8 == 0).any() and ((c8 > 0) & (c8 < 8)).any()
    # every listed record is what nh_closest gives for that collider alone; the rest are nh_closest's miss records
    comb = _combined(h8, nbox)
    for i in range(0, n, 7):
        for j in range(8):
            if j < c8[i]:
                alone = H.closest(rec, nbox, q[i:i + 1], only=int(comb[i, j]))[0]
                assert h8[i, j].tobytes() == alone.tobytes(), (i, j)
            else:
                assert h8[i, j]["shape"] == NONE and h8[i, j]["distance"] == q["max_distance"][i] and h8[i, j]["body"] == NONE
    # non-decreasing distances, ties in index order; nothing listed twice, nothing of the ignored body, nothing beyond max_distance
    for i in range(n):
        m = int(c8[i])
        d, c = h8[i, :m]["distance"], comb[i, :m]
        assert (np.diff(d) >= 0).all() and (np.diff(c)[np.diff(d) == 0] > 0).all() and len(set(c.tolist())) == m
        assert (d <= q["max_distance"][i]).all() and (h8[i, :m]["body"] != q["ignore_body"][i]).all()


# ---- hand-made worlds -------------------------------------------------------------------------------------------------------------------------------
def _rec(colliders):
    """Records of (kind, position, rotation, size, body): boxes first, as the build numbers them."""
    rec = np.zeros(len(colliders), dtype=Q.REC)
    for i, (kind, p, q, h, body) in enumerate(colliders):
        rec[i]["p"], rec[i]["q"], rec[i]["body"], rec[i]["tag"] = p, q, body, 100 + i
        rec[i]["h"] = h if kind == "box" else (h, h, h)
    return rec, sum(1 for k in colliders if k[0] == "box")


def test_three_spheres_at_known_distances():
    rec, nbox = _rec([("sphere", (10, 0, 0), IDENTITY, 1.0, 1), ("sphere", (-4, 0, 0), IDENTITY, 1.0, 2), ("sphere", (0, 6, 0), IDENTITY, 2.0, 3)])
    counts, hits = N.closest_k(rec, nbox, _query([(0, 0, 0)]), 4)
    assert counts[0] == 3 and list(hits[0]["distance"]) == [3.0, 4.0, 9.0, np.inf]
    assert list(hits[0]["collider"]) == [1, 2, 0, NONE] and list(hits[0]["body"]) == [2, 3, 1, NONE] and list(hits[0]["tag"]) == [101, 102, 100, NONE]
    assert list(hits[0]["shape"]) == [1, 1, 1, NONE] and not hits[0]["reserved"].any()
    assert np.array_equal(hits[0]["normal"][:3], np.float32([[1, 0, 0], [0, -1, 0], [-1, 0, 0]]))
    assert np.array_equal(hits[0]["point"][:3], np.float32([[-3, 0, 0], [0, 4, 0], [9, 0, 0]]))
    # max_distance cuts the list: exactly 4.0 still counts
    counts, hits = N.closest_k(rec, nbox, _query([(0, 0, 0)], max_distance=4.0), 4)
    assert counts[0] == 2 and list(hits[0]["distance"]) == [3.0, 4.0, 4.0, 4.0] and list(hits[0]["shape"]) == [1, 1, NONE, NONE]
    # k below the candidates: the nearest k
    counts, hits = N.closest_k(rec, nbox, _query([(0, 0, 0)]), 2)
    assert counts[0] == 2 and list(hits[0]["collider"]) == [1, 2]
    # ignore_body takes the nearest out
    counts, hits = N.closest_k(rec, nbox, _query([(0, 0, 0)], ignore_body=2), 4)
    assert counts[0] == 2 and list(hits[0]["body"]) == [3, 1, NONE, NONE]
    # max_distance 0: only what contains or touches the point, the deepest first
    counts, hits = N.closest_k(rec, nbox, _query([(0, 5, 0)], max_distance=0.0), 4)
    assert counts[0] == 1 and hits[0]["distance"][0] == -1.0 and hits[0]["body"][0] == 3


def test_coincident_equal_colliders_tie_strictly_by_index():
    rec, nbox = _rec([("box", (1, 2, 3), IDENTITY, (0.5, 0.5, 0.5), 1 + i) for i in range(6)] + [("sphere", (1, 2, 3), IDENTITY, 0.5, 10 + i) for i in range(3)])
    counts, hits = N.closest_k(rec, nbox, _query([(1, 2, 3), (4, 2, 3)]), 8)
    assert list(counts) == [8, 8]
    for i in (0, 1):                         # at the centre all nine are 0.5 deep; from outside the boxes and the balls are 2.5 away
        assert len(set(hits[i]["distance"].tolist())) == 1
        assert list(_combined(hits[i], nbox)) == [0, 1, 2, 3, 4, 5, 6, 7]
    counts, hits = N.closest_k(rec, nbox, _query([(1, 2, 3)], ignore_body=3), 8)
    assert list(_combined(hits[0], nbox)) == [0, 1, 3, 4, 5, 6, 7, 8]


def test_invalid_queries_and_nan_poses():
    rec, nbox = _rec([("box", (0, 0, 0), IDENTITY, (1, 1, 1), 1), ("sphere", (0, 0, 0), IDENTITY, 1.0, 2), ("sphere", (3, 0, 0), IDENTITY, 1.0, 3)])
    pts = np.float32([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0, 0, 0], [0, 0, 0]])
    q = _query(pts)
    q["max_distance"][3], q["max_distance"][4] = np.nan, -1.0
    counts, hits = N.closest_k(rec, nbox, q, 3)
    assert not counts.any() and np.isnan(hits["distance"]).all() and (hits["shape"] == NONE).all() and not hits["normal"].any() and not hits["point"].any()
    assert (hits["body"] == NONE).all() and (hits["collider"] == NONE).all() and (hits["tag"] == NONE).all() and not hits["reserved"].any()
    # a collider of a NaN pose is never listed, even where k exceeds what remains
    rec["p"][1] = np.nan
    rec["q"][1] = np.nan
    counts, hits = N.closest_k(rec, nbox, _query([(0, 0, 0), (5, 5, 5)]), 3)
    assert list(counts) == [2, 2] and (hits[:, 2]["shape"] == NONE).all() and np.isinf(hits[:, 2]["distance"]).all()
    assert sorted(hits[0, :2]["body"].tolist()) == [1, 3] and sorted(hits[1, :2]["body"].tolist()) == [1, 3]
