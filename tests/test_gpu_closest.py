"""Closest-point queries on the GPU (pytest -m gpu): nh_closest (include/nudge_hip.h, "scene queries").

The oracle is a brute force over every collider on the host with the same arithmetic (nudge_amd/csrc/nh_query.h through tests/hostpoint_util.py)
and the header's exact rules -- the reach rule included -- so the tree walk's answer must equal it in every byte of every record.  Queries are
observers like the other queries."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostpoint_util as H                   # noqa: E402
import hostquery_util as Q                   # noqa: E402
from query_util import OBSERVED, SMALL, bounds as _bounds, same_stepped_world as _same_stepped_world, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
FUSED = E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP


def _queries(points, max_distance=np.inf, ignore_body=NONE):
    q = np.zeros(len(points), dtype=E.POINT_QUERY)
    q["point"] = points
    q["max_distance"] = max_distance
    q["ignore_body"] = ignore_body
    return q


def _points(rng, n, rec, lo, hi, kind):
    """`kind`: near collider centres (inside piles: negative distances); uniform over the scene's bounds; far above the world."""
    live = rec["p"][np.isfinite(rec["p"]).all(axis=1)].astype(np.float64)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    span = np.maximum(hi - lo, 1.0)
    if kind == "inside":
        return live[rng.integers(0, len(live), size=n)] + rng.normal(scale=0.3, size=(n, 3))
    if kind == "uniform":
        return rng.uniform(lo - 0.2 * span, hi + 0.2 * span, size=(n, 3))
    p = rng.uniform(lo, hi, size=(n, 3))
    p[:, 1] = hi[1] + 20.0
    return p


def _closest(w, queries):
    raw = w.closest_records(_upload(w, queries))
    return np.frombuffer(raw.cpu().numpy().tobytes(), dtype=E.POINT_HIT).copy()


def _same_hits(got, ref, what):
    bad = (got.view(np.uint8).reshape(-1, 48) != ref.view(np.uint8).reshape(-1, 48)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(ref)} hit records differ, first at {int(np.argmax(bad))}: {got[bad][:1]} vs {ref[bad][:1]}"


def _check_world(w, scene, rng, n, what):
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    if not len(rec):
        q = _queries(rng.uniform(-5, 5, size=(n, 3)))
        _same_hits(_closest(w, q), H.closest(rec, w.nbox, q), f"{what} / empty")
        return []
    lo, hi = _bounds(rec)
    share = []
    for kind in ("inside", "uniform", "above"):
        q = _queries(_points(rng, n, rec, lo, hi, kind))
        ref = H.closest(rec, w.nbox, q)
        _same_hits(_closest(w, q), ref, f"{what} / {kind}")
        share.append(float((ref["distance"] < 0).mean()))
        if kind == "inside":
            # the nearest surface points of those queries, queried themselves: distances at or next to zero
            s = ref["shape"] != NONE
            q2 = _queries(ref["point"][s])
            _same_hits(_closest(w, q2), H.closest(rec, w.nbox, q2), f"{what} / on surfaces")
    return share


@pytest.mark.parametrize("name", sorted(SMALL))
def test_closest_points_equal_the_brute_force_before_and_after_stepping(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(600 + sorted(SMALL).index(name))
    w = E.World(scene, flags=FUSED)
    assert max(_check_world(w, scene, rng, 16384, f"{name} initial")) > 0.05
    w.step(50)
    assert max(_check_world(w, scene, rng, 16384, f"{name} after 50 steps")) > 0.05
    w.close()


def test_degenerate_worlds():
    rng = np.random.default_rng(61)
    scene = S.pile(4, 0, seed=3)
    w = E.World(scene, flags=FUSED)
    w.set_counts(len(scene["body_transforms"]), 0, 0)          # no collider at all: every query misses
    w.query_build()
    q = _queries(rng.uniform(-5, 5, size=(1024, 3)), max_distance=rng.choice([np.inf, 1.0, 0.0], size=1024))
    got = _closest(w, q)
    assert (got["shape"] == NONE).all() and np.array_equal(got["distance"], q["max_distance"])
    _same_hits(got, H.closest(np.zeros(0, dtype=Q.REC), 0, q), "no collider")
    w.set_counts(len(scene["body_transforms"]), 1, 0)          # the ground slab alone (body 0)
    _check_world(w, scene, rng, 2048, "one collider")
    w.close()

    scene = S.pile(4096, 0, seed=3)
    scene["body_transforms"]["position"][1:] = (0.25, 3.0, -0.5)        # every Morton key equal but the ground's
    w = E.World(scene, flags=FUSED)
    _check_world(w, scene, rng, 2048, "4096 coincident boxes")
    q = _queries(np.tile([0.25, 3.0, -0.5], (64, 1)))                       # at the common centre: the deepest box wins
    got = _closest(w, q)
    _same_hits(got, H.closest(Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph), w.nbox, q), "the common centre")
    assert (got["shape"] == E.NH_SHAPE_BOX).all() and (got["distance"] < -0.4).all() and len(np.unique(got["collider"])) == 1
    w.close()


def test_mixed_max_distance_and_ignore_body():
    scene = SMALL["pile"]()
    w = E.World(scene, flags=FUSED)
    w.step(30)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(62)
    n = 16384
    p = np.concatenate([_points(rng, n // 2, rec, lo, hi, "inside"), _points(rng, n // 2, rec, lo, hi, "uniform")])
    q = _queries(p, max_distance=rng.choice(np.float32([np.inf, 0.0, 0.1, 0.5, 2.0]), size=n))
    q["ignore_body"][::3] = rng.integers(0, 64, size=len(q[::3]))
    bad = rng.choice(n, size=64, replace=False)
    q["point"][bad[:16], 0] = np.nan
    q["point"][bad[16:32], 2] = np.inf
    q["max_distance"][bad[32:48]] = np.nan
    q["max_distance"][bad[48:]] = -1.0
    ref = H.closest(rec, w.nbox, q)
    assert np.isnan(ref["distance"][bad]).all() and (ref["shape"][bad] == NONE).all()
    _same_hits(_closest(w, q), ref, "mixed")
    hit = ref["shape"] != NONE
    assert hit.mean() > 0.3 and (~hit).mean() > 0.05
    assert (ref["body"][hit][::3] != q["ignore_body"][hit][::3]).all()
    w.close()


def test_nan_pose_colliders_are_never_reported():
    scene = S.pile(256, 64, seed=1)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    w.set_counts(nb - 10, w.nbox, w.nsph)                  # the last 10 spheres belong to bodies that no longer exist: NaN poses
    w.query_build()
    bt = w.get_bodies()["transforms"]
    rec = Q.records(bt[: nb - 10], scene, w.nbox, w.nsph)
    assert np.isnan(rec["p"][-10:]).all() and np.isfinite(rec["p"][:-10]).all()
    where = Q.records(bt, scene, w.nbox, w.nsph)["p"][-10:]
    rng = np.random.default_rng(63)
    q = _queries(np.repeat(where, 64, axis=0) + rng.normal(scale=0.2, size=(640, 3)), max_distance=rng.choice([np.inf, 0.0, 1.0], size=640))
    got = _closest(w, q)
    _same_hits(got, H.closest(rec, w.nbox, q), "NaN pose")
    assert not ((got["shape"] == E.NH_SHAPE_SPHERE) & (got["collider"] >= w.nsph - 10)).any()
    w.close()


def test_abi_edge_cases():
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    L = w.L
    q = _queries(np.random.default_rng(64).uniform(-5, 5, size=(1024, 3)))
    t = _upload(w, q)
    import torch
    hits = torch.zeros((1025, 48), dtype=torch.uint8, device=w.dev)
    hp = hits.data_ptr()
    assert L.nh_closest(w.ctx, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hp), 0) == 1          # before any build: NH_ERR_INVALID
    assert L.nh_closest(None, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hp), 0) == 1
    w.query_build()
    assert L.nh_closest(w.ctx, C.c_void_p(t.data_ptr()), 0, C.c_void_p(hp), 0) == 0            # count 0: a no-op
    assert L.nh_closest(w.ctx, None, 0, None, 0) == 0
    assert L.nh_closest(w.ctx, C.c_void_p(t.data_ptr()), 1024, None, 0) == 1                    # null hits / queries
    assert L.nh_closest(w.ctx, None, 1024, C.c_void_p(hp), 0) == 1
    assert L.nh_closest(w.ctx, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hp), 1) == 1           # flags other than 0
    assert L.nh_closest(w.ctx, C.c_void_p(t.data_ptr() + 4), 1023, C.c_void_p(hp), 0) == 1       # misaligned queries / hits
    assert L.nh_closest(w.ctx, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hp + 8), 0) == 1
    w.torch.cuda.synchronize()
    assert int(hits.sum()) == 0                                                                   # nothing was written
    assert L.nh_closest(w.ctx, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hp), 0) == 0
    w.torch.cuda.synchronize()
    assert int(hits[1024].sum()) == 0                                                             # nothing behind the last record
    # the world shrinks and grows back: the rebuild answers with the colliders there are
    rng = np.random.default_rng(65)
    w.set_counts(len(scene["body_transforms"]), 33, 8)
    _check_world(w, scene, rng, 1024, "after set_counts")
    w.set_counts(len(scene["body_transforms"]), 65, 16)
    _check_world(w, scene, rng, 1024, "grown back")
    w.close()


def test_the_python_wrappers_write_the_records_they_describe():
    scene = SMALL["grid_tiles"]()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(66)
    p = _points(rng, 2048, rec, lo, hi, "inside").astype(np.float32)
    md = rng.choice(np.float32([np.inf, 0.25, 1.0]), size=2048)
    ign = rng.integers(0, 40, size=2048)
    out = w.closest(p, max_distance=md, ignore_body=ign, synchronize=True)
    ref = H.closest(rec, w.nbox, _queries(p, md, ign))
    _same_hits(np.frombuffer(out["raw"].cpu().numpy().tobytes(), dtype=E.POINT_HIT), ref, "closest()")
    assert np.array_equal(out["distance"].cpu().numpy().view(np.uint32), ref["distance"].view(np.uint32))
    assert np.array_equal(out["normal"].cpu().numpy(), ref["normal"]) and np.array_equal(out["point"].cpu().numpy(), ref["point"])
    for k in ("body", "collider", "shape", "tag"):
        assert np.array_equal(out[k].cpu().numpy(), ref[k].astype(np.int64)), k
    # defaults: +inf, nothing ignored -- every query finds a collider
    out = w.closest(p[:16], synchronize=True)
    assert (out["shape"].cpu().numpy() != NONE).all()
    _same_hits(np.frombuffer(out["raw"].cpu().numpy().tobytes(), dtype=E.POINT_HIT), H.closest(rec, w.nbox, _queries(p[:16])), "closest() defaults")
    w.close()


# ---- observers -----------------------------------------------------------------------------------------------------------------------------
def _query(w, queries_t, hits_t):
    w.query_build()
    w.closest_records(queries_t, hits=hits_t)


@pytest.mark.parametrize("name", sorted(OBSERVED))
def test_closest_queries_between_calls_change_nothing(name):
    scene = OBSERVED[name]()
    rng = np.random.default_rng(67)
    q = _queries(rng.uniform((-30, -12, -30), (30, 20, 30), size=(4096, 3)), max_distance=rng.choice([np.inf, 1.0], size=4096))
    # between nh_step calls
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    qt = _upload(a, q)
    ht = a.torch.empty((4096, 48), dtype=a.torch.uint8, device=a.dev)
    done = 0
    for k in [1, 2, 3, 5, 7, 4, 8] * 10:
        k = min(k, 300 - done)
        if k <= 0:
            break
        _query(a, qt, ht)
        a.step(k)
        b.step(k)
        done += k
    _query(a, qt, ht)
    _same_stepped_world(a, b, f"{name} nh_step")
    if name == "grid_tiles":
        assert a.counts()["still_steps"] > 0, a.counts()
    a.close(); b.close()
    # between every call of the fused step
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    qt = _upload(a, q)
    ht = a.torch.empty((4096, 48), dtype=a.torch.uint8, device=a.dev)
    for s in range(300):
        for call in ("collide", "gravity", "read_cache", "setup", "apply", "update", "write_cache", "advance"):
            _query(a, qt, ht)
            getattr(a, call)()
            getattr(b, call)()
        a.step_done(); b.step_done()
    _query(a, qt, ht)
    _same_stepped_world(a, b, f"{name} call by call")
    if name == "grid_tiles":
        assert a.counts()["still_steps"] > 0, a.counts()
    a.close(); b.close()


# ---- at size -------------------------------------------------------------------------------------------------------------------------------
def test_a_million_closest_point_queries_on_the_landed_config_2_world():
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED, max_contacts=6 * nb)
    w.step(70)
    assert w.counts()["error"] == 0
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(68)
    n = 1 << 20
    k = n // 4
    live = rec["p"][1 + 124:].astype(np.float64)
    near = live[rng.integers(0, len(live), size=k)] + rng.normal(scale=0.5, size=(k, 3))
    q = np.concatenate([_queries(near, 2.0), _queries(_points(rng, k, rec, lo, hi, "uniform")), _queries(_points(rng, k, rec, lo, hi, "above")),
                        _queries(_points(rng, n - 3 * k, rec, lo, hi, "inside"), rng.choice(np.float32([np.inf, 0.0, 0.5]), size=n - 3 * k))])
    got = _closest(w, q)
    assert (got["shape"][k:3 * k] != NONE).all()                          # +inf: every query finds a collider
    assert (got["distance"][:k][got["shape"][:k] != NONE] <= 2.0).all()
    assert (got["distance"][2 * k:3 * k] > 0).all() and (got["distance"][3 * k:] < 0).mean() > 0.2
    # 2048 queries spread over the batch, byte for byte against the brute force over all 1,004,524 colliders
    pick = np.linspace(0, n - 1, 2048).astype(np.int64)
    _same_hits(got[pick], H.closest(rec, w.nbox, q[pick]), "config 2, 1 M closest-point queries")
    w.close()
