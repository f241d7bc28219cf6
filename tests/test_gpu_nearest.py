"""k-nearest closest-point queries on the GPU (pytest -m gpu): nh_closest_k (include/nudge_hip.h, "scene queries").

The oracle is a brute force on the host that evaluates every collider with the same arithmetic, sorts ALL candidates and takes the first k
(tests/hostnearest_util.py); the kernel's pruned walk with its bounded lists must equal it in every byte of all count * k records and in every count.
Queries are observers like the other queries."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostnearest_util as N                 # noqa: E402
import hostquery_util as Q                   # noqa: E402
from test_gpu_closest import _closest, _points, _queries                                 # noqa: E402
from query_util import OBSERVED, SMALL, bounds as _bounds, same_stepped_world as _same_stepped_world, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
FUSED = E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP
# 1, 2, 3, 8, 32 and both sides of the kernel's block-size boundaries (k <= 8: 256 lanes, k <= 16: 128, above: 64)
KS = (1, 2, 3, 8, 9, 16, 17, 32)


def _nearest(w, queries, k):
    """(counts, hits (n, k)) of the GPU; the buffers carry a guard word / record behind the end that must stay as it was."""
    import torch
    n = len(queries)
    counts = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int32, device=w.dev)
    hits = torch.full((n * k + 1, 48), 0xA5, dtype=torch.uint8, device=w.dev)
    w.closest_k_records(_upload(w, queries), k, counts=counts, hits=hits)
    c = counts.cpu().numpy().view(np.uint32)
    h = np.frombuffer(hits.cpu().numpy().tobytes(), dtype=E.POINT_HIT)
    assert c[n] == 0x5A5A5A5A and (h[n * k:].view(np.uint8) == 0xA5).all(), "written behind the end"
    return c[:n].copy(), h[:n * k].reshape(n, k).copy()


def _same(got, ref, what):
    (gc, gh), (rc, rh) = got, ref
    k = rh.shape[1]
    bad = (gh.view(np.uint8).reshape(-1, 48 * k) != rh.view(np.uint8).reshape(-1, 48 * k)).any(axis=1) | (gc != rc)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {len(rc)} queries differ, first at {int(np.argmax(bad))}: counts {gc[bad][:1]} vs {rc[bad][:1]}, "
                           f"{gh[bad][:1]} vs {rh[bad][:1]}")


def _check_world(w, scene, rng, n, what, ks=KS):
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    full = []
    for kind in ("inside", "uniform", "above"):
        q = _queries(_points(rng, n, rec, lo, hi, kind))
        single = _closest(w, q)
        for k in ks:
            ref = N.closest_k(rec, w.nbox, q, k)
            got = _nearest(w, q, k)
            _same(got, ref, f"{what} / {kind} / k {k}")
            if k == 1:
                assert got[1][:, 0].tobytes() == single.tobytes(), f"{what} / {kind}: k = 1 is not nh_closest"
            full.append(float((ref[0] == k).mean()))
    return full


@pytest.mark.parametrize("name", sorted(SMALL))
def test_the_k_nearest_equal_the_brute_force_before_and_after_stepping(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(800 + sorted(SMALL).index(name))
    w = E.World(scene, flags=FUSED)
    assert min(_check_world(w, scene, rng, 4097, f"{name} initial")) == 1.0          # +inf: every list is full
    w.step(50)
    assert min(_check_world(w, scene, rng, 4097, f"{name} after 50 steps")) == 1.0
    w.close()


def _mixed_queries(rng, rec, lo, hi, n):
    """Half the points around collider centres, half over the scene's bounds; max_distance from {inf, 0, 0.1, 0.5, 2}, a third with a body ignored,
    64 invalid queries.  Returns (queries, indices of the invalid ones)."""
    p = np.concatenate([_points(rng, n // 2, rec, lo, hi, "inside"), _points(rng, n - n // 2, rec, lo, hi, "uniform")])
    q = _queries(p, max_distance=rng.choice(np.float32([np.inf, 0.0, 0.1, 0.5, 2.0]), size=n))
    q["ignore_body"][::3] = rng.integers(0, 64, size=len(q[::3]))
    bad = rng.choice(n, size=64, replace=False)
    q["point"][bad[:16], 0] = np.nan
    q["point"][bad[16:32], 2] = np.inf
    q["max_distance"][bad[32:48]] = np.nan
    q["max_distance"][bad[48:]] = -1.0
    return q, bad


def test_mixed_max_distance_and_ignore_body():
    scene = SMALL["pile"]()
    w = E.World(scene, flags=FUSED)
    w.step(30)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    q, bad = _mixed_queries(np.random.default_rng(82), rec, lo, hi, 4097)
    k = 8
    ref = N.closest_k(rec, w.nbox, q, k)
    rc, rh = ref
    assert not rc[bad].any() and np.isnan(rh["distance"][bad]).all() and (rh["shape"][bad] == NONE).all()
    _same(_nearest(w, q, k), ref, "mixed")
    valid = np.ones(len(q), dtype=bool)
    valid[bad] = False
    m = rc[valid]
    assert (m == k).mean() >= 0.05 and ((m >= 1) & (m < k)).mean() >= 0.05 and (m == 0).mean() >= 0.05, np.bincount(m, minlength=k + 1)
    listed = rh["shape"] != NONE
    assert (rh["body"][::3][listed[::3]] != np.broadcast_to(q["ignore_body"][::3, None], rh[::3].shape)[listed[::3]]).all()
    w.close()


def test_degenerate_worlds():
    rng = np.random.default_rng(83)
    scene = S.pile(4, 0, seed=3)
    w = E.World(scene, flags=FUSED)
    w.set_counts(len(scene["body_transforms"]), 0, 0)          # no collider at all: every record is a miss
    w.query_build()
    q = _queries(rng.uniform(-5, 5, size=(1024, 3)), max_distance=rng.choice([np.inf, 1.0, 0.0], size=1024))
    gc, gh = _nearest(w, q, 8)
    assert not gc.any() and (gh["shape"] == NONE).all() and np.array_equal(gh["distance"], np.repeat(q["max_distance"][:, None], 8, axis=1))
    _same((gc, gh), N.closest_k(np.zeros(0, dtype=Q.REC), 0, q, 8), "no collider")
    w.set_counts(len(scene["body_transforms"]), 1, 0)          # the ground slab alone (body 0), k = 8
    _check_world(w, scene, rng, 1025, "one collider", ks=(1, 8))
    w.set_counts(len(scene["body_transforms"]), 5, 0)          # k larger than the collider count
    full = _check_world(w, scene, rng, 1025, "five colliders", ks=(4, 5, 6, 32))
    assert max(full[2:4]) == 0.0 and min(full[0:2]) == 1.0
    w.close()

    scene = S.pile(4096, 0, seed=3)
    scene["body_transforms"]["position"][1:] = (0.25, 3.0, -0.5)        # every Morton key equal but the ground's
    scene["box_data"]["size"][1:] = (0.5, 0.5, 0.5)                      # and every box the same: at the centre all of them tie
    w = E.World(scene, flags=FUSED)
    _check_world(w, scene, rng, 1025, "4096 coincident boxes", ks=(1, 8, 32))
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    q = _queries(np.tile([0.25, 3.0, -0.5], (64, 1)))
    got = _nearest(w, q, 32)
    _same(got, N.closest_k(rec, w.nbox, q, 32), "the common centre")
    assert (got[0] == 32).all() and (got[1]["distance"] == -0.5).all() and (got[1]["shape"] == E.NH_SHAPE_BOX).all()
    assert (got[1]["collider"] == np.arange(1, 33)).all()                # the 32 lowest box indices that tie
    body = int(rec["body"][5])
    q["ignore_body"] = body
    got = _nearest(w, q, 32)
    _same(got, N.closest_k(rec, w.nbox, q, 32), "the common centre, one ignored")
    assert (got[1]["collider"] == np.array([c for c in range(1, 34) if c != 5])).all()     # the next index moves up
    w.close()


def test_nan_pose_colliders_are_never_listed():
    scene = S.pile(24, 16, seed=1)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    w.set_counts(nb - 10, w.nbox, w.nsph)                  # the last 10 spheres belong to bodies that no longer exist: NaN poses
    w.query_build()
    bt = w.get_bodies()["transforms"]
    rec = Q.records(bt[: nb - 10], scene, w.nbox, w.nsph)
    assert np.isnan(rec["p"][-10:]).all() and np.isfinite(rec["p"][:-10]).all()
    where = Q.records(scene["body_transforms"], scene, w.nbox, w.nsph)["p"][-10:]          # where those spheres stood (the world has not stepped)
    assert np.isfinite(where).all()
    rng = np.random.default_rng(84)
    q = _queries(np.repeat(where, 64, axis=0) + rng.normal(scale=0.2, size=(640, 3)), max_distance=rng.choice([np.inf, 0.0, 1.0], size=640))
    live = len(rec) - 10
    for k in (8, 32):                                      # 32 exceeds the 31 that remain: the list ends early rather than take a NaN pose
        ref = N.closest_k(rec, w.nbox, q, k)
        got = _nearest(w, q, k)
        _same(got, ref, f"NaN pose, k {k}")
        assert not ((got[1]["shape"] == E.NH_SHAPE_SPHERE) & (got[1]["collider"] >= w.nsph - 10)).any()
        assert got[0].max() == min(k, live)
    w.close()


def test_a_refit_answers_as_a_build_does():
    scene = SMALL["pile"]()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    w.step(20)
    w.query_refit()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(85)
    q = np.concatenate([_queries(_points(rng, 2049, rec, lo, hi, "inside"), rng.choice(np.float32([np.inf, 0.5]), size=2049)),
                        _queries(_points(rng, 2048, rec, lo, hi, "uniform"))])
    refit = {k: _nearest(w, q, k) for k in (1, 8, 32)}
    w.query_build()
    for k, got in refit.items():
        _same(got, _nearest(w, q, k), f"refit against build, k {k}")
        _same(got, N.closest_k(rec, w.nbox, q, k), f"refit against the brute force, k {k}")
    w.close()


def test_abi_edge_cases():
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    L = w.L
    import torch
    n, k = 1024, 4
    q = _queries(np.random.default_rng(86).uniform(-5, 5, size=(n, 3)))
    t = _upload(w, q)
    hits = torch.zeros((n * k + 1, 48), dtype=torch.uint8, device=w.dev)
    counts = torch.zeros(n + 1, dtype=torch.int32, device=w.dev)
    qp, hp, cp = t.data_ptr(), hits.data_ptr(), counts.data_ptr()

    def call(ctx, queries, count, kk, cnt, hit, flags):
        return L.nh_closest_k(ctx, C.c_void_p(queries) if queries else None, count, kk, C.c_void_p(cnt) if cnt else None, C.c_void_p(hit) if hit else None, flags)

    assert call(w.ctx, qp, n, k, cp, hp, 0) == 1                  # before any build: NH_ERR_INVALID
    assert call(None, qp, n, k, cp, hp, 0) == 1
    w.query_build()
    assert call(None, qp, n, k, cp, hp, 0) == 1
    assert call(w.ctx, qp, 0, k, cp, hp, 0) == 0                  # count 0: a no-op
    assert call(w.ctx, None, 0, k, None, None, 0) == 0
    assert call(w.ctx, qp, n, 0, cp, hp, 0) == 1                  # k = 0, k = 33
    assert call(w.ctx, qp, n, 33, cp, hp, 0) == 1
    assert call(w.ctx, qp, n, k, cp, hp, 1) == 1                  # flags other than 0
    assert call(w.ctx, None, n, k, cp, hp, 0) == 1                # null queries / hits
    assert call(w.ctx, qp, n, k, cp, None, 0) == 1
    assert call(w.ctx, qp + 4, n - 1, k, cp, hp, 0) == 1          # misaligned queries / hits / counts
    assert call(w.ctx, qp, n, k, cp, hp + 8, 0) == 1
    assert call(w.ctx, qp, n - 1, k, cp + 2, hp, 0) == 1
    assert call(w.ctx, qp, 1 << 30, k, cp, hp, 0) == 1            # count >= 2^30
    torch.cuda.synchronize()
    assert int(hits.sum()) == 0 and int(counts.sum()) == 0        # the refused calls wrote nothing
    assert call(w.ctx, qp, n, k, None, hp, 0) == 0                # counts = NULL is accepted
    torch.cuda.synchronize()
    without = hits.cpu().numpy().copy()
    assert int(counts.sum()) == 0 and not without[n * k].any()    # nothing behind the last record
    assert call(w.ctx, qp, n, k, cp, hp, 0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(hits.cpu().numpy(), without) and int(counts[n]) == 0
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    rc, rh = N.closest_k(rec, w.nbox, q, k)
    assert without[:n * k].tobytes() == rh.tobytes() and np.array_equal(counts[:n].cpu().numpy().view(np.uint32), rc)
    w.close()


def test_the_python_wrapper_returns_the_fields_of_the_records():
    scene = SMALL["grid_tiles"]()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(87)
    n, k = 1025, 5
    p = _points(rng, n, rec, lo, hi, "inside").astype(np.float32)
    md = rng.choice(np.float32([np.inf, 0.25, 1.0]), size=n)
    ign = rng.integers(0, 40, size=n)
    out = w.closest_k(p, k, max_distance=md, ignore_body=ign, synchronize=True)
    rc, rh = N.closest_k(rec, w.nbox, _queries(p, md, ign), k)
    assert out["raw"].cpu().numpy().tobytes() == rh.tobytes()
    assert np.array_equal(out["count"].cpu().numpy(), rc.astype(np.int64))
    assert out["distance"].shape == (n, k) and out["normal"].shape == (n, k, 3) and out["point"].shape == (n, k, 3)
    assert np.array_equal(out["distance"].cpu().numpy().view(np.uint32), rh["distance"].view(np.uint32))
    assert np.array_equal(out["normal"].cpu().numpy(), rh["normal"]) and np.array_equal(out["point"].cpu().numpy(), rh["point"])
    for f in ("body", "collider", "shape", "tag"):
        assert out[f].shape == (n, k) and np.array_equal(out[f].cpu().numpy(), rh[f].astype(np.int64)), f
    # defaults: +inf, nothing ignored -- every slot holds a collider
    out = w.closest_k(p[:16], 3, synchronize=True)
    assert (out["count"].cpu().numpy() == 3).all() and (out["shape"].cpu().numpy() != NONE).all()
    assert out["raw"].cpu().numpy().tobytes() == N.closest_k(rec, w.nbox, _queries(p[:16]), 3)[1].tobytes()
    w.close()


# ---- observers -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(OBSERVED))
def test_k_nearest_queries_between_nh_step_calls_change_nothing(name):
    scene = OBSERVED[name]()
    rng = np.random.default_rng(88)
    q = _queries(rng.uniform((-30, -12, -30), (30, 20, 30), size=(4096, 3)), max_distance=rng.choice([np.inf, 1.0], size=4096))
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    qt = _upload(a, q)
    ht = a.torch.empty((4096 * 8, 48), dtype=a.torch.uint8, device=a.dev)
    ct = a.torch.empty(4096, dtype=a.torch.int32, device=a.dev)

    def query():
        a.query_build()
        a.closest_k_records(qt, 8, counts=ct, hits=ht)

    done = 0
    for steps in [1, 2, 3, 5, 7, 4, 8] * 10:
        steps = min(steps, 300 - done)
        if steps <= 0:
            break
        query()
        a.step(steps)
        b.step(steps)
        done += steps
    query()
    assert done == 300
    _same_stepped_world(a, b, f"{name} nh_step")
    if name == "grid_tiles":
        assert a.counts()["still_steps"] > 0, a.counts()
    a.close(); b.close()
