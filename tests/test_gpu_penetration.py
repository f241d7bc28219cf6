"""Penetration queries on the GPU (pytest -m gpu): nh_penetration (include/nudge_hip.h, "scene queries").

The oracle is a brute force over every collider on the host with the same arithmetic (nudge_amd/csrc/nh_query.h through tests/hostpen_util.py)
and the header's exact rules, so offsets and every byte of every 32-byte record must equal it, and so must every byte of `hits` behind the
written prefix (a sentinel there stays the sentinel).  On the GPU itself the call is nh_overlap with a richer record: the same offsets, and
nh_overlap's record in the last 16 bytes of each.  Queries are observers like the other queries."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostpen_util as H                     # noqa: E402
import hostquery_util as Q                   # noqa: E402
import list_util as LU                       # noqa: E402
from list_util import SENTINEL, gpu_list, same_lists      # noqa: E402
from query_util import FUSED, NONE, OBSERVED, SMALL, bounds as _bounds, unit_quats as _unit_quats, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ("sphere", "box", "capsule", "mixed")


def _queries(rng, n, rec, kind, scale=1.0):
    """Spheres, oriented boxes or capsules, or a mixed batch with ignore_body, capsules of half height 0 and invalid queries: half of them on a
    collider (inside piles: deep records), half anywhere around the scene."""
    lo, hi = _bounds(rec)
    span = np.maximum(hi - lo, 1.0)
    live = np.nonzero(np.isfinite(rec["p"]).all(axis=1))[0]
    q = np.zeros(n, dtype=E.OVERLAP_QUERY)
    q["ignore_body"] = NONE
    near = rng.random(n) < 0.5
    on = rec["p"][rng.choice(live, size=n)].astype(np.float64) + rng.normal(scale=0.3 * scale, size=(n, 3))
    q["center"] = np.where(near[:, None], on, rng.uniform(lo - 0.1 * span, hi + 0.1 * span, size=(n, 3)))
    q["rotation"] = _unit_quats(rng, n)
    q["rotation"][::4] = (0.0, 0.0, 0.0, 1.0)                      # (axis-aligned against axis-aligned colliders: parallel edges)
    q["size"] = rng.uniform(0.0, 1.5 * scale, size=(n, 3))
    shape = dict(sphere=E.NH_SHAPE_SPHERE, box=E.NH_SHAPE_BOX, capsule=E.NH_SHAPE_CAPSULE)
    if kind in shape:
        q["shape"] = shape[kind]
        return q
    q["shape"] = rng.choice([E.NH_SHAPE_SPHERE, E.NH_SHAPE_BOX, E.NH_SHAPE_CAPSULE], size=n)
    flat = (q["shape"] == E.NH_SHAPE_CAPSULE) & (rng.random(n) < 0.25)
    q["size"][flat, 1] = 0.0
    q["rotation"][flat] = np.nan                                   # (not read)
    ign = rng.random(n) < 0.3
    q["ignore_body"][ign] = rec["body"][rng.choice(live, size=int(ign.sum()))]
    bad = rng.choice(np.nonzero(~flat)[0], size=max(1, n // 64), replace=False)
    for j, b in enumerate(bad):
        k = j % 5
        if k == 0:
            q["shape"][b] = 7
        elif k == 1:
            q["center"][b, 1] = np.nan
        elif k == 2:
            q["size"][b, 0] = -0.5
        elif k == 3:
            q["size"][b, 1] = np.inf
            q["shape"][b] = E.NH_SHAPE_BOX
        else:
            q["rotation"][b, 0] = np.nan
            q["shape"][b] = E.NH_SHAPE_BOX
    return q


def _gpu(w, queries, capacity, call="penetration"):
    """(offsets, hits): one call with `hits` pre-filled with the sentinel (capacity records; None = count only)."""
    return gpu_list(w, call + "_records", queries, capacity, E.PENETRATION_HIT if call == "penetration" else E.OVERLAP_HIT)


def _same(w, rec, queries, what, capacity=None):
    """The count-only call, then a list call with `capacity` (None: exactly the total), against the brute force -- and against nh_overlap on the
    GPU itself; returns the host offsets and the total."""
    off, hits, total = same_lists(w, "penetration_records", H.penetration, rec, queries, E.PENETRATION_HIT, what, capacity, with_hits=True)
    ooff, ohits = _gpu(w, queries, (0 if total >= NONE else total) if capacity is None else capacity, call="overlap")
    assert ooff.tobytes() == off.tobytes(), f"{what}: offsets differ from nh_overlap's"
    assert hits.view(np.uint8).reshape(-1, 32)[:, 16:].tobytes() == ohits.view(np.uint8).reshape(-1, 16).tobytes(), f"{what}: records differ from nh_overlap's"
    return off, total


def _check_world(w, scene, rng, n, what, build=True):
    if build:
        w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    several, none = [], []
    for kind in KINDS:
        off, total = _same(w, rec, _queries(rng, n, rec, kind), f"{what} / {kind}")
        counts = np.diff(off.astype(np.int64))
        several.append(float((counts > 1).mean())); none.append(float((counts == 0).mean()))
    return several, none


@pytest.mark.parametrize("name", sorted(SMALL))
def test_penetrations_equal_the_brute_force_before_and_after_stepping(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(700 + sorted(SMALL).index(name))
    w = E.World(scene, flags=FUSED)
    for when in ("initial", "after 50 steps"):
        several, none = _check_world(w, scene, rng, 8192, f"{name} {when}")
        assert np.mean(several) > 0.05 and np.mean(none) > 0.005, (name, when, several, none)          # segments of several records, and empty ones
        w.step(50)
    w.close()


def test_count_only_and_a_capacity_in_the_middle_of_the_list():
    scene = SMALL["pile"]()
    w = E.World(scene, flags=FUSED)
    w.step(30)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    rng = np.random.default_rng(71)
    q = _queries(rng, 4096, rec, "mixed", scale=1.5)
    full_off, full, total = H.penetration(rec, w.nbox, q)
    assert total > 1024
    # count only: offsets alone
    cnt, none = _gpu(w, q, None)
    assert none is None and cnt.tobytes() == full_off.tobytes()
    for cap in (1, total // 3, int(full_off[len(q) // 2]), int(full_off[len(q) // 2]) + 1, total - 1, total, total + 100):
        off, hits = _gpu(w, q, cap)
        written = int(full_off[np.searchsorted(full_off, cap, side="right") - 1])
        assert off.tobytes() == full_off.tobytes(), cap
        assert hits[:written].tobytes() == full[:written].tobytes(), (cap, LU.differ(hits[:written], full[:written]))
        assert (hits[written:].view(np.uint8) == SENTINEL).all(), cap          # every byte behind the written prefix is untouched
        _same(w, rec, q, f"capacity {cap}", capacity=cap)
    w.close()


def test_abi_edge_cases():
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    L = w.L
    import torch
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    q = _queries(np.random.default_rng(72), 1024, rec, "mixed")
    t = _upload(w, q)
    ot = torch.zeros(1026, dtype=torch.int32, device=w.dev)
    hits = torch.zeros((4096, 32), dtype=torch.uint8, device=w.dev)
    qp, op, hp = t.data_ptr(), ot.data_ptr(), hits.data_ptr()
    call = lambda *a: L.nh_penetration(w.ctx, *[C.c_void_p(x) if i in (0, 2, 3) else x for i, x in enumerate(a)])          # noqa: E731
    assert call(qp, 1024, op, hp, 4096, 0) == 1                                # before any build: NH_ERR_INVALID
    assert L.nh_penetration(None, C.c_void_p(qp), 1024, C.c_void_p(op), C.c_void_p(hp), 4096, 0) == 1
    w.query_build()
    assert call(qp, 0, op, hp, 4096, 0) == 0                                   # count 0: a no-op
    assert call(qp, 1024, op, hp, 4096, 1) == 1                                # flags other than 0
    assert call(None, 1024, op, hp, 4096, 0) == 1                              # null queries / offsets, null hits with a capacity
    assert call(qp, 1024, None, hp, 4096, 0) == 1
    assert call(qp, 1024, op, None, 4096, 0) == 1
    assert call(qp + 4, 1023, op, hp, 4096, 0) == 1                            # misaligned queries / offsets / hits
    assert call(qp, 1024, op + 2, hp, 4096, 0) == 1
    assert call(qp, 1024, op, hp + 8, 4095, 0) == 1
    assert call(qp, 1 << 30, op, hp, 4096, 0) == 1                             # count >= 2^30
    torch.cuda.synchronize()
    assert int(hits.sum()) == 0 and int(ot.abs().sum()) == 0                   # nothing was written
    assert call(qp, 1024, op, hp, 4096, 0) == 0
    assert call(qp, 1024, op, None, 0, 0) == 0                                 # count only
    torch.cuda.synchronize()
    assert int(ot[1025]) == 0                                                  # nothing behind offsets[count]
    w.close()


def test_the_same_bytes_after_a_refit_as_after_a_build():
    scene = SMALL["pile"]()
    rng = np.random.default_rng(73)
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    a.query_build()
    for k in (10, 40):
        a.step(k); b.step(k)
        a.query_refit()
        b.query_build()
        rec = Q.records(a.get_bodies()["transforms"], scene, a.nbox, a.nsph)
        q = _queries(rng, 4096, rec, "mixed")
        _, total = _same(a, rec, q, f"refit after {k} steps")
        off_a, hits_a = _gpu(a, q, total)
        off_b, hits_b = _gpu(b, q, total)
        assert total > 1024 and off_a.tobytes() == off_b.tobytes() and hits_a.tobytes() == hits_b.tobytes()
    a.close(); b.close()


def test_degenerate_worlds():
    rng = np.random.default_rng(74)
    scene = S.pile(4, 0, seed=3)
    w = E.World(scene, flags=FUSED)
    w.set_counts(len(scene["body_transforms"]), 0, 0)          # no collider at all: every count is 0
    w.query_build()
    q = np.zeros(1024, dtype=E.OVERLAP_QUERY)
    q["shape"], q["rotation"], q["ignore_body"] = rng.choice([0, 1, 2], size=1024), (0, 0, 0, 1), NONE
    q["center"], q["size"] = rng.uniform(-5, 5, size=(1024, 3)), rng.uniform(0, 5, size=(1024, 3))
    off, hits = _gpu(w, q, 16)
    assert not off.any() and (hits.view(np.uint8) == SENTINEL).all()
    w.set_counts(len(scene["body_transforms"]), 1, 0)          # the ground slab alone (body 0)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    top = rec["p"][0, 1] + rec["h"][0, 1]
    q["center"][:, 1] = rng.uniform(top - 2, top + 8, size=1024)               # in the slab, on it, above it
    q["center"][:, [0, 2]] = rec["p"][0, [0, 2]] + rng.uniform(-3, 3, size=(1024, 2))
    _, total = _same(w, rec, q, "one collider")
    assert 100 < total < 1024
    w.close()

    scene = S.pile(4096, 0, seed=3)
    scene["body_transforms"]["position"][1:] = (0.25, 3.0, -0.5)        # every Morton key equal but the ground's
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    q = q[:64]
    q["center"] = np.float32([0.25, 3.0, -0.5]) + rng.normal(scale=0.5, size=(64, 3))
    _, total = _same(w, rec, q, "4096 coincident boxes")
    assert total > 32 * 4096
    w.close()


def test_the_python_wrappers_write_the_records_they_describe():
    scene = SMALL["grid_tiles"]()
    w = E.World(scene, flags=FUSED)
    w.step(20)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    rng = np.random.default_rng(75)
    for kind in ("sphere", "box", "capsule"):
        q = _queries(rng, 2048, rec, kind)
        q["ignore_body"] = rng.integers(0, 40, size=2048)
        kw = dict(radii=q["size"][:, 0]) if kind != "box" else dict(half_extents=q["size"])
        if kind == "capsule":
            kw["half_heights"] = q["size"][:, 1]
        if kind != "sphere":
            kw["rotations"] = q["rotation"]
        ref_off, ref, total = H.penetration(rec, w.nbox, q)
        for capacity in (None, total // 2):
            out = w.penetration(q["center"], ignore_body=q["ignore_body"], capacity=capacity, synchronize=True, **kw)
            written = int(out["written"])
            assert written == (total if capacity is None else int(ref_off[np.searchsorted(ref_off, capacity, side="right") - 1]))
            assert np.array_equal(out["offsets"].cpu().numpy(), ref_off.astype(np.int64))
            raw = np.frombuffer(out["raw"].cpu().numpy().tobytes(), dtype=E.PENETRATION_HIT)
            assert raw[:written].tobytes() == ref[:written].tobytes(), (kind, capacity)
            assert np.array_equal(out["normal"].cpu().numpy()[:written], ref["normal"][:written])
            assert np.array_equal(out["depth"].cpu().numpy()[:written].view(np.uint32), ref["depth"][:written].view(np.uint32))
            for k in ("body", "collider", "shape", "tag"):
                assert np.array_equal(out[k].cpu().numpy()[:written], ref[k][:written].astype(np.int64)), k
            assert np.array_equal(out["query"].cpu().numpy()[:written], np.repeat(np.arange(2048), np.diff(ref_off.astype(np.int64)))[:written])
        assert total > 512
    w.close()


# ---- observers -----------------------------------------------------------------------------------------------------------------------------
def _query(w, queries_t, offsets_t, hits_t, capacity):
    w.query_build()
    w.penetration_records(queries_t, offsets=offsets_t, hits=hits_t, capacity=capacity)


@pytest.mark.parametrize("name", sorted(OBSERVED))
def test_penetration_queries_between_calls_change_nothing(name):
    rng = np.random.default_rng(76)
    n, cap = 4096, 1 << 16
    q = np.zeros(n, dtype=E.OVERLAP_QUERY)
    q["shape"], q["ignore_body"] = rng.choice([0, 1, 2], size=n), NONE
    q["center"] = rng.uniform((-30, -12, -30), (30, 20, 30), size=(n, 3))
    q["rotation"], q["size"] = _unit_quats(rng, n), rng.uniform(0.1, 3.0, size=(n, 3))

    def buffers(w, scene):
        return _upload(w, q), w.torch.empty(n + 1, dtype=w.torch.int32, device=w.dev), w.torch.empty((cap, 32), dtype=w.torch.uint8, device=w.dev), cap

    still = name == "grid_tiles"
    _, ot, _, _ = LU.queries_between_nh_step_calls_change_nothing(OBSERVED[name], buffers, _query, name, still=still)
    assert 0 < (int(ot[n]) & NONE) != NONE                                     # the queries did find something
    LU.queries_between_every_call_of_the_fused_step_change_nothing(OBSERVED[name], buffers, _query, name, still=still)
