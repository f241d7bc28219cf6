"""Overlap queries on the GPU (pytest -m gpu): nh_overlap (include/nudge_hip.h, "scene queries").

The oracle is a brute force over every collider on the host with the same predicates (nudge_amd/csrc/nh_query.h through
tests/hostoverlap_util.py).  The answer is defined without reference to the tree -- per query the colliders in ascending combined index, laid
out by the exclusive scan of the counts -- so offsets and records must equal the brute force byte for byte, and so must every byte of `hits`
behind the written prefix (a sentinel there stays the sentinel).  Queries are observers: worlds that answer them between every pair of entry
points must step exactly like worlds that do not."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostoverlap_util as O                 # noqa: E402
import list_util as LU                       # noqa: E402
from list_util import SENTINEL, gpu_list, same_lists, sentinel_hits      # noqa: E402
from query_util import FUSED, NONE, OBSERVED, SMALL, bounds as _bounds, unit_quats as _unit_quats, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu



def _queries(rng, n, rec, kind, scale=1.0):
    """`kind`: spheres / boxes anywhere around the scene; points (radius 0) on collider centres; a mixed batch with ignore_body and invalid
    queries.  `scale`: the size of the query shapes (about one collider's at 1)."""
    lo, hi = _bounds(rec)
    span = np.maximum(hi - lo, 1.0)
    live = np.nonzero(np.isfinite(rec["p"]).all(axis=1))[0]
    q = np.zeros(n, dtype=E.OVERLAP_QUERY)
    q["ignore_body"] = NONE
    q["rotation"] = (0.0, 0.0, 0.0, 1.0)
    near = rng.random(n) < 0.5                     # half of them on a collider, half anywhere
    on = rec["p"][rng.choice(live, size=n)].astype(np.float64) + rng.normal(scale=0.3 * scale, size=(n, 3))
    q["center"] = np.where(near[:, None], on, rng.uniform(lo - 0.1 * span, hi + 0.1 * span, size=(n, 3)))
    if kind == "sphere":
        q["shape"] = E.NH_SHAPE_SPHERE
        q["size"][:, 0] = rng.uniform(0.0, 2.0 * scale, size=n)
    elif kind == "box":
        q["shape"] = E.NH_SHAPE_BOX
        q["size"] = rng.uniform(0.0, 1.5 * scale, size=(n, 3))
        q["rotation"] = _unit_quats(rng, n)
    elif kind == "point":
        q["shape"] = E.NH_SHAPE_SPHERE
        q["center"] = rec["p"][rng.choice(live, size=n)]
    else:
        q["shape"] = rng.choice([E.NH_SHAPE_SPHERE, E.NH_SHAPE_BOX], size=n)
        q["size"] = rng.uniform(0.0, 1.5 * scale, size=(n, 3))
        q["rotation"] = _unit_quats(rng, n)
        ign = rng.random(n) < 0.3
        q["ignore_body"][ign] = rec["body"][rng.choice(live, size=int(ign.sum()))]
        bad = rng.choice(n, size=max(1, n // 64), replace=False)
        for j, b in enumerate(bad):
            k = j % 5
            if k == 0:
                q["shape"][b] = 7
            elif k == 1:
                q["center"][b, 1] = np.nan
            elif k == 2:
                q["size"][b, 0] = -0.5
            elif k == 3:
                q["size"][b, 2] = np.inf
            else:
                q["rotation"][b, 0] = np.nan
    return q


def _capsule_queries(rng, n, rec, scale=1.0):
    """Capsule queries around the scene: half on a collider, radii and half heights from 0, random rotations, some ignore_body and invalid ones."""
    q = _queries(rng, n, rec, "sphere", scale)
    q["shape"] = E.NH_SHAPE_CAPSULE
    q["size"][:, 0] = rng.uniform(0.0, 1.2 * scale, size=n)
    q["size"][:, 1] = rng.choice([0.0, 0.3, 1.0, 2.5], size=n) * scale
    q["size"][:, 2] = np.nan                                           # (not read)
    q["rotation"] = _unit_quats(rng, n)
    q["rotation"][(q["size"][:, 1] == 0.0) & (rng.random(n) < 0.5)] = np.nan     # (not read at half height 0)
    live = np.nonzero(np.isfinite(rec["p"]).all(axis=1))[0]
    ign = rng.random(n) < 0.2
    q["ignore_body"][ign] = rec["body"][rng.choice(live, size=int(ign.sum()))]
    bad = rng.choice(n, size=max(1, n // 64), replace=False)
    for j, b in enumerate(bad):
        k = j % 4
        if k == 0:
            q["size"][b, 1] = -0.5
        elif k == 1:
            q["size"][b, 1] = np.nan
        elif k == 2:
            q["size"][b, 1], q["rotation"][b, 2] = 1.0, np.inf
        else:
            q["center"][b, 0] = np.nan
    return q


def _gpu(w, queries, capacity):
    """(offsets, hits): one nh_overlap call with `hits` pre-filled with the sentinel (capacity records; None = count only)."""
    return gpu_list(w, "overlap_records", queries, capacity, E.OVERLAP_HIT)


def _same(w, rec, queries, what, capacity=None):
    """The count-only call, then a list call with `capacity` (None: exactly the total), against the brute force; returns the host offsets and the total."""
    return same_lists(w, "overlap_records", O.overlap, rec, queries, E.OVERLAP_HIT, what, capacity)


def _check_world(w, scene, rng, n, what):
    w.query_build()
    rec = O.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    totals = []
    for kind in ("sphere", "box", "point", "mixed"):
        _, total = _same(w, rec, _queries(rng, n, rec, kind), f"{what} / {kind}")
        totals.append(total)
    return totals


@pytest.mark.parametrize("name", sorted(SMALL))
def test_overlaps_equal_the_brute_force_before_and_after_stepping(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(200 + sorted(SMALL).index(name))
    w = E.World(scene, flags=FUSED)
    totals = _check_world(w, scene, rng, 8192, f"{name} initial")
    assert min(totals) > 1000, totals
    w.step(50)
    totals = _check_world(w, scene, rng, 8192, f"{name} after 50 steps")
    assert min(totals) > 1000, totals
    w.close()


def test_two_identical_calls_give_identical_bytes():
    scene = SMALL["grid_tiles"]()
    w = E.World(scene, flags=FUSED)
    w.step(20)
    w.query_build()
    rec = O.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    q = _queries(np.random.default_rng(11), 16384, rec, "mixed")
    ref_off, _, total = O.overlap(rec, w.nbox, q, capacity=0)
    a, b = _gpu(w, q, total), _gpu(w, q, total)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    w.close()


def test_a_single_collider():
    scene = S.pile(4, 0, seed=3)
    w = E.World(scene, flags=FUSED)
    w.set_counts(len(scene["body_transforms"]), 1, 0)          # the ground slab alone (body 0)
    rng = np.random.default_rng(1)
    _check_world(w, scene, rng, 4096, "one collider")
    rec = O.records(w.get_bodies()["transforms"], scene, 1, 0)
    q = _queries(rng, 64, rec, "point")
    off, hits = _gpu(w, q, 64)
    assert (np.diff(off.astype(np.int64)) == 1).all() and (hits["body"] == 0).all() and (hits["shape"] == E.NH_SHAPE_BOX).all()
    w.close()


def test_only_spheres_and_only_boxes():
    scene = S.pile(300, 300, seed=3)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    rng = np.random.default_rng(2)
    w.set_counts(nb, 0, 300)
    _check_world(w, scene, rng, 4096, "spheres only")
    w.set_counts(nb, 301, 0)
    _check_world(w, scene, rng, 4096, "boxes only")
    w.close()


def _coincident(n=4096):
    scene = S.pile(n, 0, seed=3)
    scene["body_transforms"]["position"][1:] = (0.25, 3.0, -0.5)        # every box at one position; the ground slab elsewhere
    return scene


def test_four_thousand_boxes_at_one_position():
    scene = _coincident()
    w = E.World(scene, flags=FUSED)
    rng = np.random.default_rng(3)
    _check_world(w, scene, rng, 2048, "4096 coincident boxes")
    w.close()


def test_a_scene_spanning_a_thousandth_and_ten_thousand_units():
    scene = S.pile(2000, 1000, seed=3)
    rng = np.random.default_rng(4)
    nb = len(scene["body_transforms"])
    small = rng.random(nb) < 0.5
    pos = np.where(small[:, None], rng.uniform(-0.05, 0.05, size=(nb, 3)), rng.uniform(-1e4, 1e4, size=(nb, 3))).astype(np.float32)
    scene["body_transforms"]["position"][1:] = pos[1:]
    bsmall = small[scene["box_transforms"]["body"][1:]]
    scene["box_data"]["size"][1:] = np.where(bsmall[:, None], np.float32(1e-3), np.float32(30.0))
    scene["sphere_data"]["radius"] = np.where(small[scene["sphere_transforms"]["body"]], np.float32(1e-3), np.float32(25.0))
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = O.records(w.get_bodies()["transforms"], scene)
    for kind in ("sphere", "box", "point", "mixed"):
        _same(w, rec, _queries(rng, 4096, rec, kind, scale=30.0), f"1e-3 .. 1e4, large / {kind}")
    tiny = rec[(rec["h"][:, 0] <= 1e-3)]
    for kind in ("sphere", "box", "point"):
        _same(w, rec, _queries(rng, 4096, tiny, kind, scale=1e-3), f"1e-3 .. 1e4, the small cluster / {kind}")
    w.close()


# ---- capacity -------------------------------------------------------------------------------------------------------------------------------
def test_capacity_writes_whole_segments_and_nothing_behind_them():
    scene = SMALL["pile"]()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = O.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    q = _queries(np.random.default_rng(12), 2048, rec, "mixed")
    ref_off, _, total = O.overlap(rec, w.nbox, q, capacity=0)
    nz = np.nonzero(np.diff(ref_off.astype(np.int64)) > 1)[0]
    boundary = int(ref_off[nz[len(nz) // 2]])                  # the start of a segment of at least two records
    caps = [total, total - 1, boundary, boundary + 1, 0]
    for cap in caps:
        _same(w, rec, q, f"capacity {cap} of {total}", capacity=cap)
    # capacity 0 with a non-null hits buffer: count only, the buffer untouched
    off, hits = _gpu(w, q, 0)
    assert off.tobytes() == ref_off.tobytes() and set(hits.tobytes()) == {SENTINEL}
    w.close()


def test_one_query_over_every_collider_of_a_4096_collider_world():
    scene = S.pile(4096, 0, seed=3)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    w.set_counts(nb, 4096, 0)
    w.query_build()
    rec = O.records(w.get_bodies()["transforms"], scene, 4096, 0)
    q = np.zeros(1, dtype=E.OVERLAP_QUERY)
    q["shape"], q["size"], q["rotation"], q["ignore_body"] = E.NH_SHAPE_SPHERE, (1e4, 0, 0), (0, 0, 0, 1), NONE
    _same(w, rec, q, "one segment of 4096")
    off, hits = _gpu(w, q, 4096)
    assert list(off) == [0, 4096] and np.array_equal(hits["collider"], np.arange(4096)) and (hits["shape"] == E.NH_SHAPE_BOX).all()
    r = w.overlap(np.zeros((1, 3)), radii=1e4, synchronize=True)
    assert int(r["written"]) == 4096 and np.array_equal(r["collider"].cpu().numpy(), np.arange(4096)) and (r["query"] == 0).all()
    w.close()


def test_a_total_of_two_to_the_thirty_second_writes_the_marker_and_no_record():
    scene = _coincident()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = O.records(w.get_bodies()["transforms"], scene)
    q = np.zeros(1 << 20, dtype=E.OVERLAP_QUERY)
    q["shape"], q["center"], q["rotation"], q["ignore_body"] = E.NH_SHAPE_SPHERE, (0.25, 3.0, -0.5), (0, 0, 0, 1), NONE
    one, _, total = O.overlap(rec, w.nbox, q[:1], capacity=0)
    assert total == 4096                                   # so 2^20 of them make exactly 2^32: the 32-bit scan wraps to 0
    cnt, _ = _gpu(w, q, None)
    assert cnt[-1] == NONE
    off, hits = _gpu(w, q, 1 << 16)
    assert off[-1] == NONE and set(hits.tobytes()) == {SENTINEL}
    # 2^20 - 1 queries: 2^32 - 4096 records, no wrap, the prefix rule applies
    cnt, _ = _gpu(w, q[1:], None)
    assert int(cnt[-1]) == (1 << 32) - 4096 and (np.diff(cnt.astype(np.int64)) == 4096).all()
    r = w.overlap(q["center"], radii=0.0, capacity=1000, synchronize=True)
    assert int(r["offsets"][-1]) == NONE and int(r["written"]) == 0
    w.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_abi_edge_cases():
    import torch
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    L = w.L
    rec = O.records(w.get_bodies()["transforms"], scene)
    q = _queries(np.random.default_rng(5), 1024, rec, "mixed")
    qt = _upload(w, q)
    buf = torch.zeros(4 * 1032, dtype=torch.int32, device=w.dev)
    ot = buf[:1025]
    ht = torch.zeros((4096, 16), dtype=torch.uint8, device=w.dev)
    qp, op, hp = C.c_void_p(qt.data_ptr()), C.c_void_p(ot.data_ptr()), C.c_void_p(ht.data_ptr())
    assert L.nh_overlap(w.ctx, qp, 1024, op, hp, 4096, 0) == 1                 # before any build: NH_ERR_INVALID
    assert L.nh_overlap(None, qp, 1024, op, hp, 4096, 0) == 1
    w.query_build()
    assert L.nh_overlap(w.ctx, qp, 1024, op, hp, 4096, 1) == 1                 # flags
    assert L.nh_overlap(w.ctx, None, 1024, op, hp, 4096, 0) == 1               # null / unaligned queries
    assert L.nh_overlap(w.ctx, C.c_void_p(qt.data_ptr() + 4), 1023, op, hp, 4096, 0) == 1
    assert L.nh_overlap(w.ctx, qp, 1024, None, hp, 4096, 0) == 1               # null / unaligned offsets
    assert L.nh_overlap(w.ctx, qp, 1024, C.c_void_p(ot.data_ptr() + 2), hp, 4096, 0) == 1
    assert L.nh_overlap(w.ctx, qp, 1024, op, None, 4096, 0) == 1               # null hits with a capacity, unaligned hits
    assert L.nh_overlap(w.ctx, qp, 1024, op, C.c_void_p(ht.data_ptr() + 8), 4095, 0) == 1
    assert L.nh_overlap(w.ctx, qp, 1 << 30, op, hp, 4096, 0) == 1              # count >= 2^30: refused on the host, nothing launched
    assert L.nh_overlap(w.ctx, qp, 0xFFFFFFFF, op, hp, 4096, 0) == 1
    assert L.nh_overlap(w.ctx, qp, 0, op, hp, 4096, 0) == 0                    # count 0: a no-op
    assert L.nh_overlap(w.ctx, None, 0, None, None, 0, 0) == 0
    w.torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0 and int(ht.sum()) == 0                    # nothing was written
    # offsets need 4-byte alignment only
    ot4 = buf[1:1026]
    assert L.nh_overlap(w.ctx, qp, 1024, C.c_void_p(ot4.data_ptr()), hp, 4096, 0) == 0
    ref_off, ref_hits, total = O.overlap(rec, w.nbox, q, capacity=4096, hits=sentinel_hits(4096, E.OVERLAP_HIT))
    assert total <= 4096
    assert ot4.cpu().numpy().view(np.uint32).tobytes() == ref_off.tobytes()
    got = np.frombuffer(ht.cpu().numpy().tobytes(), dtype=E.OVERLAP_HIT)
    assert got[:total].tobytes() == ref_hits[:total].tobytes() and not got[total:].view(np.uint8).any()
    w.close()


# ---- observers -----------------------------------------------------------------------------------------------------------------------------
def _query(w, qt, ot, ht):
    w.query_build()
    w.overlap_records(qt, offsets=ot)
    w.overlap_records(qt, offsets=ot, hits=ht, capacity=ht.shape[0])


def _observer_batch(a, scene):
    import torch
    a.query_build()
    rec = O.records(a.get_bodies()["transforms"], scene, a.nbox, a.nsph)
    q = _queries(np.random.default_rng(7), 4096, rec, "mixed")
    qt = _upload(a, q)
    ot = torch.empty(4097, dtype=torch.int32, device=a.dev)
    ht = torch.empty((8192, 16), dtype=torch.uint8, device=a.dev)
    return qt, ot, ht


@pytest.mark.parametrize("name", sorted(OBSERVED))
def test_overlaps_between_nh_step_calls_change_nothing(name):
    LU.queries_between_nh_step_calls_change_nothing(OBSERVED[name], _observer_batch, _query, name, still=name == "grid_tiles")


@pytest.mark.parametrize("name", sorted(OBSERVED))
def test_overlaps_between_every_call_of_the_fused_step_change_nothing(name):
    LU.queries_between_every_call_of_the_fused_step_change_nothing(OBSERVED[name], _observer_batch, _query, name, still=name == "grid_tiles")


# ---- at size -------------------------------------------------------------------------------------------------------------------------------
def test_a_million_sphere_queries_on_the_landed_config_2_world():
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED, max_contacts=6 * nb)
    w.step(70)
    assert w.counts()["error"] == 0
    w.query_build()
    rec = O.records(w.get_bodies()["transforms"], scene)
    assert len(rec) == 1004524
    rng = np.random.default_rng(9)
    n = 1 << 20
    dyn = np.nonzero(rec["body"] != 0)[0]
    target = rng.choice(dyn, size=n)
    q = np.zeros(n, dtype=E.OVERLAP_QUERY)
    q["shape"], q["rotation"], q["ignore_body"] = E.NH_SHAPE_SPHERE, (0, 0, 0, 1), NONE
    q["center"] = rec["p"][target]
    point = np.arange(n) < n // 2                  # half zero-radius queries on a collider's centre, half about one box's size around it
    q["size"][~point, 0] = rng.uniform(0.25, 1.0, size=int((~point).sum()))
    q["center"][~point] += rng.normal(scale=0.5, size=(int((~point).sum()), 3)).astype(np.float32)
    cnt, _ = _gpu(w, q, None)
    total = int(cnt[-1])
    assert total < NONE and total >= n // 2
    off, hits = _gpu(w, q, total)
    assert off.tobytes() == cnt.tobytes()
    # full batch: every zero-radius query lists the collider it is centred on
    qi = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    comb = hits["collider"].astype(np.int64) + np.where(hits["shape"] == E.NH_SHAPE_BOX, 0, w.nbox)
    own = comb == target[qi]
    found = np.zeros(n, dtype=bool)
    found[qi[own]] = True
    assert found[point].all(), f"{int((~found[point]).sum())} zero-radius queries miss their own collider"
    # 1024 queries spread over the batch, byte for byte against the brute force over all 1,004,524 colliders
    pick = np.linspace(0, n - 1, 1024).astype(np.int64)
    ref_off, ref_hits, ref_total = O.overlap(rec, w.nbox, q[pick])
    seg = np.concatenate([hits[off[i]:off[i + 1]] for i in pick])
    assert np.array_equal(np.diff(ref_off.astype(np.int64)), np.diff(off.astype(np.int64))[pick])
    assert seg.tobytes() == ref_hits[:ref_total].tobytes()
    w.close()


def test_boxes_a_hair_beside_resting_boxes():
    """Axis-aligned query boxes next to nearly axis-aligned resting boxes, a hair apart or touching: the near-parallel edges of the box-box test."""
    scene = SMALL["stacks"]()
    w = E.World(scene, flags=FUSED)
    w.step(120)
    w.query_build()
    rec = O.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    rng = np.random.default_rng(13)
    boxes = np.nonzero((rec["body"][:w.nbox] != 0))[0]
    n = 8192
    pick = rng.choice(boxes, size=n)
    axis = rng.integers(0, 3, size=n)
    sign = rng.choice([-1.0, 1.0], size=n)
    gap = 10.0 ** rng.uniform(-8, -2, size=n) * rng.choice([-1.0, 0.0, 1.0], size=n)
    q = np.zeros(n, dtype=E.OVERLAP_QUERY)
    q["shape"], q["ignore_body"] = E.NH_SHAPE_BOX, NONE
    q["rotation"] = (0.0, 0.0, 0.0, 1.0)
    h = rec["h"][pick].astype(np.float64)
    q["size"] = h
    c = rec["p"][pick].astype(np.float64)
    c[np.arange(n), axis] += sign * (2.0 * h[np.arange(n), axis] + gap)
    q["center"] = c
    _same(w, rec, q, "a hair beside resting boxes")
    w.close()
