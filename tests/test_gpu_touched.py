"""nh_move_touched, nh_boxmove_touched, nh_walk_touched and nh_boxwalk_touched on the GPU (pytest -m gpu): the movers' results and, beside them, the list
of everything each mover touched (include/nudge_hip.h, "nh_move_touched").

The oracle is the host's brute force (tests/hostoracle/hosttouch.cpp through tests/hosttouch_util.py): the loops the kernels run around a cast over every
collider, so results, counts and the written touches must equal it byte for byte.  Every GPU call here goes through `_touched`, which fills the arrays and
one record behind them with SENTINEL first: the slots at or behind counts[i] and everything behind the arrays must still hold it.  The identities T1 - T5
are tested against the GPU's own plain movers and casts."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostquery_util as Q                   # noqa: E402
import hosttouch_util as HT                  # noqa: E402
import touched_batches as TB                 # noqa: E402
import walk_batches as WB                    # noqa: E402
import boxwalk_batches as BWB                # noqa: E402
import mover_util as MU                      # noqa: E402
from mover_util import FUSED, NONE, SENTINEL, records as _records, same as _same, terrain_world as _terrain_world      # noqa: E402
from query_util import OBSERVED, SMALL, same_stepped_world as _same_stepped_world, unit_quats, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = sorted(TB.SHAPES)
# per (shape, kind): World's method prefix, the result record, the most touches
CALL = {("capsule", "move"): ("move", E.MOVE_RESULT, HT.MOVE_K), ("box", "move"): ("boxmove", E.MOVE_RESULT, HT.MOVE_K),
        ("capsule", "walk"): ("walk", E.WALK_RESULT, HT.WALK_K), ("box", "walk"): ("boxwalk", E.WALK_RESULT, HT.WALK_K)}


def _touched(w, shape, kind, records, k=None):
    """World.<call>_touched_records on the numpy records: (results, counts, touches ((n, k) E.TOUCH)) back on the host.  The arrays and one record behind
    each are SENTINEL before the call; what the call may not write must still be."""
    import torch
    name, result, k_max = CALL[shape, kind]
    k = k or k_max
    n, size = len(records), result.itemsize
    r = torch.full((n + 1, size), SENTINEL, dtype=torch.uint8, device=w.dev)
    c = torch.full((n + 1,), SENTINEL * 0x01010101 - (1 << 32), dtype=torch.int32, device=w.dev)
    t = torch.full((n + 1, k, 64), SENTINEL, dtype=torch.uint8, device=w.dev)
    getattr(w, name + "_touched_records")(_upload(w, records), k, results=r, counts=c, touches=t)
    torch.cuda.synchronize()
    r, c, t = r.cpu().numpy(), c.cpu().numpy().view(np.uint32), t.cpu().numpy()
    assert (r[n:] == SENTINEL).all() and c[n] == SENTINEL * 0x01010101 and (t[n:] == SENTINEL).all(), f"{name}_touched wrote behind its arrays"
    counts = c[:n].copy()
    assert (counts <= k_max).all()
    assert (t[:n][~HT.written(counts, k)] == SENTINEL).all(), f"{name}_touched wrote a slot at or behind its record's count"
    return np.frombuffer(r[:n].tobytes(), dtype=result).copy(), counts, np.frombuffer(t[:n].tobytes(), dtype=E.TOUCH).reshape(n, k).copy()


def _plain(w, shape, kind, records):
    return getattr(MU, CALL[shape, kind][0])(w, records)


def _cast(w, shape, casts):
    return (MU.boxcast if shape == "box" else MU.capsulecast)(w, casts)


def _oracle(shape, kind):
    return getattr(TB.SHAPES[shape], kind)


def _check(w, shape, kind, rec, records, what, **masked):
    """The call at k = the maximum against the brute force; returns the GPU's (results, counts, touches)."""
    ref, ref_counts, ref_touches = _oracle(shape, kind)(rec, w.nbox, records, **masked)
    got, counts, touches = _touched(w, shape, kind, records)
    _same(got, ref, what)
    HT.same_touches(touches, counts, ref_touches, ref_counts, what)
    return got, counts, touches


def _world_walks(shape, rng, rec, nbox, n):
    return (BWB if shape == "box" else WB).world_walks(rng, rec, nbox, n)


# ---- against the brute force ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SMALL))
@pytest.mark.parametrize("shape", SHAPES)
def test_moves_and_their_touches_equal_the_brute_force_before_and_after_stepping(shape, name):
    scene = SMALL[name]()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    m = TB.world_moves(shape, name, rec, w.nbox)
    got, counts, touches = _check(w, shape, "move", rec, m, f"{shape} {name} initial")
    assert (counts >= 1).mean() >= 0.25 and (counts >= 2).mean() >= 0.02, np.bincount(counts).tolist()
    HT.check_move_identities(got, counts, touches, f"{shape} {name} initial")
    w.step(50)
    # the refit of the tree built before the bodies moved, then a new build: the same bytes
    w.query_refit()
    rec = _records(w, scene)
    m = TB.world_moves(shape, name, rec, w.nbox, seed=20)
    got, counts, touches = _check(w, shape, "move", rec, m, f"{shape} {name} after 50 steps, refit")
    assert (counts >= 1).mean() >= 0.25 and (counts >= 2).mean() >= 0.02, np.bincount(counts).tolist()
    HT.check_move_identities(got, counts, touches, f"{shape} {name} refit")
    w.query_build()
    again, counts2, touches2 = _touched(w, shape, "move", m)
    _same(again, got, f"{shape} {name} after 50 steps, built")
    HT.same_touches(touches2, counts2, touches, counts, f"{shape} {name} after 50 steps, built")
    w.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_terrain_walks_and_their_touches_equal_the_brute_force(shape):
    w, scene, rec = _terrain_world()
    walks = TB.terrain_walks(shape)
    got, counts, touches = _check(w, shape, "walk", rec, walks, f"{shape} terrain")
    HT.check_walk_identities(got, counts, touches, f"{shape} terrain")
    assert (TB.phases(counts, touches) >= 3).mean() >= 0.05
    # T1 against the GPU's own plain call; T2 against its own cast, all touches in one call; T5
    _same(got, _plain(w, shape, "walk", walks), "T1")
    casts, _, hits = TB.SHAPES[shape].touch_casts(walks, counts, touches)
    assert len(casts) == counts.sum() and _cast(w, shape, casts).tobytes() == hits.tobytes()
    for k in (1, 3):
        g, c, t = _touched(w, shape, "walk", walks, k)
        _same(g, got, f"T5 k = {k}")
        HT.same_touches(t, c, touches, counts, f"T5 k = {k}")
    assert (counts > 3).sum() >= 10
    # after stepping (the one dynamic box falls far above) and a refit: the same bytes
    w.step(20)
    w.query_refit()
    _check(w, shape, "walk", _records(w, scene), walks, f"{shape} terrain, refit")
    w.close()


@pytest.mark.parametrize("name", ["grid_tiles", "stacks"])
@pytest.mark.parametrize("shape", SHAPES)
def test_world_walks_and_their_touches_equal_the_brute_force(shape, name):
    scene = SMALL[name]()
    w = E.World(scene, flags=FUSED)
    w.step(50)
    w.query_build()
    rec = _records(w, scene)
    walks = _world_walks(shape, np.random.default_rng(1100 + SHAPES.index(shape)), rec, w.nbox, 2048)
    got, counts, touches = _check(w, shape, "walk", rec, walks, f"{shape} {name}")
    HT.check_walk_identities(got, counts, touches, f"{shape} {name}")
    assert (counts >= 1).mean() >= 0.25
    w.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_move_identities_against_the_gpus_own_calls(shape):
    """T1 with the filter off and under per-query masks, T2 against the GPU's own cast, T5."""
    scene = SMALL["grid_tiles"]()
    w = E.World(scene, flags=FUSED)
    w.step(30)
    w.query_build()
    rec = _records(w, scene)
    m = TB.world_moves(shape, "grid_tiles", rec, w.nbox, seed=40)
    got, counts, touches = _touched(w, shape, "move", m)
    _same(got, _plain(w, shape, "move", m), "T1, filter off")
    HT.check_move_identities(got, counts, touches, "T3")
    casts, _, hits = TB.SHAPES[shape].touch_casts(m, counts, touches)
    assert len(casts) == counts.sum() >= 1024 and _cast(w, shape, casts).tobytes() == hits.tobytes()
    for k in (1, 3):
        g, c, t = _touched(w, shape, "move", m, k)
        _same(g, got, f"T5 k = {k}")
        HT.same_touches(t, c, touches, counts, f"T5 k = {k}")
    assert (counts > 1).mean() >= 0.02
    # per-query masks over two layers: T1, and T2 with each touch's cast under its record's mask
    words = np.where(np.arange(len(rec)) % 3 == 0, 1, 2).astype(np.uint32)
    w.query_set_layers(words[:w.nbox], words[w.nbox:])
    masks = np.where(np.arange(len(m)) % 2 == 0, 2, 3).astype(np.uint32)
    w.query_filter(_upload(w, masks).view(w.torch.int32))
    fg, fc, ft = _check(w, shape, "move", rec, m, "per-query masks", words=words, masks=masks)
    _same(fg, _plain(w, shape, "move", m), "T1, per-query masks")
    casts, owner, hits = TB.SHAPES[shape].touch_casts(m, fc, ft)
    w.query_filter(_upload(w, masks[owner]).view(w.torch.int32))
    assert _cast(w, shape, casts).tobytes() == hits.tobytes()
    h = ft["hit"][HT.written(fc, HT.MOVE_K)]                               # every touched collider is one its record's mask sees
    assert len(h) > 500 and (words[np.where(h["shape"] == E.NH_SHAPE_BOX, 0, w.nbox) + h["collider"]] & masks[owner] != 0).all()
    w.query_filter(None)
    w.close()


# ---- layer masks ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["move", "walk"])
@pytest.mark.parametrize("shape", SHAPES)
def test_touches_under_layer_masks_equal_the_brute_force_over_the_masked_world(shape, kind):
    scene = SMALL["pile"]()
    w = E.World(scene, flags=FUSED)
    w.step(40)
    w.query_build()
    rec = _records(w, scene)
    words = np.full(len(rec), 2, dtype=np.uint32)
    words[0] = 1                                                           # the ground slab (box 0, body 0) alone in layer 1
    w.query_set_layers(words[:w.nbox], words[w.nbox:])
    rng = np.random.default_rng(1120)
    n = 2048
    T = TB.SHAPES[shape]
    # shapes that drop onto the slab, away from the pile (top face at y = -10), beside a batch around the pile
    o = np.stack([rng.uniform(20, 300, n) * rng.choice([-1.0, 1.0], n), rng.uniform(-9.0, -7.0, n), rng.uniform(20, 300, n) * rng.choice([-1.0, 1.0], n)], axis=1)
    d = np.stack([rng.uniform(-3, 3, n), rng.uniform(-5.0, -3.5, n), rng.uniform(-3, 3, n)], axis=1)
    size = ((0.3, 0.4, 0.3),) if shape == "box" else (0.4, rng.choice([0.0, 0.5], n))
    if kind == "move":
        above = T.mover.moves(o, d, *size, rotations=unit_quats(rng, n))
        recs = np.concatenate([above, TB.world_moves(shape, "pile", rec, w.nbox, n, seed=60)])
    else:
        above = T.mover.walks(o, d, *size, snap_distance=0.3, step_height=0.4)
        recs = np.concatenate([above, _world_walks(shape, rng, rec, w.nbox, n)])
    off, off_counts, off_touches = _check(w, shape, kind, rec, recs, "filter off")
    assert (off_counts[:n] >= 1).all() and (off_touches["hit"]["collider"][:n, 0] == 0).all()
    for mask in (3, 2, 1, 0):
        w.query_filter(mask)
        got, counts, touches = _check(w, shape, kind, rec, recs, f"uniform mask {mask}", words=words, mask=mask)
        if mask == 3:
            _same(got, off, "mask 3 beside filter off")
            HT.same_touches(touches, counts, off_touches, off_counts, "mask 3 beside filter off")
        if mask == 2:                                                      # the slab is hidden: those above it touch nothing
            assert (counts[:n] == 0).all()
        if mask == 0:
            assert (counts == 0).all()
    masks = np.where(np.arange(len(recs)) % 2 == 0, 2, 3).astype(np.uint32)
    w.query_filter(_upload(w, masks).view(w.torch.int32))
    got, counts, touches = _check(w, shape, kind, rec, recs, "per-query masks", words=words, masks=masks)
    assert (counts[:n][0::2] == 0).all() and (counts[:n][1::2] >= 1).all()
    w.query_filter(None)
    again, counts, touches = _touched(w, shape, kind, recs)
    _same(again, off, "filter off again")
    HT.same_touches(touches, counts, off_touches, off_counts, "filter off again")
    w.close()


# ---- degenerate worlds ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_degenerate_worlds(shape):
    T = TB.SHAPES[shape]
    scene = S.pile(4, 0, seed=3)
    w = E.World(scene, flags=FUSED)
    w.set_counts(len(scene["body_transforms"]), 1, 0)          # the ground slab alone (body 0)
    w.query_build()
    rng = np.random.default_rng(1130)
    rec = _records(w, scene)
    n = 1024
    o = np.stack([rng.uniform(-50, 50, n), rng.uniform(-9.5, -7.0, n), rng.uniform(-50, 50, n)], axis=1)
    d = rng.normal(size=(n, 3)) * (2.0, 3.0, 2.0)
    size = (rng.uniform(0.1, 0.6, (n, 3)),) if shape == "box" else (rng.uniform(0.1, 0.6, n), rng.uniform(0.0, 0.8, n))
    m = T.mover.moves(o, d, *size, rotations=unit_quats(rng, n), max_slides=rng.integers(0, 9, n))
    got, counts, touches = _check(w, shape, "move", rec, m, "one collider")
    assert (counts >= 1).mean() > 0.2 and (got["slides"] <= 1).all()
    wk = T.mover.walks(o, d, *size, max_slides=rng.integers(0, 9, n), snap_distance=0.3, step_height=0.4)
    got, counts, touches = _check(w, shape, "walk", rec, wk, "one collider, walks")
    assert (counts >= 1).mean() > 0.2 and (touches["hit"]["collider"][HT.written(counts, HT.WALK_K)] == 0).all()
    w.close()

    scene = S.pile(300, 300, seed=3)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    for boxes, spheres, what in ((0, 300, "spheres only"), (301, 0, "boxes only")):
        w.set_counts(nb, boxes, spheres)
        w.query_build()
        rec = _records(w, scene)
        _, counts, touches = _check(w, shape, "move", rec, TB.world_moves(shape, "pile", rec, w.nbox, 2048, seed=70), what)
        assert (counts >= 1).mean() > 0.2
        assert (touches["hit"]["shape"][HT.written(counts, HT.MOVE_K)] == (E.NH_SHAPE_BOX if boxes else E.NH_SHAPE_SPHERE)).all()
    w.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_4096_coincident_boxes(shape):
    scene = S.pile(4096, 0, seed=3)
    scene["body_transforms"]["position"][1:] = (0.25, 3.0, -0.5)        # every Morton key equal but the ground's
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    rng = np.random.default_rng(1140)
    m = (TB.BMB if shape == "box" else TB.MB).moves(rng, rec, w.nbox, 1024, free_share=0.5)
    got, counts, touches = _check(w, shape, "move", rec, m, "4096 coincident boxes")
    HT.check_move_identities(got, counts, touches, "4096 coincident boxes")
    # half the moves start inside the heap: START OVERLAP at once, the tie among thousands of t = 0 hits going to the lowest index -- and the touch is that collider
    start = (got["flags"] & E.NH_MOVE_START_OVERLAP) != 0
    assert start.mean() > 0.2
    first = start & (got["slides"] == 0)
    assert first.any() and (counts[first] == 1).all() and (touches["hit"]["t"][first, 0] == 0).all()
    assert touches["hit"][first, 0].tobytes() == got["last_hit"][first].tobytes() and (touches["hit"]["shape"][first, 0] == E.NH_SHAPE_BOX).all()
    w.close()


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["move", "walk"])
@pytest.mark.parametrize("shape", SHAPES)
def test_abi_edge_cases(shape, kind):
    import torch
    name, result, k_max = CALL[shape, kind]
    T = TB.SHAPES[shape]
    scene = WB.terrain() if kind == "walk" else S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    fn = getattr(w.L, f"nh_{name}_touched")
    rec0 = Q.records(scene["body_transforms"], scene)
    n = 1024
    recs = TB.terrain_walks(shape, n, seed=6) if kind == "walk" else TB.world_moves(shape, "pile", rec0, len(scene["box_tags"]), n, seed=80)
    t = _upload(w, recs)
    size = result.itemsize
    out = torch.full((n + 1, size), SENTINEL, dtype=torch.uint8, device=w.dev)
    cnt = torch.full((n + 1, 4), SENTINEL, dtype=torch.uint8, device=w.dev)
    tch = torch.full((n + 1, k_max, 64), SENTINEL, dtype=torch.uint8, device=w.dev)
    ptr = lambda x, byte=0: C.c_void_p(x.data_ptr() + byte)               # noqa: E731
    call = lambda ctx=w.ctx, a=ptr(t), count=n, r=ptr(out), k=k_max, c=ptr(cnt), x=ptr(tch), flags=0: fn(ctx, a, count, r, k, c, x, flags)      # noqa: E731
    assert call() == 1                                                     # before any build: NH_ERR_INVALID
    assert call(ctx=None) == 1
    w.query_build()
    assert call(flags=1) == 1 and call(flags=0x80000000) == 1              # flags != 0
    assert call(count=1 << 30) == 1 and call(count=0xFFFFFFFF) == 1        # count >= 2^30
    assert call(k=0) == 1 and call(k=k_max + 1) == 1 and call(k=0xFFFFFFFF) == 1      # k out of range
    assert call(a=None) == 1 and call(r=None) == 1 and call(c=None) == 1 and call(x=None) == 1      # null
    for byte in (4, 8):                                                    # not 16-byte aligned
        assert call(a=ptr(t, byte), count=n - 1) == 1 and call(r=ptr(out, byte), count=n - 1) == 1 and call(x=ptr(tch, byte), count=n - 1) == 1
    for byte in (1, 2):                                                    # counts not 4-byte aligned
        assert call(c=ptr(cnt, byte), count=n - 1) == 1
    assert call(count=0) == 0 and fn(w.ctx, None, 0, None, k_max, None, None, 0) == 0          # count = 0: a no-op
    assert call(count=0, flags=4) == 1 and call(count=0, k=0) == 1         # (the flags and k are checked first)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((cnt == SENTINEL).all()) and bool((tch == SENTINEL).all())      # a refused call writes nothing

    # invalid records mixed into a valid batch: the plain call's invalid result, counts 0, no touch; two calls, the same bytes
    rec = _records(w, scene)
    bad = np.random.default_rng(1150).choice(1000, size=40, replace=False)
    recs["origin"][bad[:10], 1] = np.nan
    recs["displacement"][bad[10:20], 0] = np.inf
    recs["skin"][bad[20:30]] = -0.01
    recs["max_slides"][bad[30:40]] = 9
    got, counts, touches = _check(w, shape, kind, rec, recs[:1000], "invalid records in a valid batch")
    _same(got, _plain(w, shape, kind, recs[:1000]), "beside the plain call")
    invalid = E.NH_WALK_INVALID if kind == "walk" else E.NH_MOVE_INVALID
    assert (got["flags"][bad] == invalid).all() and (counts[bad] == 0).all() and (got["flags"][np.setdiff1d(np.arange(1000), bad)] != invalid).all()
    again, counts2, touches2 = _touched(w, shape, kind, recs[:1000])
    _same(again, got, "two calls")
    HT.same_touches(touches2, counts2, touches, counts, "two calls")
    # the Python front end with touched = k gives the raw call's bytes
    pick = np.setdiff1d(np.arange(1000), bad)[:256]
    v = recs[pick]
    shape_args = (v["size"],) if shape == "box" else (v["radius"], v["half_height"])
    kw = dict(rotations=v["rotation"], skin=v["skin"], max_slides=v["max_slides"].astype(np.int64), ignore_body=v["ignore_body"].astype(np.int64), synchronize=True)
    if kind == "walk":
        kw.update(up=v["up"], step_height=v["step_height"], snap_distance=v["snap_distance"], min_ground_up=v["min_ground_up"], probe_only=(v["options"] & 1).astype(np.int64))
    for k in (k_max, 2):
        py = getattr(w, name)(v["origin"], v["displacement"], *shape_args, touched=k, **kw)
        assert py["raw"].cpu().numpy().tobytes() == got[pick].tobytes()
        assert np.array_equal(py["touch_count"].cpu().numpy(), counts[pick])
        raw = np.frombuffer(py["touches"]["raw"].cpu().numpy().tobytes(), dtype=E.TOUCH).reshape(len(pick), k)
        HT.same_touches(raw, counts[pick], touches[pick], counts[pick], f"the front end, k = {k}")
        wr = HT.written(counts[pick], k)
        for field in ("t", "body", "collider", "shape", "tag"):
            assert np.array_equal(py["touches"][field].cpu().numpy()[wr], touches[pick]["hit"][field][:, :k][wr]), field
        for field in ("origin", "direction", "phase", "cast"):
            assert np.array_equal(py["touches"][field].cpu().numpy()[wr], touches[pick][field][:, :k][wr]), field
    plain = getattr(w, name)(v["origin"], v["displacement"], *shape_args, **kw)
    assert "touches" not in plain and "touch_count" not in plain and plain["raw"].cpu().numpy().tobytes() == got[pick].tobytes()
    w.close()


# ---- observers -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_touched_walks_between_nh_step_calls_change_nothing(shape):
    scene = OBSERVED["pile"]()
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    rec0 = Q.records(scene["body_transforms"], scene)
    walks = _world_walks(shape, np.random.default_rng(1160), rec0, len(scene["box_tags"]), 2048)
    moves = TB.SHAPES[shape].mover.head(walks)
    wt, mt = _upload(a, walks), _upload(a, moves)
    torch = a.torch
    rw, rm = torch.empty((2048, 112), dtype=torch.uint8, device=a.dev), torch.empty((2048, 64), dtype=torch.uint8, device=a.dev)
    cn = torch.empty(2048, dtype=torch.int32, device=a.dev)
    tw, tm = torch.empty((2048, HT.WALK_K, 64), dtype=torch.uint8, device=a.dev), torch.empty((2048, 4, 64), dtype=torch.uint8, device=a.dev)
    walk_name, move_name = CALL[shape, "walk"][0], CALL[shape, "move"][0]

    def query():
        a.query_build()
        getattr(a, walk_name + "_touched_records")(wt, HT.WALK_K, results=rw, counts=cn, touches=tw)
        getattr(a, move_name + "_touched_records")(mt, 4, results=rm, counts=cn, touches=tm)

    done = 0
    for k in [1, 2, 3, 5, 7, 4, 8] * 4:
        k = min(k, 100 - done)
        if k <= 0:
            break
        query()
        a.step(k)
        b.step(k)
        done += k
    query()
    assert done == 100
    _same_stepped_world(a, b, f"pile, touched {shape} walks and moves between nh_step calls")
    a.close(); b.close()
