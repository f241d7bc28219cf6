"""nh_boxmove on the GPU (pytest -m gpu): collide-and-slide for swept oriented boxes on the scene BVH (include/nudge_hip.h, "nh_boxmove, nh_boxwalk").

The oracle is the host's brute force (tests/hostoracle/hostmover.cpp through tests/hostmover_util.py): the state machine of nudge_amd/csrc/nh_query.h,
"move" -- the functions the kernel runs -- around a box cast over every collider, so the kernel's 64 bytes per move must equal it bit for bit.  The
identities of the header are tested against the GPU's own nh_boxcast and nh_move: max_slides = 0, size 0, and the REPLAY of the loop from the host."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boxmove_batches as BMB                # noqa: E402
import hostmover_util as MV                  # noqa: E402
import hostquery_util as Q                   # noqa: E402
from hostmover_util import BOX as HBM, CAPSULE as HM      # noqa: E402
from mover_util import FUSED, NONE, SENTINEL, boxcast as _boxcast, boxmove as _boxmove, records as _records, same as _same      # noqa: E402
from test_cpu_boxmove import BATCH_SEED, DRAW      # noqa: E402
from query_util import OBSERVED, SMALL, same_stepped_world as _same_stepped_world, unit_quats, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu


def _check_world(w, scene, rng, n, what, **kw):
    """n moves against the brute force; returns (the moves, the GPU's results)."""
    rec = _records(w, scene)
    m = BMB.moves(rng, rec, w.nbox, n, **kw)
    ref = HBM.move(rec, w.nbox, m)
    got = _boxmove(w, m)
    _same(got, ref, what)
    return m, got


@pytest.mark.parametrize("name", sorted(SMALL))
def test_moves_equal_the_brute_force_before_and_after_stepping(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(BATCH_SEED + sorted(SMALL).index(name))
    draw = DRAW.get(name, 4)
    w = E.World(scene, flags=FUSED)
    w.query_build()
    _, got = _check_world(w, scene, rng, 4096, f"{name} initial", draw=draw)
    once, twice = BMB.shares(got)
    assert once >= 0.25 and twice >= 0.02, (once, twice)
    w.step(50)
    # the refit of the tree built before the bodies moved, then a new build: the same bytes (identity 6)
    w.query_refit()
    m, refit = _check_world(w, scene, rng, 4096, f"{name} after 50 steps, refit", draw=draw)
    once, twice = BMB.shares(refit)
    assert once >= 0.25 and twice >= 0.02, (once, twice)
    w.query_build()
    _same(_boxmove(w, m), refit, f"{name} after 50 steps, built")
    w.close()


@pytest.mark.parametrize("name", ["pile", "compound"])
def test_max_slides_zero_is_the_box_cast(name):
    """Identity 1."""
    scene = SMALL[name]()
    w = E.World(scene, flags=FUSED)
    w.step(20)
    w.query_build()
    rec = _records(w, scene)
    m = BMB.moves(np.random.default_rng(BATCH_SEED + 10), rec, w.nbox, 4096)
    m["max_slides"] = 0
    got = _boxmove(w, m)
    hits = _boxcast(w, HBM.first_casts(m))
    assert got["last_hit"].tobytes() == hits.tobytes()
    assert ((hits["shape"] != NONE) & (hits["t"] > 0)).mean() > 0.25 and (got["slides"] <= 1).all()
    w.close()


def test_size_zero_is_nh_move_of_a_point_and_does_not_read_the_rotation():
    """Identity 2, against the GPU's own nh_move."""
    scene = SMALL["grid_tiles"]()
    w = E.World(scene, flags=FUSED)
    w.step(20)
    w.query_build()
    rec = _records(w, scene)
    m = BMB.moves(np.random.default_rng(BATCH_SEED + 11), rec, w.nbox, 4096)
    m["size"] = 0.0
    m["rotation"] = MV.IDENTITY
    plain = _boxmove(w, m)
    _same(plain, HBM.move(rec, w.nbox, m), "rays")
    m["rotation"] = np.nan
    _same(_boxmove(w, m), plain, "rays with NaN rotations")
    assert (plain["flags"] & E.NH_MOVE_INVALID == 0).all() and BMB.shares(plain)[0] >= 0.1
    cm = HM.moves(m["origin"], m["displacement"], 0.0, 0.0, rotations=m["rotation"], skin=m["skin"], max_slides=m["max_slides"], ignore_body=m["ignore_body"])
    mv = np.frombuffer(w.move_records(_upload(w, cm)).cpu().numpy().tobytes(), dtype=E.MOVE_RESULT)
    _same(plain, mv, "nh_move with radius = half_height = 0")
    w.close()


def test_replay_from_the_host_gives_the_same_bytes():
    """Identity 3: the loop run from the host -- one GPU nh_boxcast per round, nh_q_move_advance (hbm_advance) between them -- gives nh_boxmove's bytes."""
    scene = SMALL["grid_tiles"]()
    w = E.World(scene, flags=FUSED)
    w.step(30)
    w.query_build()
    rec = _records(w, scene)
    m = BMB.moves(np.random.default_rng(BATCH_SEED + 12), rec, w.nbox, 2048)
    got = _boxmove(w, m)
    ref, rounds = HBM.replay_move(m, lambda c: _boxcast(w, c))
    _same(got, ref, "replay")
    assert 3 <= rounds <= E.NH_MOVE_MAX_SLIDES + 1 and BMB.shares(got)[1] >= 0.02
    w.close()


def test_degenerate_worlds():
    scene = S.pile(4, 0, seed=3)
    w = E.World(scene, flags=FUSED)
    w.set_counts(len(scene["body_transforms"]), 1, 0)          # the ground slab alone (body 0)
    w.query_build()
    rng = np.random.default_rng(BATCH_SEED + 13)
    rec = _records(w, scene)
    m = HBM.moves(np.stack([rng.uniform(-50, 50, 1024), rng.uniform(-9.0, -7.0, 1024), rng.uniform(-50, 50, 1024)], axis=1),
                  rng.normal(size=(1024, 3)) * (2.0, 3.0, 2.0), rng.uniform(0.1, 0.6, (1024, 3)), rotations=unit_quats(rng, 1024),
                  max_slides=rng.integers(0, 9, 1024))
    got = _boxmove(w, m)
    _same(got, HBM.move(rec, w.nbox, m), "one collider")
    assert BMB.shares(got)[0] > 0.2 and (got["slides"] <= 1).all()          # (one convex collider is never hit twice)
    w.close()

    scene = S.pile(300, 300, seed=3)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    w.set_counts(nb, 0, 300)
    w.query_build()
    _, got = _check_world(w, scene, rng, 2048, "spheres only")
    assert BMB.shares(got)[0] > 0.2
    w.set_counts(nb, 301, 0)
    w.query_build()
    _, got = _check_world(w, scene, rng, 2048, "boxes only")
    assert BMB.shares(got)[0] > 0.2
    w.close()


def test_4096_coincident_boxes():
    scene = S.pile(4096, 0, seed=3)
    scene["body_transforms"]["position"][1:] = (0.25, 3.0, -0.5)        # every Morton key equal but the ground's
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rng = np.random.default_rng(BATCH_SEED + 14)
    m, got = _check_world(w, scene, rng, 1024, "4096 coincident boxes", free_share=0.5)
    # half the moves start inside the heap: START OVERLAP at once, the tie among thousands of t = 0 hits going to the lowest index (the oracle's rule,
    # nh_q_better, checked bit for bit above); the others meet it from outside
    start = (got["flags"] & E.NH_MOVE_START_OVERLAP) != 0
    assert (start & (got["slides"] == 0)).mean() > 0.2 and (~start).mean() > 0.2
    assert (got["last_hit"]["t"][start] == 0).all() and (got["last_hit"]["shape"][start] == E.NH_SHAPE_BOX).all()
    w.close()


def test_a_scene_spanning_a_thousandth_and_ten_thousand_units():
    scene = S.pile(2000, 1000, seed=3)
    rng = np.random.default_rng(BATCH_SEED + 15)
    nb = len(scene["body_transforms"])
    small = rng.random(nb) < 0.5
    pos = np.where(small[:, None], rng.uniform(-0.05, 0.05, size=(nb, 3)), rng.uniform(-1e4, 1e4, size=(nb, 3))).astype(np.float32)
    scene["body_transforms"]["position"][1:] = pos[1:]
    bsmall = small[scene["box_transforms"]["body"][1:]]
    scene["box_data"]["size"][1:] = np.where(bsmall[:, None], np.float32(1e-3), np.float32(30.0))
    scene["sphere_data"]["radius"] = np.where(small[scene["sphere_transforms"]["body"]], np.float32(1e-3), np.float32(25.0))
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    is_small = np.concatenate([[False], bsmall, small[scene["sphere_transforms"]["body"]]])
    # movers of the local size, skin scaled with them
    for scale, pick, what in ((1e-3, is_small, "small cluster"), (30.0, ~is_small, "large bodies")):
        sub = rec.copy()
        sub["p"][~pick] = np.nan                                           # (the generator places its moves around these; the world stays whole)
        m = BMB.moves(rng, sub, w.nbox, 2048, scale=scale, bodies=nb)
        got = _boxmove(w, m)
        _same(got, HBM.move(rec, w.nbox, m), what)
        assert (got["flags"] & E.NH_MOVE_HIT != 0).mean() > 0.1, what
    w.close()


# ---- layer masks ----------------------------------------------------------------------------------------------------------------------------
def test_moves_under_layer_masks_equal_the_brute_force_over_the_masked_world():
    scene = SMALL["pile"]()
    w = E.World(scene, flags=FUSED)
    w.step(40)
    w.query_build()
    rec = _records(w, scene)
    words = np.full(len(rec), 2, dtype=np.uint32)
    words[0] = 1                                                           # the ground slab (box 0, body 0) alone in layer 1
    w.query_set_layers(words[:w.nbox], words[w.nbox:])
    rng = np.random.default_rng(BATCH_SEED + 16)
    n = 2048
    # boxes that drop onto the slab, away from the pile, and slide along it: top face at y = -10
    o = np.stack([rng.uniform(20, 300, n) * rng.choice([-1.0, 1.0], n), rng.uniform(-8.9, -7.0, n), rng.uniform(20, 300, n) * rng.choice([-1.0, 1.0], n)], axis=1)
    d = np.stack([rng.uniform(-3, 3, n), rng.uniform(-5.0, -3.5, n), rng.uniform(-3, 3, n)], axis=1)
    above = HBM.moves(o, d, (0.4, 0.3, 0.5), rotations=unit_quats(rng, n))
    m = np.concatenate([above, BMB.moves(rng, rec, w.nbox, n)])
    off = _boxmove(w, m)
    _same(off, HBM.move(rec, w.nbox, m), "filter off")
    assert ((off["flags"][:n] == E.NH_MOVE_HIT) & (off["slides"][:n] == 1)).all()
    # a mask that hides the slab's layer: the moves above it pass through
    w.query_filter(2)
    hidden = _boxmove(w, m)
    _same(hidden, HBM.move(rec, w.nbox, m, words=words, mask=2), "uniform mask 2")
    assert (hidden["flags"][:n] == 0).all() and hidden["position"][:n].tobytes() == (m["origin"][:n] + m["displacement"][:n]).tobytes()
    # the mask that sees everything writes the filter-off bytes; the one that sees only the slab, and mask 0
    for mask in (3, 1, 0):
        w.query_filter(mask)
        got = _boxmove(w, m)
        _same(got, HBM.move(rec, w.nbox, m, words=words, mask=mask), f"uniform mask {mask}")
        if mask == 3:
            _same(got, off, "mask 3 beside filter off")
    # per-query masks, alternating within every wave
    masks = np.where(np.arange(len(m)) % 2 == 0, 2, 3).astype(np.uint32)
    mt = _upload(w, masks).view(w.torch.int32)
    w.query_filter(mt)
    got = _boxmove(w, m)
    _same(got, HBM.move(rec, w.nbox, m, words=words, masks=masks), "per-query masks")
    assert (got["flags"][:n][0::2] == 0).all() and (got["flags"][:n][1::2] == E.NH_MOVE_HIT).all()
    w.query_filter(None)
    _same(_boxmove(w, m), off, "filter off again")
    w.close()


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_abi_edge_cases():
    import torch
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    L = w.L
    rec0 = Q.records(scene["body_transforms"], scene)
    m = BMB.moves(np.random.default_rng(BATCH_SEED + 17), rec0, len(scene["box_tags"]), 1024)
    t = _upload(w, m)
    out = torch.full((1024 + 1, 64), SENTINEL, dtype=torch.uint8, device=w.dev)
    ptr = lambda x, byte=0: C.c_void_p(x.data_ptr() + byte)               # noqa: E731
    assert L.nh_boxmove(w.ctx, ptr(t), 1024, ptr(out), 0) == 1             # before any build: NH_ERR_INVALID
    assert L.nh_boxmove(None, ptr(t), 1024, ptr(out), 0) == 1
    w.query_build()
    assert L.nh_boxmove(w.ctx, ptr(t), 1024, ptr(out), 1) == 1             # flags != 0
    assert L.nh_boxmove(w.ctx, ptr(t), 1024, ptr(out), 0x80000000) == 1
    assert L.nh_boxmove(w.ctx, ptr(t), 1 << 30, ptr(out), 0) == 1          # count >= 2^30
    assert L.nh_boxmove(w.ctx, ptr(t), 0xFFFFFFFF, ptr(out), 0) == 1
    assert L.nh_boxmove(w.ctx, None, 1024, ptr(out), 0) == 1               # null
    assert L.nh_boxmove(w.ctx, ptr(t), 1024, None, 0) == 1
    for byte in (4, 8):                                                    # not 16-byte aligned
        assert L.nh_boxmove(w.ctx, ptr(t, byte), 1023, ptr(out), 0) == 1
        assert L.nh_boxmove(w.ctx, ptr(t), 1023, ptr(out, byte), 0) == 1
    assert L.nh_boxmove(w.ctx, ptr(t), 0, ptr(out), 0) == 0                # count = 0: a no-op
    assert L.nh_boxmove(w.ctx, None, 0, None, 0) == 0
    assert L.nh_boxmove(w.ctx, ptr(t), 0, ptr(out), 4) == 1                # (the flags are checked first)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                   # a refused call writes nothing, and neither does count = 0

    # invalid records mixed into a valid batch; nothing behind `count` results; two calls, the same bytes
    rec = _records(w, scene)
    bad = np.random.default_rng(BATCH_SEED + 18).choice(1000, size=70, replace=False)
    m["origin"][bad[:10], 1] = np.nan
    m["displacement"][bad[10:20], 0] = np.inf
    m["size"][bad[20:30], 0] = -1.0
    m["size"][bad[30:40], 2] = np.nan
    m["skin"][bad[40:50]] = -0.01
    m["max_slides"][bad[50:60]] = 9
    m["rotation"][bad[60:70], 2] = np.nan
    m["size"][bad[60:70]] = (0.0, 0.5, 0.0)
    m["max_slides"][bad[0]] = 8                                            # (still invalid: its origin)
    t = _upload(w, m)
    assert L.nh_boxmove(w.ctx, ptr(t), 1000, ptr(out), 0) == 0
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert (raw[1000:] == SENTINEL).all()
    got = np.frombuffer(raw[:1000].tobytes(), dtype=E.MOVE_RESULT)
    ref = HBM.move(rec, w.nbox, m[:1000])
    _same(got, ref, "invalid records in a valid batch")
    good = np.setdiff1d(np.arange(1000), bad)
    assert (got["flags"][bad] == E.NH_MOVE_INVALID).all() and (got["flags"][good] != E.NH_MOVE_INVALID).all()
    assert got["position"][bad].tobytes() == m["origin"][bad].tobytes() and got["remaining"][bad].tobytes() == m["displacement"][bad].tobytes()
    assert np.isnan(got["last_hit"]["t"][bad]).all() and (got["last_hit"]["shape"][bad] == NONE).all()
    again = torch.full((1000, 64), SENTINEL, dtype=torch.uint8, device=w.dev)
    assert L.nh_boxmove(w.ctx, ptr(t), 1000, ptr(again), 0) == 0
    torch.cuda.synchronize()
    assert again.cpu().numpy().tobytes() == raw[:1000].tobytes()
    # the Python front end packs the same records
    k = good[:256]
    py = w.boxmove(m["origin"][k], m["displacement"][k], m["size"][k], rotations=m["rotation"][k], skin=m["skin"][k],
                   max_slides=m["max_slides"][k].astype(np.int64), ignore_body=m["ignore_body"][k].astype(np.int64), synchronize=True)
    assert py["raw"].cpu().numpy().tobytes() == got[k].tobytes()
    assert np.array_equal(py["slides"].cpu().numpy(), got["slides"][k]) and np.array_equal(py["flags"].cpu().numpy(), got["flags"][k])
    assert py["position"].cpu().numpy().tobytes() == got["position"][k].tobytes() and np.array_equal(py["last_hit"]["shape"].cpu().numpy(), got["last_hit"]["shape"][k])
    # rotations=None is the identity: the axis-aligned box of a voxel world
    ident = m[k].copy()
    ident["rotation"] = MV.IDENTITY
    py = w.boxmove(ident["origin"], ident["displacement"], ident["size"], skin=ident["skin"], max_slides=ident["max_slides"].astype(np.int64),
                   ignore_body=ident["ignore_body"].astype(np.int64), synchronize=True)
    assert py["raw"].cpu().numpy().tobytes() == _boxmove(w, ident).tobytes()
    w.close()


# ---- observers -----------------------------------------------------------------------------------------------------------------------------
def test_moves_between_nh_step_calls_change_nothing():
    # (the observer tests' pile, boxes only, as in tests/test_gpu_move.py)
    scene = OBSERVED["pile"]()
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    rec0 = Q.records(scene["body_transforms"], scene)
    m = BMB.moves(np.random.default_rng(BATCH_SEED + 19), rec0, len(scene["box_tags"]), 2048)
    mt = _upload(a, m)
    rt = a.torch.empty((2048, 64), dtype=a.torch.uint8, device=a.dev)
    done = 0
    for k in [1, 2, 3, 5, 7, 4, 8] * 4:
        k = min(k, 100 - done)
        if k <= 0:
            break
        a.query_build()
        a.boxmove_records(mt, results=rt)
        a.step(k)
        b.step(k)
        done += k
    a.query_build()
    a.boxmove_records(mt, results=rt)
    assert done == 100
    _same_stepped_world(a, b, "pile, box moves between nh_step calls")
    a.close(); b.close()
