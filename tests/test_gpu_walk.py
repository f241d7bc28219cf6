"""nh_walk on the GPU (pytest -m gpu): a grounded character step on the scene BVH (include/nudge_hip.h, "nh_walk").

The oracle is the host's brute force (tests/hostoracle/hostmover.cpp through tests/hostmover_util.py): the phase machine of nudge_amd/csrc/nh_query.h,
"walk" -- the functions the kernel runs -- around a capsule cast over every collider, so the kernel's 112 bytes per walk must equal it bit for bit.  The
identities of the header are tested against the GPU's own nh_move, nh_capsulecast and nh_spherecast."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostmover_util as MV                  # noqa: E402
import hostquery_util as Q                   # noqa: E402
import walk_batches as WB                    # noqa: E402
from hostmover_util import CAPSULE as HW     # noqa: E402
from mover_util import (FUSED, NONE, SENTINEL, capsulecast as _capsulecast, move as _move, records as _records, same as _same,      # noqa: E402
                        terrain_world as _terrain_world, walk as _walk)
from test_cpu_walk import BALL_PIT_SHARES, RESTING, TERRAIN_SEED, TERRAIN_SHARES, WORLD_SEED, WORLD_SHARES, check_shares      # noqa: E402
from query_util import OBSERVED, SMALL, same_stepped_world as _same_stepped_world, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu


def test_terrain_walks_equal_the_brute_force():
    w, scene, rec = _terrain_world()
    walks = WB.terrain_walks(np.random.default_rng(TERRAIN_SEED), 2048)
    ref = HW.walk(rec, w.nbox, walks)
    got = _walk(w, walks)
    _same(got, ref, "terrain")
    check_shares(walks, got, TERRAIN_SHARES, "terrain")
    # identity 5
    live = (got["flags"] & (E.NH_WALK_INVALID | E.NH_MOVE_START_OVERLAP)) == 0
    assert (got["casts"][live] <= E.NH_WALK_MAX_CASTS).all()
    g = (got["flags"] & E.NH_WALK_GROUNDED) != 0
    u = (got["ground"]["normal"].astype(np.float64) * walks["up"]).sum(axis=1)
    assert (u[g] > 0).all() and (u[g] >= walks["min_ground_up"][g] - 2.0 ** -22).all()
    w.close()


def _world_need(name, resting):
    if name == "ball_pit":
        return BALL_PIT_SHARES
    return WORLD_SHARES if resting else dict(grounded=WORLD_SHARES["grounded"])


@pytest.mark.parametrize("name", sorted(SMALL))
def test_walks_equal_the_brute_force_before_and_after_stepping(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(WORLD_SEED + sorted(SMALL).index(name))
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    walks = WB.world_walks(rng, rec, w.nbox, 2048)
    got = _walk(w, walks)
    _same(got, HW.walk(rec, w.nbox, walks), f"{name} initial")
    check_shares(walks, got, _world_need(name, name in RESTING), f"{name} initial")
    w.step(50)
    # the refit of the tree built before the bodies moved, then a new build: the same bytes (identity 4)
    w.query_refit()
    rec = _records(w, scene)
    walks = WB.world_walks(rng, rec, w.nbox, 2048)
    refit = _walk(w, walks)
    _same(refit, HW.walk(rec, w.nbox, walks), f"{name} after 50 steps, refit")
    check_shares(walks, refit, _world_need(name, name in RESTING), f"{name} after 50 steps")
    w.query_build()
    _same(_walk(w, walks), refit, f"{name} after 50 steps, built")
    if name == "pile":
        # the pile's bodies fall from up to 300 units: landed, it has steps to climb like the others
        w.step(1500)
        w.query_refit()
        rec = _records(w, scene)
        walks = WB.world_walks(rng, rec, w.nbox, 2048)
        landed = _walk(w, walks)
        _same(landed, HW.walk(rec, w.nbox, walks), "pile landed, refit")
        check_shares(walks, landed, WORLD_SHARES, "pile landed")
    w.close()


def test_without_its_rules_a_walk_is_nh_move():
    """Identity 1, against the GPU's own nh_move."""
    w, scene, rec = _terrain_world()
    walks = WB.terrain_walks(np.random.default_rng(TERRAIN_SEED + 1), 2048)
    walks["step_height"], walks["snap_distance"], walks["min_ground_up"] = 0.0, 0.0, 0.0
    got = _walk(w, walks)
    mv = _move(w, HW.head(walks))
    assert got.view(np.uint8).reshape(-1, 112)[:, :64].tobytes() == mv.tobytes()
    miss = np.zeros(1, dtype=E.RAY_HIT)
    miss["t"], miss["body"], miss["collider"], miss["shape"], miss["tag"] = 1.0, NONE, NONE, NONE, NONE
    assert got["ground"].tobytes() == np.repeat(miss, len(got)).tobytes() and (mv["slides"] >= 1).mean() >= 0.25
    w.close()
    # ... and on a world of bodies
    scene = SMALL["grid_tiles"]()
    w = E.World(scene, flags=FUSED)
    w.step(20)
    w.query_build()
    rec = _records(w, scene)
    walks = WB.world_walks(np.random.default_rng(WORLD_SEED + 20), rec, w.nbox, 2048)
    walks["step_height"], walks["snap_distance"], walks["min_ground_up"] = 0.0, 0.0, 0.0
    got = _walk(w, walks)
    assert got.view(np.uint8).reshape(-1, 112)[:, :64].tobytes() == _move(w, HW.head(walks)).tobytes()
    w.close()


@pytest.mark.parametrize("where", ["terrain", "grid_tiles"])
def test_replay_from_the_host_gives_the_same_bytes(where):
    """Identity 2: the phases run from the host -- GPU nh_move calls for A, U, F and D, a GPU nh_capsulecast call for C, nh_query.h's decisions between them
    -- give nh_walk's 112 bytes."""
    if where == "terrain":
        w, scene, rec = _terrain_world()
        walks = WB.terrain_walks(np.random.default_rng(TERRAIN_SEED + 2), 2048)
    else:
        scene = SMALL[where]()
        w = E.World(scene, flags=FUSED)
        w.step(30)
        w.query_build()
        rec = _records(w, scene)
        walks = WB.world_walks(np.random.default_rng(WORLD_SEED + 21), rec, w.nbox, 2048)
    walks["min_ground_up"] = 0.0
    got = _walk(w, walks)
    ref, calls = HW.replay_walk(walks, lambda m: _move(w, m), lambda c: _capsulecast(w, c))
    _same(got, ref, f"replay on {where}")
    s = MV.shares(walks, got)
    assert s["stepped"] >= 0.02 and s["snapped"] >= 0.05 and calls >= 6, (s, calls)
    w.close()


def test_half_height_zero_does_not_read_the_rotation():
    """Identity 3; and a ball's walk with max_slides 0 and no rules casts what nh_spherecast casts."""
    w, scene, rec = _terrain_world()
    walks = WB.terrain_walks(np.random.default_rng(TERRAIN_SEED + 3), 2048)
    walks["origin"][:, 1] -= walks["half_height"]                          # the balls stand where the capsules' lower ends stood
    walks["half_height"] = 0.0
    walks["rotation"] = MV.IDENTITY
    plain = _walk(w, walks)
    _same(plain, HW.walk(rec, w.nbox, walks), "balls")
    walks["rotation"] = np.nan
    _same(_walk(w, walks), plain, "balls with NaN rotations")
    s = MV.shares(walks, plain)
    assert (plain["flags"] & E.NH_WALK_INVALID == 0).all() and s["stepped"] >= 0.05 and s["snapped"] >= 0.05, s
    walks["max_slides"], walks["step_height"], walks["snap_distance"], walks["min_ground_up"] = 0, 0.0, 0.0, 0.0
    sph = np.zeros(len(walks), dtype=E.SPHERE_CAST)
    sph["origin"], sph["max_t"], sph["direction"], sph["ignore_body"], sph["radius"] = walks["origin"], 1.0, walks["displacement"], walks["ignore_body"], walks["radius"]
    hits = np.frombuffer(w.spherecast_records(_upload(w, sph)).cpu().numpy().tobytes(), dtype=E.RAY_HIT)
    assert _walk(w, walks)["last_hit"].tobytes() == hits.tobytes()
    w.close()


# ---- layer masks ----------------------------------------------------------------------------------------------------------------------------
def test_walks_under_layer_masks_equal_the_brute_force_over_the_masked_world():
    w, scene, rec = _terrain_world()
    words = np.full(len(rec), 2, dtype=np.uint32)
    words[0] = 1                                                           # the floor (box 0) alone in layer 1
    w.query_set_layers(words[:w.nbox], words[w.nbox:])
    walks = WB.terrain_walks(np.random.default_rng(TERRAIN_SEED + 4), 2048)
    open_lane = WB.terrain_walks(np.random.default_rng(TERRAIN_SEED + 5), 512)
    open_lane["origin"][:, 2] = WB.LANE["open"]                            # nothing but the floor under or before these
    open_lane["origin"][:, 1] = WB.SKIN + open_lane["radius"] + open_lane["half_height"]
    open_lane["snap_distance"], open_lane["options"] = 0.3, 0
    walks = np.concatenate([open_lane, walks])
    n = len(open_lane)
    off = _walk(w, walks)
    _same(off, HW.walk(rec, w.nbox, walks), "filter off")
    assert ((off["flags"][:n] & E.NH_WALK_GROUNDED) != 0).all()
    # a mask that hides the floor's layer: every walk over the open floor is airborne
    w.query_filter(2)
    hidden = _walk(w, walks)
    _same(hidden, HW.walk(rec, w.nbox, walks, words=words, mask=2), "uniform mask 2")
    assert (hidden["flags"][:n] == 0).all() and (hidden["ground"]["shape"][:n] == NONE).all() and (hidden["casts"][:n] >= 1).all()
    assert hidden["position"][:n].tobytes() == (walks["origin"][:n] + walks["displacement"][:n]).tobytes()
    for mask in (3, 1, 0):
        w.query_filter(mask)
        got = _walk(w, walks)
        _same(got, HW.walk(rec, w.nbox, walks, words=words, mask=mask), f"uniform mask {mask}")
        if mask == 3:
            _same(got, off, "mask 3 beside filter off")
    # per-query masks, alternating within every wave
    masks = np.where(np.arange(len(walks)) % 2 == 0, 2, 3).astype(np.uint32)
    mt = _upload(w, masks).view(w.torch.int32)
    w.query_filter(mt)
    got = _walk(w, walks)
    _same(got, HW.walk(rec, w.nbox, walks, words=words, masks=masks), "per-query masks")
    assert (got["flags"][:n][0::2] == 0).all() and ((got["flags"][:n][1::2] & E.NH_WALK_GROUNDED) != 0).all()
    w.query_filter(None)
    _same(_walk(w, walks), off, "filter off again")
    w.close()


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_abi_edge_cases():
    import torch
    scene = WB.terrain()
    w = E.World(scene, flags=FUSED)
    L = w.L
    walks = WB.terrain_walks(np.random.default_rng(TERRAIN_SEED + 6), 1024)
    t = _upload(w, walks)
    out = torch.full((1024 + 1, 112), SENTINEL, dtype=torch.uint8, device=w.dev)
    ptr = lambda x, byte=0: C.c_void_p(x.data_ptr() + byte)               # noqa: E731
    assert L.nh_walk(w.ctx, ptr(t), 1024, ptr(out), 0) == 1                # before any build: NH_ERR_INVALID
    assert L.nh_walk(None, ptr(t), 1024, ptr(out), 0) == 1
    w.query_build()
    assert L.nh_walk(w.ctx, ptr(t), 1024, ptr(out), 1) == 1                # flags != 0
    assert L.nh_walk(w.ctx, ptr(t), 1024, ptr(out), 0x80000000) == 1
    assert L.nh_walk(w.ctx, ptr(t), 1 << 30, ptr(out), 0) == 1             # count >= 2^30
    assert L.nh_walk(w.ctx, ptr(t), 0xFFFFFFFF, ptr(out), 0) == 1
    assert L.nh_walk(w.ctx, None, 1024, ptr(out), 0) == 1                  # null
    assert L.nh_walk(w.ctx, ptr(t), 1024, None, 0) == 1
    for byte in (4, 8):                                                    # not 16-byte aligned
        assert L.nh_walk(w.ctx, ptr(t, byte), 1023, ptr(out), 0) == 1
        assert L.nh_walk(w.ctx, ptr(t), 1023, ptr(out, byte), 0) == 1
    assert L.nh_walk(w.ctx, ptr(t), 0, ptr(out), 0) == 0                   # count = 0: a no-op
    assert L.nh_walk(w.ctx, None, 0, None, 0) == 0
    assert L.nh_walk(w.ctx, ptr(t), 0, ptr(out), 4) == 1                   # (the flags are checked first)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                   # a refused call writes nothing, and neither does count = 0

    # invalid records mixed into a valid batch; nothing behind `count` results; two calls, the same bytes
    rec = _records(w, scene)
    bad = np.random.default_rng(TERRAIN_SEED + 7).choice(1000, size=130, replace=False)
    walks["origin"][bad[:10], 1] = np.nan
    walks["displacement"][bad[10:20], 0] = np.inf
    walks["radius"][bad[20:30]] = -1.0
    walks["half_height"][bad[30:40]] = np.nan
    walks["skin"][bad[40:50]] = -0.01
    walks["max_slides"][bad[50:60]] = 9
    walks["rotation"][bad[60:70], 2] = np.nan
    walks["half_height"][bad[60:70]] = 0.5
    walks["up"][bad[70:80], 0] = np.nan
    walks["up"][bad[80:90]] = (0.0, 1.002, 0.0)
    walks["step_height"][bad[90:100]] = -0.5
    walks["snap_distance"][bad[100:110]] = np.inf
    walks["min_ground_up"][bad[110:120]] = 1.5
    walks["options"][bad[120:130]] = 2
    t = _upload(w, walks)
    assert L.nh_walk(w.ctx, ptr(t), 1000, ptr(out), 0) == 0
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert (raw[1000:] == SENTINEL).all()
    got = np.frombuffer(raw[:1000].tobytes(), dtype=E.WALK_RESULT)
    _same(got, HW.walk(rec, w.nbox, walks[:1000]), "invalid records in a valid batch")
    good = np.setdiff1d(np.arange(1000), bad)
    assert (got["flags"][bad] == E.NH_WALK_INVALID).all() and ((got["flags"][good] & E.NH_WALK_INVALID) == 0).all()
    assert got["position"][bad].tobytes() == walks["origin"][bad].tobytes() and got["remaining"][bad].tobytes() == walks["displacement"][bad].tobytes()
    for field in ("last_hit", "ground"):
        assert np.isnan(got[field]["t"][bad]).all() and (got[field]["shape"][bad] == NONE).all()
    assert (got["casts"][bad] == 0).all() and (got["reserved"] == 0).all()
    again = torch.full((1000, 112), SENTINEL, dtype=torch.uint8, device=w.dev)
    assert L.nh_walk(w.ctx, ptr(t), 1000, ptr(again), 0) == 0
    torch.cuda.synchronize()
    assert again.cpu().numpy().tobytes() == raw[:1000].tobytes()
    # the Python front end packs the same records
    k = good[:256]
    v = walks[k]
    py = w.walk(v["origin"], v["displacement"], v["radius"], v["half_height"], rotations=v["rotation"], skin=v["skin"], max_slides=v["max_slides"].astype(np.int64),
                ignore_body=v["ignore_body"].astype(np.int64), up=v["up"], step_height=v["step_height"], snap_distance=v["snap_distance"],
                min_ground_up=v["min_ground_up"], probe_only=(v["options"] & 1).astype(np.int64), synchronize=True)
    assert py["raw"].cpu().numpy().tobytes() == got[k].tobytes()
    assert np.array_equal(py["slides"].cpu().numpy(), got["slides"][k]) and np.array_equal(py["flags"].cpu().numpy(), got["flags"][k])
    assert np.array_equal(py["casts"].cpu().numpy(), got["casts"][k]) and py["step_up"].cpu().numpy().tobytes() == got["step_up"][k].tobytes()
    assert py["position"].cpu().numpy().tobytes() == got["position"][k].tobytes() and py["drop"].cpu().numpy().tobytes() == got["drop"][k].tobytes()
    assert np.array_equal(py["ground"]["shape"].cpu().numpy(), got["ground"]["shape"][k]) and np.array_equal(py["last_hit"]["shape"].cpu().numpy(), got["last_hit"]["shape"][k])
    # the slope limit in degrees is the cosine
    deg = w.walk(v["origin"], v["displacement"], v["radius"], v["half_height"], max_slope_degrees=45.0, snap_distance=0.3, synchronize=True)
    cos = w.walk(v["origin"], v["displacement"], v["radius"], v["half_height"], min_ground_up=float(np.float32(np.cos(np.deg2rad(45.0)))), snap_distance=0.3,
                 synchronize=True)
    assert deg["raw"].cpu().numpy().tobytes() == cos["raw"].cpu().numpy().tobytes()
    w.close()


# ---- observers -----------------------------------------------------------------------------------------------------------------------------
def test_walks_between_nh_step_calls_change_nothing():
    scene = OBSERVED["pile"]()
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    rec0 = Q.records(scene["body_transforms"], scene)
    walks = WB.world_walks(np.random.default_rng(WORLD_SEED + 30), rec0, len(scene["box_tags"]), 2048)
    wt = _upload(a, walks)
    rt = a.torch.empty((2048, 112), dtype=a.torch.uint8, device=a.dev)
    done = 0
    for k in [1, 2, 3, 5, 7, 4, 8] * 4:
        k = min(k, 100 - done)
        if k <= 0:
            break
        a.query_build()
        a.walk_records(wt, results=rt)
        a.step(k)
        b.step(k)
        done += k
    a.query_build()
    a.walk_records(wt, results=rt)
    assert done == 100
    _same_stepped_world(a, b, "pile, walks between nh_step calls")
    a.close(); b.close()


# ---- degenerate worlds ---------------------------------------------------------------------------------------------------------------------
def test_degenerate_worlds():
    scene = S.pile(4, 0, seed=3)
    w = E.World(scene, flags=FUSED)
    w.set_counts(len(scene["body_transforms"]), 1, 0)          # the ground slab alone (body 0), top at y = -10
    w.query_build()
    rng = np.random.default_rng(WORLD_SEED + 40)
    rec = _records(w, scene)
    walks = WB.terrain_walks(rng, 1024)
    walks["origin"][:, 1] += -10.0
    got = _walk(w, walks)
    _same(got, HW.walk(rec, w.nbox, walks), "one collider")
    s = MV.shares(walks, got)
    assert s["grounded"] > 0.4 and s["stepped"] == 0 and (got["slides"] <= 1).all(), s          # (one convex collider is never hit twice)
    w.close()

    scene = S.pile(300, 300, seed=3)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    w.set_counts(nb, 0, 300)
    w.query_build()
    rec = _records(w, scene)
    walks = WB.world_walks(rng, rec, w.nbox, 2048, slab_share=0.0)
    got = _walk(w, walks)
    _same(got, HW.walk(rec, w.nbox, walks), "spheres only")
    assert MV.shares(walks, got)["slid"] > 0.1
    w.close()


def test_4096_coincident_boxes():
    scene = S.pile(4096, 0, seed=3)
    scene["body_transforms"]["position"][1:] = (0.25, 3.0, -0.5)        # every Morton key equal but the ground's
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    walks = WB.world_walks(np.random.default_rng(WORLD_SEED + 41), rec, w.nbox, 1024, slab_share=0.3, free_share=0.5)
    got = _walk(w, walks)
    _same(got, HW.walk(rec, w.nbox, walks), "4096 coincident boxes")
    start = (got["flags"] & E.NH_MOVE_START_OVERLAP) != 0
    assert start.mean() > 0.2 and (~start).mean() > 0.2
    assert (got["last_hit"]["t"][start] == 0).all() and (got["ground"]["shape"][start] == NONE).all() and (got["casts"][start] >= 1).all()
    w.close()
