"""First-k casts on the GPU (pytest -m gpu): nh_raycast_k / nh_spherecast_k / nh_boxcast_k / nh_capsulecast_k (include/nudge_hip.h, "scene queries").

The oracle is tests/hostcastk_util.py: the all-hits brute forces' segments cut at k and padded with the closest-hit brute force's miss -- plain Python
over oracles that share no code with the kernel.  `counts` and all count * k records must equal it byte for byte; `hits` is pre-filled with a sentinel
and a guard region behind record count * k must come back untouched; counts = NULL must write the same `hits`.  k = 1 must be the closest-hit call on
the GPU itself, the first 8 of k = 32 the k = 8 call, the degenerate shapes the simpler call, a refit the build, and the calls are observers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import castk_batches as CB                   # noqa: E402
import hostcast_util as CAST                 # noqa: E402
import hostcastk_util as HK                  # noqa: E402
import hostquery_util as Q                   # noqa: E402
from cast_util import (GUARD, SENTINEL, box_casts, capsule_casts, casts_through, closest as _closest, coincident,      # noqa: E402
                       far_and_near_scene as _far_and_near_scene, first_k as _gpu, sphere_casts, wide_casts)
from query_util import FUSED, NONE, OBSERVED, SMALL, rays as _rays, records as _records, same_stepped_world as _same_stepped_world, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 8, 9, 16, 17, 32)             # both sides of each block-size step (256 lanes up to 8, 128 up to 16, 64 up to 32)
STILL = ("still_steps", "still_replays", "ahead_steps", "pair_steps", "asleep_steps")


def _differ(a, b):
    return int((np.ascontiguousarray(a).view(np.uint8).reshape(-1, 32) != np.ascontiguousarray(b).view(np.uint8).reshape(-1, 32)).any(axis=1).sum())


def _same(w, rec, casts, what, ks=KS, seg=None, closest=True):
    """Every k of `ks` against the oracle, with and without counts; k = 1 against the closest-hit call (`closest`) and k = 32 against k = 8 on the
    GPU itself.  Returns every byte the GPU wrote."""
    seg = seg if seg is not None else HK.segments(rec, w.nbox, casts)
    out, by_k = [], {}
    for k in ks:
        counts, hits = _gpu(w, casts, k)
        ref_counts, ref_hits = HK.cast_k(rec, w.nbox, casts, k, seg)
        assert counts.tobytes() == ref_counts.tobytes(), f"{what} k {k}: {int((counts != ref_counts).sum())} of {len(counts)} counts differ"
        assert hits.tobytes() == ref_hits.tobytes(), f"{what} k {k}: {_differ(hits, ref_hits)} of {hits.size} records differ"
        assert _gpu(w, casts, k, with_counts=False)[1].tobytes() == hits.tobytes(), f"{what} k {k}: counts = NULL writes other records"
        by_k[k] = hits
        out += [counts.tobytes(), hits.tobytes()]
    if closest and 1 in by_k:
        assert by_k[1][:, 0].tobytes() == _closest(w, casts).tobytes(), f"{what}: k = 1 differs from the closest-hit call"
    if 8 in by_k and 32 in by_k:
        assert np.ascontiguousarray(by_k[32][:, :8]).tobytes() == by_k[8].tobytes(), f"{what}: the first 8 of k = 32 differ from k = 8"
    return out


def _check_world(w, scene, rng, what):
    """1000 casts per shape (no multiple of a block size) against the tree the world has now; the shares that keep the comparison from being empty."""
    rec = _records(w, scene)
    out = []
    for shape, casts in CB.batches(rng, 1000, rec).items():
        seg = HK.segments(rec, w.nbox, casts)
        k = CB.assert_not_empty(seg[0], f"{what} {shape}")
        print(f"\n[{what} {shape}] shares at k = {k}: more %.3f, fewer %.3f, none %.3f" % CB.shares(seg[0], k), end="")
        out += _same(w, rec, casts, f"{what} / {shape}", seg=seg)
    return out


@pytest.mark.parametrize("name", sorted(SMALL))
def test_first_k_equal_the_oracle_built_stepped_and_refitted(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(700 + sorted(SMALL).index(name))
    w = E.World(scene, flags=FUSED)
    w.query_build()
    _check_world(w, scene, rng, f"{name} initial")
    w.step(50)
    w.query_build()
    state = rng.bit_generator.state
    built = _check_world(w, scene, rng, f"{name} after 50 steps")
    w.close()
    # the same with nh_query_refit in place of the second build: the same casts against the same oracle, and the build's bytes
    rng.bit_generator.state = state
    w = E.World(scene, flags=FUSED)
    w.query_build()
    w.step(50)
    w.query_refit()
    assert _check_world(w, scene, rng, f"{name} after 50 steps and a refit") == built
    w.close()


def test_ties_through_4096_coincident_boxes_are_the_lowest_indices_in_order():
    scene = coincident(4096)
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    rng = np.random.default_rng(740)
    rays = casts_through((0.25, 3.0, -0.5), 64, rng)
    batches = {"ray": rays, "sphere": sphere_casts(rays, invalid=False), "box": box_casts(rng, rays, invalid=False),
               "capsule": capsule_casts(rng, rays, invalid=False)}
    for shape, casts in batches.items():
        seg = HK.segments(rec, w.nbox, casts)
        assert (np.diff(seg[0].astype(np.int64)) == 4096).all(), shape
        _same(w, rec, casts, f"coincident / {shape}", ks=(1, 5, 32), seg=seg)
        counts, hits = _gpu(w, casts, 32)
        assert (counts == 32).all() and (hits["collider"] == np.arange(1, 33)).all() and (hits["shape"] == E.NH_SHAPE_BOX).all(), shape
        assert (hits["t"].copy().view(np.uint32) == hits["t"][:, :1].copy().view(np.uint32)).all(), shape
    w.close()


@pytest.mark.parametrize("colliders", [0, 1, 2])
def test_tiny_worlds_are_rows_of_misses(colliders):
    scene = S.pile(4, 0, seed=3)
    w = E.World(scene, flags=FUSED)
    w.set_counts(len(scene["body_transforms"]), colliders, 0)      # the ground slab (body 0) first
    w.query_build()
    rec = _records(w, scene)
    assert len(rec) == colliders
    rng = np.random.default_rng(750 + colliders)
    full = Q.records(w.get_bodies()["transforms"], scene)
    for shape, casts in CB.batches(rng, 1000, full).items():
        seg = HK.segments(rec, w.nbox, casts)
        assert int(seg[0][-1]) > (100 if colliders else -1), (shape, int(seg[0][-1]))
        _same(w, rec, casts, f"{colliders} colliders / {shape}", ks=(1, 32), seg=seg)
    w.close()


def _as(casts, dtype):
    out = np.zeros(len(casts), dtype=dtype)
    for name in dtype.names:
        if name in casts.dtype.names and name != "reserved":
            out[name] = casts[name]
    return out


def test_degenerate_shapes_write_the_simpler_calls_bytes_on_a_world_of_a_thousandth_to_ten_thousand_units():
    scene = _far_and_near_scene()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    rng = np.random.default_rng(760)
    batches = wide_casts(rng, rec)
    # (against the oracle alone: from 1e4 units away the ray predicates accept a sphere of 1e-3 by rounding, outside the box the closest-hit walk pads
    # by 2^-18 -- DESIGN 10.8 -- so nh_raycast itself may miss the first record of such a ray here; the k walk takes the all-hits pad and lists it)
    for shape, casts in batches.items():
        _same(w, rec, casts, f"1e-3 .. 1e4 / {shape}", ks=(1, 3, 17), closest=False)
    rays = batches["ray"]
    for k in (1, 4, 32):
        ray = _gpu(w, rays, k)
        assert int(ray[0].sum()) > 256
        # a ball of r = 0 (and -0), a box of size 0 and a capsule of r = hh = 0, whatever their rotations: the ray call's bytes
        ball = sphere_casts(rays, np.float32([0.0, -0.0]), invalid=False)
        box = box_casts(rng, rays, sizes=np.float32([(0, 0, 0), (-0.0, 0.0, -0.0)]), invalid=False)
        cap = capsule_casts(rng, rays, shapes=np.float32([(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0)]), invalid=False)
        box["rotation"][::3] = np.nan
        cap["rotation"][::3] = np.nan
        for what, casts in (("r = 0", ball), ("size 0", box), ("r = hh = 0", cap)):
            got = _gpu(w, casts, k)
            assert got[0].tobytes() == ray[0].tobytes() and got[1].tobytes() == ray[1].tobytes(), f"k {k}: {what} differs from nh_raycast_k"
        # a capsule of half height 0 is the ball of its radius, invalid radii included
        cap = capsule_casts(rng, rays, shapes=np.float32([(1e-4, 0.0), (5.0, 0.0), (100.0, -0.0), (0.0, 0.0)]), invalid=False)
        cap["rotation"][::3] = np.nan
        cap["radius"][5::40], cap["radius"][6::40] = np.nan, -1.0
        ball, got = _gpu(w, _as(cap, E.SPHERE_CAST), k), _gpu(w, cap, k)
        assert int(ball[0].sum()) > 256
        assert got[0].tobytes() == ball[0].tobytes() and got[1].tobytes() == ball[1].tobytes(), f"k {k}: hh = 0 differs from nh_spherecast_k"
    w.close()


def test_two_identical_calls_give_identical_bytes():
    scene = SMALL["grid_tiles"]()
    w = E.World(scene, flags=FUSED)
    w.step(20)
    w.query_build()
    rec = _records(w, scene)
    for shape, casts in CB.batches(np.random.default_rng(770), 4000, rec).items():
        for k in (3, 12, 32):
            a, b = _gpu(w, casts, k), _gpu(w, casts, k)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (shape, k)
    w.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CB.SHAPES)
def test_abi_edge_cases(shape):
    import torch
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    fn = getattr(w.L, "nh_%scast_k" % shape)
    rec = Q.records(w.get_bodies()["transforms"], scene)
    casts = CB.batches(np.random.default_rng(780), 1024, rec)[shape]
    ct = _upload(w, casts)
    k = 4
    buf = torch.zeros(1032, dtype=torch.int32, device=w.dev)
    nt = buf[:1024]
    ht = torch.zeros((1024 * k + GUARD, 32), dtype=torch.uint8, device=w.dev)
    cp, np_, hp = C.c_void_p(ct.data_ptr()), C.c_void_p(nt.data_ptr()), C.c_void_p(ht.data_ptr())
    assert fn(w.ctx, cp, 1024, k, np_, hp, 0) == 1                     # before any build: NH_ERR_INVALID
    assert fn(None, cp, 1024, k, np_, hp, 0) == 1
    w.query_build()
    assert fn(w.ctx, cp, 1024, k, np_, hp, E.NH_RAY_ANY_HIT) == 1      # flags: NH_RAY_ANY_HIT has no meaning here
    assert fn(w.ctx, cp, 1024, k, np_, hp, 2) == 1
    assert fn(w.ctx, cp, 1024, 0, np_, hp, 0) == 1                     # k = 0, k = 33
    assert fn(w.ctx, cp, 1024, 33, np_, hp, 0) == 1
    assert fn(w.ctx, cp, 0, 0, np_, hp, 0) == 1                        # ... refused before count = 0 is looked at, as in nh_closest_k
    assert fn(w.ctx, None, 1024, k, np_, hp, 0) == 1                   # null / unaligned casts
    assert fn(w.ctx, C.c_void_p(ct.data_ptr() + 4), 1023, k, np_, hp, 0) == 1
    assert fn(w.ctx, cp, 1024, k, np_, None, 0) == 1                   # null / unaligned hits
    assert fn(w.ctx, cp, 1024, k, np_, C.c_void_p(ht.data_ptr() + 8), 0) == 1
    assert fn(w.ctx, cp, 1024, k, C.c_void_p(nt.data_ptr() + 2), hp, 0) == 1      # unaligned counts
    assert fn(w.ctx, cp, 1 << 30, k, np_, hp, 0) == 1                  # count >= 2^30: refused on the host, nothing launched
    assert fn(w.ctx, cp, 0xFFFFFFFF, k, np_, hp, 0) == 1
    assert fn(w.ctx, cp, 0, k, np_, hp, 0) == 0                        # count 0: a no-op
    assert fn(w.ctx, None, 0, 32, None, None, 0) == 0
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0 and int(ht.sum()) == 0            # nothing was written
    # counts need 4-byte alignment only; hits hold exactly count * k records
    n4 = buf[1:1025]
    assert fn(w.ctx, cp, 1024, k, C.c_void_p(n4.data_ptr()), hp, 0) == 0
    ref_counts, ref_hits = HK.cast_k(rec, w.nbox, casts, k)
    assert 0 < int(ref_counts.sum()) < 1024 * k
    assert n4.cpu().numpy().view(np.uint32).tobytes() == ref_counts.tobytes() and int(buf[0]) == 0 and int(buf[1025:].abs().sum()) == 0
    got = np.frombuffer(ht.cpu().numpy().tobytes(), dtype=E.RAY_HIT)
    assert got[:1024 * k].tobytes() == ref_hits.tobytes() and not got[1024 * k:].view(np.uint8).any()
    # the Python wrapper: (counts, the nh_RayHit decode shaped (n, k))
    head = dict(max_t=torch.from_numpy(casts["max_t"].copy()), ignore_body=torch.from_numpy(casts["ignore_body"].astype(np.int64)))
    o, d = casts["origin"].copy(), casts["direction"].copy()
    if shape == "ray":
        counts, hits = w.raycast_k(o, d, k, synchronize=True, **head)
    elif shape == "sphere":
        counts, hits = w.spherecast_k(o, d, casts["radius"].copy(), k, synchronize=True, **head)
    elif shape == "box":
        counts, hits = w.boxcast_k(o, d, casts["size"].copy(), k, rotations=casts["rotation"].copy(), synchronize=True, **head)
    else:
        counts, hits = w.capsulecast_k(o, d, casts["radius"].copy(), casts["half_height"].copy(), k, rotations=casts["rotation"].copy(), synchronize=True, **head)
    assert counts.shape == (1024,) and hits["t"].shape == (1024, k) and hits["normal"].shape == (1024, k, 3) and hits["collider"].shape == (1024, k)
    assert np.array_equal(counts.cpu().numpy(), ref_counts) and hits["raw"].cpu().numpy().tobytes() == ref_hits.tobytes()
    assert np.array_equal(hits["collider"].cpu().numpy(), ref_hits["collider"]) and np.array_equal(hits["shape"].cpu().numpy(), ref_hits["shape"])
    w.close()


# ---- observers -----------------------------------------------------------------------------------------------------------------------------
def _observer_batch(a):
    import torch
    rays = _rays(np.random.default_rng(790), 1000, (-30, -12, -30), (30, 20, 30), "random")
    rng = np.random.default_rng(791)
    casts = [rays, sphere_casts(rays), box_casts(rng, rays), capsule_casts(rng, rays)]
    return [_upload(a, c) for c in casts], torch.empty(1000, dtype=torch.int32, device=a.dev), torch.empty((1000 * 32, 32), dtype=torch.uint8, device=a.dev)


def _query(w, casts, nt, ht, turn):
    if turn and turn % 3 == 0:
        w.query_refit()
    else:
        w.query_build()
    for j, (shape, ct) in enumerate(zip(CB.SHAPES, casts)):
        getattr(w, CAST.SHAPES[shape].call + "_k_records")(ct, KS[(turn + 2 * j) % len(KS)], counts=nt, hits=ht)


@pytest.mark.parametrize("name", sorted(OBSERVED))
def test_first_k_casts_between_nh_step_calls_change_nothing(name):
    scene = OBSERVED[name]()
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    batch = _observer_batch(a)
    done = turn = 0
    for k in [1, 2, 3, 5, 7, 4, 8] * 10:
        k = min(k, 300 - done)
        if k <= 0:
            break
        _query(a, *batch, turn)
        a.step(k)
        b.step(k)
        done += k
        turn += 1
    _query(a, *batch, turn)
    assert done == 300
    _same_stepped_world(a, b, f"{name} nh_step")
    ca, cb = a.counts(), b.counts()
    assert all(ca[key] == cb[key] for key in STILL), (ca, cb)
    if name == "grid_tiles":
        assert ca["still_steps"] > 0, ca
    a.close(); b.close()


@pytest.mark.parametrize("name", sorted(OBSERVED))
def test_first_k_casts_between_every_call_of_the_fused_step_change_nothing(name):
    scene = OBSERVED[name]()
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    batch = _observer_batch(a)
    calls = ("collide", "gravity", "read_cache", "setup", "apply", "update", "write_cache", "advance")
    turn = 0
    for s in range(300):
        for name_ in calls:
            _query(a, *batch, turn)
            turn += 1
            getattr(a, name_)()
            getattr(b, name_)()
        a.step_done(); b.step_done()
    _query(a, *batch, turn)
    _same_stepped_world(a, b, f"{name} call by call")
    ca, cb = a.counts(), b.counts()
    assert all(ca[key] == cb[key] for key in STILL), (ca, cb)
    if name == "grid_tiles":
        assert ca["still_steps"] > 0, ca
    a.close(); b.close()


# ---- the loop over casts ----------------------------------------------------------------------------------------------------------------------
def test_a_million_rays_on_4097_colliders_go_round_the_loop_with_lists_that_start_empty():
    """2^20 rays at k = 4 are 4096 workgroups of 256 lanes, more than the launch's grid: every lane takes more than one cast.  The same rays in eight
    calls of 2^17 (512 workgroups each: one cast per lane) must give the same bytes, a sample must equal the oracle, and every first record the
    closest-hit call."""
    import torch
    n = 4096
    scene = S.pile(n, 0, seed=3)
    j = np.arange(n)
    scene["body_transforms"]["position"][1:] = np.stack([1.5 * (j % 512), 3.0 + 4.0 * (j // 512), np.zeros(n)], axis=1).astype(np.float32)   # 8 rows of 512 boxes
    scene["body_transforms"]["rotation"][1:] = (0.0, 0.0, 0.0, 1.0)
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    rng = np.random.default_rng(795)
    m, k = 1 << 20, 4
    rays = np.zeros(m, dtype=E.RAY)
    rays["ignore_body"], rays["max_t"] = NONE, np.inf
    rays["origin"] = np.stack([rng.uniform(-20, 800, size=m), rng.uniform(0, 36, size=m), rng.uniform(-2, 2, size=m)], axis=1)
    d = np.zeros((m, 3))
    d[:, 0] = rng.choice([-1.0, 1.0], size=m)
    d[:, 1] = rng.normal(scale=0.02, size=m)
    rays["direction"] = d
    rays["origin"][::7, 1] = 3.0 + 4.0 * rng.integers(0, 8, size=len(rays[::7]))       # a seventh exactly along a row: hundreds of hits, lists that fill and evict
    rays["direction"][::7, 1] = 0.0
    rays["max_t"][1::2] = rng.uniform(0, 60, size=m // 2)
    rt = _upload(w, rays)
    ht = torch.full((m * k + GUARD, 32), SENTINEL, dtype=torch.uint8, device=w.dev)
    nt = torch.full((m + GUARD,), -1, dtype=torch.int32, device=w.dev)
    w.raycast_k_records(rt, k, counts=nt, hits=ht)
    assert bool((ht[m * k:] == SENTINEL).all()) and bool((nt[m:] == -1).all())
    # in pieces that need no loop
    hp = torch.empty((m * k, 32), dtype=torch.uint8, device=w.dev)
    npieces = torch.empty(m, dtype=torch.int32, device=w.dev)
    step = 1 << 17
    for at in range(0, m, step):
        w.raycast_k_records(rt[32 * at:32 * (at + step)], k, counts=npieces[at:at + step], hits=hp[at * k:(at + step) * k])
    assert torch.equal(nt[:m], npieces) and torch.equal(ht[:m * k], hp)
    counts = nt[:m].cpu().numpy()
    assert (counts == k).mean() > 0.1 and (counts == 0).any() and ((counts > 0) & (counts < k)).any()
    # k = 1 of every ray is the closest-hit call's record
    assert torch.equal(ht[:m * k].reshape(m, k, 32)[:, 0], w.raycast_records(rt))
    # a sample against the oracle: lanes of the first trip round the loop and of the later ones
    pick = np.unique(np.concatenate([np.linspace(0, m - 1, 1024).astype(np.int64), np.arange(0, 256), np.arange(m // 2, m // 2 + 256), np.arange(m - 256, m)]))
    ref_counts, ref_hits = HK.cast_k(rec, w.nbox, rays[pick], k)
    got = np.frombuffer(ht[:m * k].reshape(m, k * 32)[torch.from_numpy(pick).to(w.dev)].cpu().numpy().tobytes(), dtype=E.RAY_HIT)
    assert np.array_equal(counts[pick].view(np.uint32), ref_counts) and got.tobytes() == ref_hits.tobytes()
    w.close()
