"""Scene queries on the GPU (pytest -m gpu): nh_query_build / nh_raycast (include/nudge_hip.h, "scene queries").

The oracle is a brute force over every collider on the host with the same per-item arithmetic (nudge_amd/csrc/nh_query.h through
tests/hostquery_util.py): closest hit is defined exactly -- smallest t, ties by (shape, collider index) -- so the tree's answer must equal it bit
for bit in every field.  Queries are observers: worlds that answer them between every pair of entry points must step exactly like worlds that do not."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostcast_util as CAST                 # noqa: E402
import hostquery_util as Q                   # noqa: E402
from cast_util import closest as _cast, far_and_near, same_hits as _same_hits      # noqa: E402
from query_util import FUSED, NONE, OBSERVED, SMALL, bounds as _bounds, rays as _rays, same_stepped_world as _same_stepped_world, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu


def _check_world(w, scene, rng, n, what):
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    hit_share = []
    for kind in ("random", "axis", "down"):
        rays = _rays(rng, n, lo, hi, kind)
        got = _cast(w, rays)
        ref = CAST.cast(CAST.RAY, rec, w.nbox, rays)
        _same_hits(got, ref, f"{what} / {kind}")
        hit_share.append(float((ref["shape"] != NONE).mean()))
    return hit_share


@pytest.mark.parametrize("name", sorted(SMALL))
def test_closest_hits_equal_the_brute_force_before_and_after_stepping(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(100 + sorted(SMALL).index(name))
    w = E.World(scene, flags=FUSED)
    share = _check_world(w, scene, rng, 65536, f"{name} initial")
    assert max(share) > 0.05, share
    w.step(50)
    share = _check_world(w, scene, rng, 65536, f"{name} after 50 steps")
    assert max(share) > 0.05, share
    w.close()


def test_a_single_collider():
    scene = S.pile(4, 0, seed=3)
    w = E.World(scene, flags=FUSED)
    w.set_counts(len(scene["body_transforms"]), 1, 0)          # the ground slab alone (body 0)
    rng = np.random.default_rng(1)
    _check_world(w, scene, rng, 4096, "one collider")
    rays = _rays(rng, 64, (-1, -12, -1), (1, -10, 1), "down")
    got = _cast(w, rays)
    assert (got["shape"] == E.NH_SHAPE_BOX).all() and (got["collider"] == 0).all() and (got["body"] == 0).all()
    w.close()


def test_only_spheres_and_only_boxes():
    scene = S.pile(300, 300, seed=3)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    rng = np.random.default_rng(2)
    w.set_counts(nb, 0, 300)
    _check_world(w, scene, rng, 16384, "spheres only")
    w.set_counts(nb, 301, 0)
    _check_world(w, scene, rng, 16384, "boxes only")
    w.close()


def test_four_thousand_boxes_at_one_position():
    scene = S.pile(4096, 0, seed=3)
    scene["body_transforms"]["position"][1:] = (0.25, 3.0, -0.5)        # every Morton key equal but the ground's
    w = E.World(scene, flags=FUSED)
    rng = np.random.default_rng(3)
    _check_world(w, scene, rng, 16384, "4096 coincident boxes")
    rays = _rays(rng, 256, (0.2, 3.0, -0.6), (0.3, 3.1, -0.4), "down")
    got = _cast(w, rays)
    assert (got["shape"] == E.NH_SHAPE_BOX).all()
    w.close()


def test_a_scene_spanning_a_thousandth_and_ten_thousand_units():
    scene = S.pile(2000, 1000, seed=3)
    rng = np.random.default_rng(4)
    far_and_near(scene, rng)
    w = E.World(scene, flags=FUSED)
    _check_world(w, scene, rng, 32768, "1e-3 .. 1e4")
    # rays at the small cluster from afar and from inside it
    rec = Q.records(w.get_bodies()["transforms"], scene)
    for lo, hi in (((-0.05,) * 3, (0.05,) * 3), ((-0.01,) * 3, (0.01,) * 3)):
        rays = _rays(rng, 16384, lo, hi, "random")
        _same_hits(_cast(w, rays), CAST.cast(CAST.RAY, rec, w.nbox, rays), f"small cluster {lo}")
    w.close()


def test_abi_edge_cases():
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED, capacity=dict(bodies=len(scene["body_transforms"]), boxes=65, spheres=16))
    L = w.L
    rays = _rays(np.random.default_rng(5), 1024, (-5, -10, -5), (5, 300, 5), "random")
    t = _upload(w, rays)
    import torch
    hits = torch.zeros((1024, 32), dtype=torch.uint8, device=w.dev)
    assert L.nh_raycast(w.ctx, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hits.data_ptr()), 0) == 1          # before any build: NH_ERR_INVALID
    assert L.nh_raycast(None, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hits.data_ptr()), 0) == 1
    w.query_build()
    assert L.nh_raycast(w.ctx, C.c_void_p(t.data_ptr()), 0, C.c_void_p(hits.data_ptr()), 0) == 0            # count 0: a no-op
    assert L.nh_raycast(w.ctx, None, 0, None, 0) == 0
    assert L.nh_raycast(w.ctx, C.c_void_p(t.data_ptr()), 1024, None, 0) == 1                                  # null hits
    assert L.nh_raycast(w.ctx, None, 1024, C.c_void_p(hits.data_ptr()), 0) == 1
    assert L.nh_raycast(w.ctx, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hits.data_ptr()), 2) == 1           # unknown flag
    assert L.nh_query_build(w.ctx, None, C.byref(w.colliders)) == 1
    w.torch.cuda.synchronize()
    assert int(hits.sum()) == 0                                                                               # nothing was written
    # the world shrinks: the rebuild must not answer with colliders that are gone
    full = _cast(w, rays)
    assert (full["collider"][full["shape"] == E.NH_SHAPE_SPHERE] >= 8).any() and (full["collider"][full["shape"] == E.NH_SHAPE_BOX] >= 33).any()
    w.set_counts(len(scene["body_transforms"]), 33, 8)
    w.query_build()
    got = _cast(w, rays)
    rec = Q.records(w.get_bodies()["transforms"], scene, 33, 8)
    _same_hits(got, CAST.cast(CAST.RAY, rec, 33, rays), "after set_counts")
    assert not ((got["shape"] == E.NH_SHAPE_BOX) & (got["collider"] >= 33)).any()
    assert not ((got["shape"] == E.NH_SHAPE_SPHERE) & (got["collider"] >= 8)).any()
    # ... and grows back
    w.set_counts(len(scene["body_transforms"]), 65, 16)
    w.query_build()
    _same_hits(_cast(w, rays), full, "grown back")
    w.close()


@pytest.mark.parametrize("name", ["pile", "grid_tiles"])
def test_any_hit_agrees_with_closest_hit_about_hit_or_miss(name):
    scene = SMALL[name]()
    w = E.World(scene, flags=FUSED)
    w.step(30)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(6)
    for kind in ("random", "axis", "down"):
        rays = _rays(rng, 32768, lo, hi, kind)
        rays["max_t"] = rng.choice([np.inf, 5.0, 50.0], size=len(rays))
        closest, anyh = _cast(w, rays), _cast(w, rays, any_hit=True)
        assert np.array_equal(closest["shape"] == NONE, anyh["shape"] == NONE), kind
        miss = anyh["shape"] == NONE
        assert anyh[miss].tobytes() == closest[miss].tobytes()
        idx = np.nonzero(~miss)[0]
        assert len(idx) > 100
        assert (anyh["t"][idx] <= rays["max_t"][idx]).all()
        for i in idx[:: max(1, len(idx) // 500)]:
            c = int(anyh["collider"][i]) + (0 if anyh["shape"][i] == E.NH_SHAPE_BOX else w.nbox)
            one = CAST.cast(CAST.RAY, rec, w.nbox, rays[i:i + 1], only=c)[0]
            assert one.tobytes() == anyh[i].tobytes(), (kind, i)
    w.close()


# ---- observers -----------------------------------------------------------------------------------------------------------------------------
def _query(w, rays_t, hits_t):
    w.query_build()
    w.raycast_records(rays_t, hits=hits_t)
    w.raycast_records(rays_t, any_hit=True, hits=hits_t)


@pytest.mark.parametrize("name", sorted(OBSERVED))
def test_queries_between_nh_step_calls_change_nothing(name):
    scene = OBSERVED[name]()
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    rays = _rays(np.random.default_rng(7), 4096, (-30, -12, -30), (30, 20, 30), "random")
    rt = _upload(a, rays)
    ht = a.torch.empty((4096, 32), dtype=a.torch.uint8, device=a.dev)
    lengths = [1, 2, 3, 5, 7, 4, 8] * 10
    done = 0
    for k in lengths:
        k = min(k, 300 - done)
        if k <= 0:
            break
        _query(a, rt, ht)
        a.step(k)
        b.step(k)
        done += k
    _query(a, rt, ht)
    assert done == 300
    _same_stepped_world(a, b, f"{name} nh_step")
    c = a.counts()
    print(f"\n[{name}, nh_step] " + ", ".join(f"{k} {c[k]}" for k in ("still_steps", "still_replays", "ahead_steps", "pair_steps", "asleep_steps")))
    if name == "grid_tiles":                        # (a pile never takes still steps: tests/test_gpu_still.py)
        assert c["still_steps"] > 0, c
    a.close(); b.close()


@pytest.mark.parametrize("name", sorted(OBSERVED))
def test_queries_between_every_call_of_the_fused_step_change_nothing(name):
    scene = OBSERVED[name]()
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    rays = _rays(np.random.default_rng(8), 4096, (-30, -12, -30), (30, 20, 30), "random")
    rt = _upload(a, rays)
    ht = a.torch.empty((4096, 32), dtype=a.torch.uint8, device=a.dev)
    calls = ("collide", "gravity", "read_cache", "setup", "apply", "update", "write_cache", "advance")
    for s in range(300):
        for name_ in calls:
            _query(a, rt, ht)
            getattr(a, name_)()
            getattr(b, name_)()
        a.step_done(); b.step_done()
    _query(a, rt, ht)
    _same_stepped_world(a, b, f"{name} call by call")
    c = a.counts()
    print(f"\n[{name}, call by call] " + ", ".join(f"{k} {c[k]}" for k in ("still_steps", "still_replays", "ahead_steps", "pair_steps", "asleep_steps")))
    if name == "grid_tiles":
        assert c["still_steps"] > 0, c
    a.close(); b.close()


# ---- at size -------------------------------------------------------------------------------------------------------------------------------
def test_a_million_rays_on_the_landed_config_2_world():
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
    n_tiles = len(scene["tile_of_static"])
    w = E.World(scene, flags=FUSED, max_contacts=6 * nb)
    w.step(70)
    assert w.counts()["error"] == 0
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(9)
    n = 1 << 20
    # half the batch: downward rays into the tiles (within each ground slab's footprint), the rest random and axis-aligned over the whole world
    nd = n // 2
    tile = rng.integers(0, n_tiles, size=nd)
    centre = scene["box_transforms"]["position"][tile].astype(np.float64)
    half = scene["box_data"]["size"][tile, 0].astype(np.float64) - 0.5
    down = np.zeros(nd, dtype=E.RAY)
    down["origin"][:, 0] = centre[:, 0] + rng.uniform(-1, 1, size=nd) * half
    down["origin"][:, 1] = 20.0
    down["origin"][:, 2] = centre[:, 2] + rng.uniform(-1, 1, size=nd) * half
    down["direction"] = (0.0, -1.0, 0.0)
    down["max_t"] = np.inf
    down["ignore_body"] = NONE
    rays = np.concatenate([down, _rays(rng, n // 4, lo, hi, "random"), _rays(rng, n - nd - n // 4, lo, hi, "axis")])
    got = _cast(w, rays)
    # every downward ray hits its own tile: one of its bodies or its ground slab (box `tile` on body 0)
    g = got[:nd]
    assert (g["shape"] != NONE).all()
    slab = g["body"] == 0
    assert (g["collider"][slab] == tile[slab]).all()
    tob = scene["tile_of_body"]
    assert (tob[g["body"][~slab]] == tile[~slab]).all()
    assert (~slab).mean() > 0.2
    # 1024 rays spread over the batch, bit for bit against the brute force over all 1,004,524 colliders
    pick = np.linspace(0, n - 1, 1024).astype(np.int64)
    ref = CAST.cast(CAST.RAY, rec, w.nbox, rays[pick])
    _same_hits(got[pick], ref, "config 2, 1 M rays")
    w.close()
