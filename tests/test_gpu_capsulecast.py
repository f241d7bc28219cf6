"""Capsule casts and capsule overlaps on the GPU (pytest -m gpu): nh_capsulecast and nh_overlap's NH_SHAPE_CAPSULE (include/nudge_hip.h, "scene
queries").

The oracle is a brute force over every collider on the host with the same arithmetic (nudge_amd/csrc/nh_query.h through tests/hostcast_util.py and tests/hostcapsule_util.py)
and the header's exact rules, so the tree's answer must equal it bit for bit in every field.  Half height 0 must give nh_spherecast's bytes (and with
radius 0 nh_raycast's), the sphere and box queries of a mixed overlap batch must not notice the capsules beside them, and casts and capsule overlaps
are observers like the other queries."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostcapsule_util as H                 # noqa: E402
import hostcast_util as CAST                 # noqa: E402
import hostoverlap_util as O                 # noqa: E402
import hostquery_util as Q                   # noqa: E402
from cast_util import capsules as _casts, closest as _sweep, degenerate_worlds, same_hits as _same_hits, slide_past, spheres      # noqa: E402
from query_util import (FUSED, NONE, OBSERVED, SMALL, bounds as _bounds, mat, rays as _rays, same_stepped_world as _same_stepped_world,      # noqa: E402
                        unit_quats as _unit_quats, upload as _upload)
from test_gpu_overlap import SENTINEL, _capsule_queries, _gpu, _queries                                       # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = ((0.05, 0.5), (0.5, 0.5), (1.0, 2.0), (0.0, 1.0))         # (radius, half height)


def _check_world(w, scene, rng, n, what, shapes=SHAPES):
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    share = []
    for kind in ("random", "axis", "down"):
        for r, hh in shapes:
            for rot in (None, _unit_quats(rng, n)):
                casts = _casts(_rays(rng, n, lo, hi, kind), r, hh, rot)
                ref = CAST.cast(CAST.CAPSULE, rec, w.nbox, casts)
                _same_hits(_sweep(w, casts), ref, f"{what} / {kind} / r {r} hh {hh} / {'identity' if rot is None else 'rotated'}")
                share.append(float((ref["shape"] != NONE).mean()))
    return share


@pytest.mark.parametrize("name", sorted(SMALL))
def test_capsule_casts_equal_the_brute_force_before_and_after_stepping(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(400 + sorted(SMALL).index(name))
    w = E.World(scene, flags=FUSED)
    assert max(_check_world(w, scene, rng, 4096, f"{name} initial")) > 0.05
    w.step(50)
    assert max(_check_world(w, scene, rng, 4096, f"{name} after 50 steps")) > 0.05
    w.close()


def test_degenerate_worlds():
    degenerate_worlds(_check_world, np.random.default_rng(41), 2048, 2048, 1024, shapes=((0.5, 0.5),))


def test_mixed_radii_half_heights_rotations_ignore_body_and_max_t():
    scene = SMALL["pile"]()
    w = E.World(scene, flags=FUSED)
    w.step(30)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(42)
    n = 16384
    rays = np.concatenate([_rays(rng, n // 2, lo, hi, "random"), _rays(rng, n // 2, lo, hi, "axis")])
    rays["max_t"] = rng.choice([np.inf, 3.0, 12.0], size=n)
    rays["ignore_body"][::3] = rng.integers(0, 64, size=len(rays[::3]))
    r = rng.choice(np.float32([0.0, 0.1, 0.5, 1.5]), size=n)
    hh = rng.choice(np.float32([0.0, 0.25, 1.0, 3.0]), size=n)
    casts = _casts(rays, r, hh, _unit_quats(rng, n))
    casts["rotation"][(hh == 0.0) & (np.arange(n) % 2 == 0)] = np.nan          # (hh = 0 does not read the rotation)
    bad = rng.choice(n, size=64, replace=False)
    casts["radius"][bad[:16]] = -0.5
    casts["half_height"][bad[16:32]] = np.nan
    casts["rotation"][bad[32:48], 1] = np.inf
    casts["half_height"][bad[32:48]] = 1.0
    casts["origin"][bad[48:], 2] = np.nan
    ref = CAST.cast(CAST.CAPSULE, rec, w.nbox, casts)
    assert np.isnan(ref["t"][bad]).all()
    _same_hits(_sweep(w, casts), ref, "mixed")
    assert (ref["shape"] != NONE).mean() > 0.2
    w.close()


def test_grazing_casts_beside_resting_boxes():
    """Capsules that slide past a face of a resting box at the touching distance + offset, offsets 0 and +-1e-8 .. 1e-2, upright in the resting box's
    frame (the segment parallel to its faces) and turned at random: the walk's pruning is tested where the node test and the predicate are closest."""
    scene = S.stacks(64, 3, seed=5)
    w = E.World(scene, flags=FUSED)
    w.step(60)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    boxes = np.nonzero(rec["body"][: w.nbox] != 0)[0][:64]
    offs = [0.0] + [s * 10.0 ** e for e in range(-8, -1) for s in (-1.0, 1.0)]
    rng = np.random.default_rng(43)

    rows = []
    for k, c in enumerate(boxes):
        p, q, h = rec["p"][c].astype(np.float64), rec["q"][c], rec["h"][c].astype(np.float64)
        R = mat(q)
        for r, hh in ((0.05, 0.1), (0.3, 0.6)):
            for turned in (False, True):
                qc = _unit_quats(rng, 1)[0] if turned else q
                ext = np.abs(R.T @ mat(qc)[:, 1]) * hh + r              # the capsule's half extents along the resting box's axes
                for off in offs:
                    a, b = k % 3, (k + 1) % 3
                    for sb in (-1.0, 1.0):
                        rows.append((*slide_past(p, R, h, ext, a, b, sb, off), qc, r, hh))
    c = np.zeros(len(rows), dtype=E.CAPSULE_CAST)
    c["origin"] = [x[0] for x in rows]
    c["direction"] = [x[1] for x in rows]
    c["rotation"] = [x[2] for x in rows]
    c["radius"] = [x[3] for x in rows]
    c["half_height"] = [x[4] for x in rows]
    c["max_t"] = np.inf
    c["ignore_body"] = NONE
    ref = CAST.cast(CAST.CAPSULE, rec, w.nbox, c)
    _same_hits(_sweep(w, c), ref, "grazing")
    assert (ref["shape"] != NONE).mean() > 0.1
    w.close()


@pytest.mark.parametrize("name", ["pile", "grid_tiles", "ball_pit"])
def test_half_height_zero_equals_the_sphere_cast_and_the_ray_cast(name):
    scene = SMALL[name]()
    w = E.World(scene, flags=FUSED)
    w.step(20)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(44)
    for kind in ("random", "axis", "down"):
        rays = _rays(rng, 32768, lo, hi, kind)
        rays["max_t"][::3] = 7.0
        rays["ignore_body"][::5] = rng.integers(0, 64, size=len(rays[::5]))
        rot = _unit_quats(rng, len(rays))
        rot[::2] = np.nan
        radius = rng.choice(np.float32([0.0, 0.3, 1.2]), size=len(rays))
        got = _sweep(w, _casts(rays, radius, 0.0, rot))
        _same_hits(got, _sweep(w, spheres(rays, radius)), f"{name} / {kind}: hh 0 against nh_spherecast")
        _same_hits(_sweep(w, _casts(rays, 0.0, 0.0, rot)), _sweep(w, rays), f"{name} / {kind}: r = hh = 0 against nh_raycast")
    w.close()


@pytest.mark.parametrize("name", ["pile", "grid_tiles"])
def test_a_start_capsule_that_overlaps_hits_at_zero(name):
    scene = SMALL[name]()
    w = E.World(scene, flags=FUSED)
    w.step(30)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(45)
    n = 16384
    rays = _rays(rng, n, lo, hi, "random")
    rays["origin"] = rng.uniform(lo, hi, size=(n, 3))
    rays["ignore_body"][::4] = rng.integers(0, 64, size=len(rays[::4]))
    r = rng.uniform(0.05, 1.0, size=n).astype(np.float32)
    hh = rng.uniform(0.0, 1.5, size=n).astype(np.float32)
    rot = _unit_quats(rng, n)
    casts = _casts(rays, r, hh, rot)
    got = _sweep(w, casts)
    ov = w.overlap(rays["origin"], radii=r, half_heights=hh, rotations=rot, ignore_body=rays["ignore_body"].astype(np.int64), synchronize=True)
    off = ov["offsets"].cpu().numpy()
    touching = np.diff(off) > 0
    assert touching.mean() > 0.05, touching.mean()
    assert (got["t"][touching] == 0.0).all() and (got["shape"][touching] != NONE).all()
    first = off[:-1][touching]
    lowest = ov["collider"].cpu().numpy()[first] + np.where(ov["shape"].cpu().numpy()[first] == E.NH_SHAPE_SPHERE, w.nbox, 0)
    mine = got["collider"][touching].astype(np.int64) + np.where(got["shape"][touching] == E.NH_SHAPE_SPHERE, w.nbox, 0)
    assert (mine <= lowest).all()
    _same_hits(got, CAST.cast(CAST.CAPSULE, rec, w.nbox, casts), f"{name} start capsules")
    w.close()


@pytest.mark.parametrize("name", ["pile", "grid_tiles"])
def test_any_hit_agrees_with_closest_hit_about_hit_or_miss(name):
    scene = SMALL[name]()
    w = E.World(scene, flags=FUSED)
    w.step(30)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(46)
    for kind in ("random", "axis", "down"):
        rays = _rays(rng, 16384, lo, hi, kind)
        rays["max_t"] = rng.choice([np.inf, 5.0, 50.0], size=len(rays))
        casts = _casts(rays, rng.uniform(0.0, 1.0, size=len(rays)), rng.uniform(0.0, 2.0, size=len(rays)), _unit_quats(rng, len(rays)))
        closest, anyh = _sweep(w, casts), _sweep(w, casts, any_hit=True)
        assert np.array_equal(closest["shape"] == NONE, anyh["shape"] == NONE), kind
        miss = anyh["shape"] == NONE
        assert anyh[miss].tobytes() == closest[miss].tobytes()
        idx = np.nonzero(~miss)[0]
        assert len(idx) > 100
        assert (anyh["t"][idx] <= casts["max_t"][idx]).all()
        for i in idx[:: max(1, len(idx) // 300)]:
            c = int(anyh["collider"][i]) + (0 if anyh["shape"][i] == E.NH_SHAPE_BOX else w.nbox)
            one = CAST.cast(CAST.CAPSULE, rec, w.nbox, casts[i:i + 1], only=c)[0]
            assert one.tobytes() == anyh[i].tobytes(), (kind, i)
    w.close()


def test_abi_edge_cases():
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    L = w.L
    casts = _casts(_rays(np.random.default_rng(47), 1024, (-5, -10, -5), (5, 300, 5), "random"), 0.5, 0.5)
    t = _upload(w, casts)
    import torch
    hits = torch.zeros((1025, 32), dtype=torch.uint8, device=w.dev)
    hp = hits.data_ptr()
    assert L.nh_capsulecast(w.ctx, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hp), 0) == 1          # before any build: NH_ERR_INVALID
    assert L.nh_capsulecast(None, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hp), 0) == 1
    w.query_build()
    assert L.nh_capsulecast(w.ctx, C.c_void_p(t.data_ptr()), 0, C.c_void_p(hp), 0) == 0            # count 0: a no-op
    assert L.nh_capsulecast(w.ctx, None, 0, None, 0) == 0
    assert L.nh_capsulecast(w.ctx, C.c_void_p(t.data_ptr()), 1024, None, 0) == 1                    # null hits / casts
    assert L.nh_capsulecast(w.ctx, None, 1024, C.c_void_p(hp), 0) == 1
    assert L.nh_capsulecast(w.ctx, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hp), 2) == 1           # unknown flags
    assert L.nh_capsulecast(w.ctx, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hp), 3) == 1
    assert L.nh_capsulecast(w.ctx, C.c_void_p(t.data_ptr() + 4), 1023, C.c_void_p(hp), 0) == 1       # misaligned casts / hits
    assert L.nh_capsulecast(w.ctx, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hp + 8), 0) == 1
    w.torch.cuda.synchronize()
    assert int(hits.sum()) == 0                                                                     # nothing was written
    assert L.nh_capsulecast(w.ctx, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hp), 1) == 0
    w.torch.cuda.synchronize()
    assert int(hits[1024].sum()) == 0                                                               # nothing behind the last record
    w.close()


def test_the_python_wrappers_write_the_records_they_describe():
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    w.step(10)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    rng = np.random.default_rng(48)
    rays = _rays(rng, 2048, *_bounds(rec), "random")
    r = rng.uniform(0.1, 1.0, size=len(rays)).astype(np.float32)
    hh = rng.uniform(0.0, 1.5, size=len(rays)).astype(np.float32)
    rot = _unit_quats(rng, len(rays))
    rays["ignore_body"][::3] = 2
    out = w.capsulecast(rays["origin"], rays["direction"], r, hh, rot, max_t=40.0, ignore_body=rays["ignore_body"].astype(np.int64), synchronize=True)
    rays["max_t"] = 40.0
    ref = CAST.cast(CAST.CAPSULE, rec, w.nbox, _casts(rays, r, hh, rot))
    _same_hits(np.frombuffer(out["raw"].cpu().numpy().tobytes(), dtype=E.RAY_HIT), ref, "World.capsulecast")
    assert np.array_equal(out["collider"].cpu().numpy(), ref["collider"].astype(np.int64))
    out = w.capsulecast(rays["origin"], rays["direction"], 0.5, 1.0, synchronize=True)        # rotations=None: upright
    rays["max_t"] = np.inf
    rays["ignore_body"] = NONE
    _same_hits(np.frombuffer(out["raw"].cpu().numpy().tobytes(), dtype=E.RAY_HIT), CAST.cast(CAST.CAPSULE, rec, w.nbox, _casts(rays, 0.5, 1.0)), "upright")
    # World.overlap with half_heights: a capsule batch
    cen = rays["origin"][:512]
    ov = w.overlap(cen, radii=r[:512], half_heights=hh[:512], rotations=rot[:512], synchronize=True)
    q = np.zeros(512, dtype=E.OVERLAP_QUERY)
    q["center"], q["shape"], q["rotation"], q["ignore_body"] = cen, E.NH_SHAPE_CAPSULE, rot[:512], NONE
    q["size"][:, 0], q["size"][:, 1] = r[:512], hh[:512]
    ref_off, ref_hits, total = H.overlap(rec, w.nbox, q)
    assert np.array_equal(ov["offsets"].cpu().numpy(), ref_off.astype(np.int64))
    assert ov["raw"].cpu().numpy().tobytes() == ref_hits[:total].tobytes()
    w.close()


# ---- capsule overlaps ------------------------------------------------------------------------------------------------------------------------
def _same_capsule_overlaps(w, rec, queries, what, capacity=None):
    """Count only, then a list call with `capacity` (None: exactly the total), against hostcapsule's brute force; returns the total."""
    cnt, _ = _gpu(w, queries, None)
    ref_cnt, _, total = H.overlap(rec, w.nbox, queries, capacity=0)
    assert cnt.tobytes() == ref_cnt.tobytes(), f"{what}: count-only offsets differ in {int((cnt != ref_cnt).sum())} of {len(cnt)}"
    cap = total if capacity is None else capacity
    off, hits = _gpu(w, queries, cap)
    ref_hits = np.frombuffer(bytes([SENTINEL]) * 16 * max(cap, 1), dtype=E.OVERLAP_HIT).copy()
    ref_off, ref_hits, _ = H.overlap(rec, w.nbox, queries, capacity=cap, hits=ref_hits)
    assert off.tobytes() == ref_off.tobytes(), f"{what}: offsets differ"
    assert hits.tobytes() == ref_hits.tobytes(), \
        f"{what}: {int((hits.view(np.uint8).reshape(-1, 16) != ref_hits.view(np.uint8).reshape(-1, 16)).any(axis=1).sum())} of {len(hits)} records differ"
    return total


@pytest.mark.parametrize("name", sorted(SMALL))
def test_capsule_overlaps_equal_the_brute_force_in_mixed_batches(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(500 + sorted(SMALL).index(name))
    w = E.World(scene, flags=FUSED)
    for steps in (0, 40):
        w.step(steps)
        w.query_build()
        rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
        caps = _capsule_queries(rng, 4096, rec)
        assert _same_capsule_overlaps(w, rec, caps, f"{name} / {steps} steps / capsules") > 100
        other = _queries(rng, 4096, rec, "mixed")
        mixed = np.concatenate([caps, other])
        rng.shuffle(mixed)
        total = _same_capsule_overlaps(w, rec, mixed, f"{name} / {steps} steps / mixed")
        # the capacity prefix: about half of the records
        _same_capsule_overlaps(w, rec, mixed, f"{name} / {steps} steps / capacity", capacity=total // 2)
        # the sphere and box queries of the mixed batch give the bytes they give alone
        keep = mixed["shape"] != E.NH_SHAPE_CAPSULE
        off, hits = _gpu(w, mixed, total)
        alone_off, alone_hits = _gpu(w, mixed[keep], int(O.overlap(rec, w.nbox, mixed[keep], capacity=0)[2]))
        cnt = np.diff(off)
        assert np.array_equal(cnt[keep], np.diff(alone_off))
        mine = np.concatenate([hits[off[i]:off[i + 1]] for i in np.nonzero(keep)[0]] + [hits[:0]])
        assert mine.tobytes() == alone_hits[: len(mine)].tobytes() and len(mine) == alone_off[-1]
    w.close()


# ---- observers -----------------------------------------------------------------------------------------------------------------------------
def _query(w, casts_t, hits_t, queries_t, offsets_t):
    w.query_build()
    w.capsulecast_records(casts_t, hits=hits_t)
    w.capsulecast_records(casts_t, any_hit=True, hits=hits_t)
    w.overlap_records(queries_t, offsets=offsets_t)


@pytest.mark.parametrize("name", sorted(OBSERVED))
def test_capsule_casts_and_overlaps_between_calls_change_nothing(name):
    scene = OBSERVED[name]()
    rng = np.random.default_rng(49)
    casts = _casts(_rays(rng, 4096, (-30, -12, -30), (30, 20, 30), "random"), 0.5, 1.0, _unit_quats(rng, 4096))
    q = np.zeros(1024, dtype=E.OVERLAP_QUERY)
    q["center"] = rng.uniform((-20, -2, -20), (20, 15, 20), size=(1024, 3))
    q["shape"] = E.NH_SHAPE_CAPSULE
    q["size"][:, 0], q["size"][:, 1] = 0.75, 1.5
    q["rotation"] = _unit_quats(rng, 1024)
    q["ignore_body"] = NONE
    # between nh_step calls
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    ct, qt = _upload(a, casts), _upload(a, q)
    ht = a.torch.empty((4096, 32), dtype=a.torch.uint8, device=a.dev)
    ot = a.torch.empty(1025, dtype=a.torch.int32, device=a.dev)
    done = 0
    for k in [1, 2, 3, 5, 7, 4, 8] * 10:
        k = min(k, 300 - done)
        if k <= 0:
            break
        _query(a, ct, ht, qt, ot)
        a.step(k)
        b.step(k)
        done += k
    _query(a, ct, ht, qt, ot)
    _same_stepped_world(a, b, f"{name} nh_step")
    if name == "grid_tiles":
        assert a.counts()["still_steps"] > 0, a.counts()
    a.close(); b.close()
    # between every call of the fused step
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    ct, qt = _upload(a, casts), _upload(a, q)
    ht = a.torch.empty((4096, 32), dtype=a.torch.uint8, device=a.dev)
    ot = a.torch.empty(1025, dtype=a.torch.int32, device=a.dev)
    for s in range(300):
        for call in ("collide", "gravity", "read_cache", "setup", "apply", "update", "write_cache", "advance"):
            _query(a, ct, ht, qt, ot)
            getattr(a, call)()
            getattr(b, call)()
        a.step_done(); b.step_done()
    _query(a, ct, ht, qt, ot)
    _same_stepped_world(a, b, f"{name} call by call")
    if name == "grid_tiles":
        assert a.counts()["still_steps"] > 0, a.counts()
    a.close(); b.close()


# ---- at size -------------------------------------------------------------------------------------------------------------------------------
def test_a_million_capsule_casts_on_the_landed_config_2_world():
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
    n_tiles = len(scene["tile_of_static"])
    w = E.World(scene, flags=FUSED, max_contacts=6 * nb)
    w.step(70)
    assert w.counts()["error"] == 0
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(50)
    n = 1 << 20
    nd = n // 2
    tile = rng.integers(0, n_tiles, size=nd)
    centre = scene["box_transforms"]["position"][tile].astype(np.float64)
    half = scene["box_data"]["size"][tile, 0].astype(np.float64) - 4.0          # (a capsule of extent <= 2.5 stays inside its tile's footprint)
    down = np.zeros(nd, dtype=E.RAY)
    down["origin"][:, 0] = centre[:, 0] + rng.uniform(-1, 1, size=nd) * half
    down["origin"][:, 1] = 20.0
    down["origin"][:, 2] = centre[:, 2] + rng.uniform(-1, 1, size=nd) * half
    down["direction"] = (0.0, -1.0, 0.0)
    down["max_t"] = np.inf
    down["ignore_body"] = NONE
    rays = np.concatenate([down, _rays(rng, n // 4, lo, hi, "random"), _rays(rng, n - nd - n // 4, lo, hi, "axis")])
    rot = _unit_quats(rng, n)
    rot[: n // 4] = (0.0, 0.0, 0.0, 1.0)
    casts = _casts(rays, rng.choice(np.float32([0.25, 0.5, 0.75]), size=n), rng.choice(np.float32([0.0, 0.5, 1.5]), size=n), rot)
    got = _sweep(w, casts)
    g = got[:nd]
    assert (g["shape"] != NONE).all()
    slab = g["body"] == 0
    assert (g["collider"][slab] == tile[slab]).all()
    tob = scene["tile_of_body"]
    assert (tob[g["body"][~slab]] == tile[~slab]).all()
    assert (~slab).mean() > 0.2
    # 1024 casts spread over the batch, bit for bit against the brute force over all 1,004,524 colliders
    pick = np.linspace(0, n - 1, 1024).astype(np.int64)
    _same_hits(got[pick], CAST.cast(CAST.CAPSULE, rec, w.nbox, casts[pick]), "config 2, 1 M capsule casts")
    w.close()
