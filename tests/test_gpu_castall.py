"""All-hits casts on the GPU (pytest -m gpu): nh_raycast_all / nh_spherecast_all (include/nudge_hip.h, "scene queries").

The oracle is a brute force over every collider on the host with the same arithmetic (nudge_amd/csrc/nh_query.h through tests/hostcast_util.py,
itself checked against the existing single-collider oracles in tests/test_cpu_castall.py).  The answer is defined without reference to the tree --
per cast the colliders it hits in ascending t, ties in ascending combined index, laid out by the exclusive scan of the counts -- so offsets and
records must equal the brute force byte for byte, and so must every byte of `hits` behind the written prefix (a sentinel there stays the sentinel).
The first record of every segment must be the closest-hit call's record on the GPU itself, radius 0 must give the ray bytes, and the calls are
observers: worlds that answer them between every pair of entry points must step exactly like worlds that do not."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostcast_util as CAST                 # noqa: E402
import hostquery_util as Q                   # noqa: E402
from cast_util import (SENTINEL, all_hits as _gpu, far_and_near, first_record_is_the_closest_hit as _first_record_is_the_closest_hit,      # noqa: E402
                       host_all_hits as _host, mixed as _mixed, same_all_hits, spheres as _casts)
import list_util as LU                       # noqa: E402
from query_util import FUSED, NONE, OBSERVED, SMALL, bounds as _bounds, rays as _rays, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

RADII = (0.05, 0.75)


def _same(w, rec, casts, what, capacity=None):
    """cast_util.same_all_hits(); returns the total."""
    return same_all_hits(w, rec, casts, what, capacity)[2]


def _check_world(w, scene, rng, n, what, radii=RADII):
    """Against the tree the world has now (the caller built or refitted it)."""
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    totals = []
    for kind in ("random", "axis", "down", "mixed"):
        rays = _mixed(rng, n, rec, lo, hi) if kind == "mixed" else _rays(rng, n, lo, hi, kind)
        totals.append(_same(w, rec, rays, f"{what} / {kind} rays"))
        for r in radii:
            casts = _casts(rays, r)
            if kind == "mixed":
                casts["radius"][::97], casts["radius"][1::97], casts["radius"][2::97], casts["radius"][3::97] = -0.5, np.nan, np.inf, -0.0
            totals.append(_same(w, rec, casts, f"{what} / {kind} / r {r}"))
        # r = 0 IS A RAY
        a, b = _gpu(w, rays, totals[-1 - len(radii)]), _gpu(w, _casts(rays, 0.0), totals[-1 - len(radii)])
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), f"{what} / {kind}: radius 0 differs from the ray call"
    return totals


@pytest.mark.parametrize("name", sorted(SMALL))
def test_all_hits_equal_the_brute_force_before_and_after_stepping_and_after_a_refit(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(400 + sorted(SMALL).index(name))
    w = E.World(scene, flags=FUSED)
    w.query_build()
    totals = _check_world(w, scene, rng, 4096, f"{name} initial")
    assert max(totals) > 4096, totals
    w.step(50)
    w.query_build()
    state = rng.bit_generator.state
    totals = _check_world(w, scene, rng, 4096, f"{name} after 50 steps")
    assert max(totals) > 4096, totals
    w.close()
    # the same with nh_query_refit in place of the second build: the same casts against the same oracle
    rng.bit_generator.state = state
    w = E.World(scene, flags=FUSED)
    w.query_build()
    w.step(50)
    w.query_refit()
    assert _check_world(w, scene, rng, 4096, f"{name} after 50 steps and a refit") == totals
    w.close()


def test_two_identical_calls_give_identical_bytes():
    scene = SMALL["grid_tiles"]()
    w = E.World(scene, flags=FUSED)
    w.step(20)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    rays = _mixed(np.random.default_rng(41), 16384, rec, lo, hi)
    for casts in (rays, _casts(rays, 0.5)):
        total = _host(rec, w.nbox, casts, 0)[2]
        a, b = _gpu(w, casts, total), _gpu(w, casts, total)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    w.close()


def test_a_single_collider():
    scene = S.pile(4, 0, seed=3)
    w = E.World(scene, flags=FUSED)
    w.set_counts(len(scene["body_transforms"]), 1, 0)          # the ground slab alone (body 0)
    w.query_build()
    totals = _check_world(w, scene, np.random.default_rng(42), 4096, "one collider")
    assert max(totals) > 100
    w.close()


def test_only_spheres_and_only_boxes():
    scene = S.pile(300, 300, seed=3)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    rng = np.random.default_rng(43)
    w.set_counts(nb, 0, 300)
    w.query_build()
    _check_world(w, scene, rng, 4096, "spheres only")
    w.set_counts(nb, 301, 0)
    w.query_build()
    _check_world(w, scene, rng, 4096, "boxes only")
    w.close()


def _coincident(n=4096):
    scene = S.pile(n, 0, seed=3)
    scene["body_transforms"]["position"][1:] = (0.25, 3.0, -0.5)        # every box at one position; the ground slab elsewhere
    return scene


def test_four_thousand_boxes_at_one_position():
    scene = _coincident()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rng = np.random.default_rng(44)
    _check_world(w, scene, rng, 512, "4096 coincident boxes")
    # one ray through all of them at one t: 4096 records in index order
    scene["body_transforms"]["rotation"][1:] = (0.0, 0.0, 0.0, 1.0)
    scene["box_data"]["size"][1:] = scene["box_data"]["size"][1]
    w.close()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene)
    ray = np.zeros(1, dtype=E.RAY)
    ray["origin"], ray["direction"], ray["max_t"], ray["ignore_body"] = (0.25, 3.0, -20.0), (0, 0, 1), np.inf, 0
    for casts in (ray, _casts(ray, 0.75)):
        assert _same(w, rec, casts, "one cast through 4096 coincident boxes") == 4096
        off, hits = _gpu(w, casts, 4096)
        assert list(off) == [0, 4096] and np.array_equal(hits["collider"], np.arange(1, 4097)) and len(np.unique(hits["t"])) == 1
    w.close()


def test_a_scene_spanning_a_thousandth_and_ten_thousand_units():
    scene = S.pile(2000, 1000, seed=3)
    rng = np.random.default_rng(45)
    far_and_near(scene, rng)
    w = E.World(scene, flags=FUSED)
    w.query_build()
    _check_world(w, scene, rng, 4096, "1e-3 .. 1e4", radii=(1e-4, 5.0, 100.0))
    rec = Q.records(w.get_bodies()["transforms"], scene)
    rays = _rays(rng, 4096, (-0.05,) * 3, (0.05,) * 3, "random")
    _same(w, rec, rays, "small cluster rays")
    for r in (1e-4, 0.01):
        _same(w, rec, _casts(rays, r), f"small cluster r {r}")
    w.close()


# ---- capacity -------------------------------------------------------------------------------------------------------------------------------
def test_capacity_writes_whole_segments_and_nothing_behind_them():
    scene = SMALL["pile"]()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    rays = _mixed(np.random.default_rng(46), 2048, rec, lo, hi)
    for casts in (rays, _casts(rays, 0.5)):
        ref_off, _, total = _host(rec, w.nbox, casts, 0)
        nz = np.nonzero(np.diff(ref_off.astype(np.int64)) > 1)[0]
        boundary = int(ref_off[nz[len(nz) // 2]])                  # the start of a segment of at least two records
        for cap in (total, total + 7, total - 1, boundary, boundary + 1, 1, 0):
            _same(w, rec, casts, f"capacity {cap} of {total}", capacity=cap)
        # capacity 0 with a non-null hits buffer: count only, the buffer untouched
        off, hits = _gpu(w, casts, 0)
        assert off.tobytes() == ref_off.tobytes() and set(hits.tobytes()) == {SENTINEL}
    w.close()


def test_one_ray_along_a_row_of_a_4096_collider_world_and_a_million_rays_around_it():
    n = 4096
    scene = S.pile(n, 0, seed=3)
    k = np.arange(n)
    pos = np.stack([1.5 * (k % 512), 3.0 + 4.0 * (k // 512), np.zeros(n)], axis=1).astype(np.float32)      # 8 rows of 512 boxes along x
    scene["body_transforms"]["position"][1:] = pos
    scene["body_transforms"]["rotation"][1:] = (0.0, 0.0, 0.0, 1.0)
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene)
    ray = np.zeros(1, dtype=E.RAY)
    ray["origin"], ray["direction"], ray["max_t"], ray["ignore_body"] = (-10.0, 3.0, 0.0), (1, 0, 0), np.inf, NONE
    for casts in (ray, _casts(ray, 0.25)):
        total = _same(w, rec, casts, "one cast along a row")
        assert total >= 512
        off, hits = _gpu(w, casts, total)
        assert (np.diff(hits["t"]) >= 0).all() and (hits["shape"] == E.NH_SHAPE_BOX).all()
    r = w.raycast_all(ray["origin"], ray["direction"], synchronize=True)
    assert int(r["written"]) == int(r["offsets"][-1]) >= 512
    assert (r["query"] == 0).all() and (np.diff(r["t"].cpu().numpy()) >= 0).all()
    s = w.spherecast_all(ray["origin"], ray["direction"], 0.25, capacity=100, synchronize=True)
    assert int(s["written"]) == 0 and int(s["offsets"][-1]) >= 512
    # 2^20 rays on the 4097 colliders: more than 64 key bits (21 + 32 + 13), the chain's two-sort ordering
    rng = np.random.default_rng(47)
    m = 1 << 20
    rays = np.zeros(m, dtype=E.RAY)
    rays["ignore_body"], rays["max_t"] = NONE, np.inf
    rays["origin"] = np.stack([rng.uniform(-20, 800, size=m), rng.uniform(0, 36, size=m), rng.uniform(-2, 2, size=m)], axis=1)
    d = np.zeros((m, 3))
    d[:, 0] = rng.choice([-1.0, 1.0], size=m)
    d[:, 1] = rng.normal(scale=0.02, size=m)
    rays["direction"] = d
    rays["origin"][::256, 1] = 3.0 + 4.0 * rng.integers(0, 8, size=len(rays[::256]))       # some of them exactly along a row: segments of hundreds
    rays["direction"][::256, 1] = 0.0
    rays["max_t"][1::2] = rng.uniform(0, 60, size=m // 2)
    cnt, _ = _gpu(w, rays, None)
    ref_cnt, _, total = CAST.cast_all(CAST.RAY, rec, w.nbox, rays, capacity=0)
    assert cnt.tobytes() == ref_cnt.tobytes() and m // 8 < total < NONE
    off, hits = _gpu(w, rays, total)
    assert off.tobytes() == cnt.tobytes()
    _first_record_is_the_closest_hit(w, rays, off, hits, "2^20 rays on 4097 colliders")
    pick = np.unique(np.concatenate([np.linspace(0, m - 1, 2048).astype(np.int64), np.argsort(np.diff(off.astype(np.int64)))[-64:]]))
    ref_off, ref_hits, ref_total = CAST.cast_all(CAST.RAY, rec, w.nbox, rays[pick])
    assert np.array_equal(np.diff(ref_off.astype(np.int64)), np.diff(off.astype(np.int64))[pick])
    seg = np.concatenate([hits[off[i]:off[i + 1]] for i in pick])
    assert seg.tobytes() == ref_hits[:ref_total].tobytes()
    w.close()


def test_a_total_of_two_to_the_thirty_second_writes_the_marker_and_no_record():
    scene = _coincident()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene)
    rays = np.zeros(1 << 20, dtype=E.RAY)
    rays["origin"], rays["direction"], rays["max_t"], rays["ignore_body"] = (0.25, 3.0, -0.5), (0, 0, 1), np.inf, 0
    assert CAST.cast_all(CAST.RAY, rec, w.nbox, rays[:1], capacity=0)[2] == 4096          # so 2^20 of them make exactly 2^32: the 32-bit scan wraps to 0
    for casts in (rays, _casts(rays, 0.5)):
        cnt, _ = _gpu(w, casts, None)
        assert cnt[-1] == NONE
        off, hits = _gpu(w, casts, 1 << 16)
        assert off[-1] == NONE and set(hits.tobytes()) == {SENTINEL}
        # 2^20 - 1 casts: 2^32 - 4096 records, no wrap, the prefix rule applies
        cnt, _ = _gpu(w, casts[1:], None)
        assert int(cnt[-1]) == (1 << 32) - 4096 and (np.diff(cnt.astype(np.int64)) == 4096).all()
        off, hits = _gpu(w, casts[1:], 8192)
        assert off.tobytes() == cnt.tobytes()
        ref = _host(rec, w.nbox, casts[1:3], 8192)[1]
        assert hits.tobytes() == ref.tobytes()
    r = w.raycast_all(rays["origin"], rays["direction"], ignore_body=0, capacity=1000, synchronize=True)
    assert int(r["offsets"][-1]) == NONE and int(r["written"]) == 0
    w.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["nh_raycast_all", "nh_spherecast_all"])
def test_abi_edge_cases(entry):
    import torch
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    fn = getattr(w.L, entry)
    rec = Q.records(w.get_bodies()["transforms"], scene)
    lo, hi = _bounds(rec)
    casts = _mixed(np.random.default_rng(48), 1024, rec, lo, hi)
    if entry == "nh_spherecast_all":
        casts = _casts(casts, 0.5)
    ct = _upload(w, casts)
    buf = torch.zeros(4 * 1032, dtype=torch.int32, device=w.dev)
    ot = buf[:1025]
    cap = 16384
    ht = torch.zeros((cap, 32), dtype=torch.uint8, device=w.dev)
    cp, op, hp = C.c_void_p(ct.data_ptr()), C.c_void_p(ot.data_ptr()), C.c_void_p(ht.data_ptr())
    assert fn(w.ctx, cp, 1024, op, hp, cap, 0) == 1                    # before any build: NH_ERR_INVALID
    assert fn(None, cp, 1024, op, hp, cap, 0) == 1
    w.query_build()
    assert fn(w.ctx, cp, 1024, op, hp, cap, E.NH_RAY_ANY_HIT) == 1     # flags: NH_RAY_ANY_HIT has no meaning here
    assert fn(w.ctx, cp, 1024, op, hp, cap, 2) == 1
    assert fn(w.ctx, None, 1024, op, hp, cap, 0) == 1                  # null / unaligned casts
    assert fn(w.ctx, C.c_void_p(ct.data_ptr() + 4), 1023, op, hp, cap, 0) == 1
    assert fn(w.ctx, cp, 1024, None, hp, cap, 0) == 1                  # null / unaligned offsets
    assert fn(w.ctx, cp, 1024, C.c_void_p(ot.data_ptr() + 2), hp, cap, 0) == 1
    assert fn(w.ctx, cp, 1024, op, None, cap, 0) == 1                  # null hits with a capacity, unaligned hits
    assert fn(w.ctx, cp, 1024, op, C.c_void_p(ht.data_ptr() + 8), cap - 1, 0) == 1
    assert fn(w.ctx, cp, 1 << 30, op, hp, cap, 0) == 1                 # count >= 2^30: refused on the host, nothing launched
    assert fn(w.ctx, cp, 0xFFFFFFFF, op, hp, cap, 0) == 1
    assert fn(w.ctx, cp, 0, op, hp, cap, 0) == 0                       # count 0: a no-op
    assert fn(w.ctx, None, 0, None, None, 0, 0) == 0
    w.torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0 and int(ht.sum()) == 0            # nothing was written
    # offsets need 4-byte alignment only
    ot4 = buf[1:1026]
    assert fn(w.ctx, cp, 1024, C.c_void_p(ot4.data_ptr()), hp, cap, 0) == 0
    ref_off, ref_hits, total = CAST.cast_all(CAST.shape_of(casts), rec, w.nbox, casts, capacity=cap)
    assert 0 < total <= cap
    assert ot4.cpu().numpy().view(np.uint32).tobytes() == ref_off.tobytes()
    got = np.frombuffer(ht.cpu().numpy().tobytes(), dtype=E.RAY_HIT)
    assert got[:total].tobytes() == ref_hits[:total].tobytes() and not got[total:].view(np.uint8).any()
    w.close()


# ---- observers -----------------------------------------------------------------------------------------------------------------------------
def _query(w, rt, ct, ot, ht):
    w.query_build()
    w.raycast_all_records(rt, offsets=ot)
    w.raycast_all_records(rt, offsets=ot, hits=ht, capacity=ht.shape[0])
    w.spherecast_all_records(ct, offsets=ot)
    w.spherecast_all_records(ct, offsets=ot, hits=ht, capacity=ht.shape[0])


def _observer_batch(a):
    import torch
    rays = _rays(np.random.default_rng(49), 4096, (-30, -12, -30), (30, 20, 30), "random")
    rt, ct = _upload(a, rays), _upload(a, _casts(rays, 0.5))
    ot = torch.empty(4097, dtype=torch.int32, device=a.dev)
    ht = torch.empty((16384, 32), dtype=torch.uint8, device=a.dev)
    return rt, ct, ot, ht


@pytest.mark.parametrize("name", sorted(OBSERVED))
def test_all_hits_casts_between_nh_step_calls_change_nothing(name):
    LU.queries_between_nh_step_calls_change_nothing(OBSERVED[name], lambda a, scene: _observer_batch(a), _query, name, still=name == "grid_tiles")


@pytest.mark.parametrize("name", sorted(OBSERVED))
def test_all_hits_casts_between_every_call_of_the_fused_step_change_nothing(name):
    LU.queries_between_every_call_of_the_fused_step_change_nothing(OBSERVED[name], lambda a, scene: _observer_batch(a), _query, name, still=name == "grid_tiles")


# ---- at size -------------------------------------------------------------------------------------------------------------------------------
def test_a_million_rays_on_the_landed_config_2_world():
    import torch
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED, max_contacts=6 * nb)
    w.step(70)
    assert w.counts()["error"] == 0
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene)
    assert len(rec) == 1004524
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(50)
    n = 1 << 20
    rays = np.concatenate([_rays(rng, n // 2, lo, hi, "down"), _rays(rng, n // 4, lo, hi, "random"), _rays(rng, n // 4, lo, hi, "axis")])
    rays["max_t"][1::4] = rng.uniform(0.0, 100.0, size=len(rays[1::4]))
    rt = _upload(w, rays)
    ot = torch.full((n + 1,), -1, dtype=torch.int32, device=w.dev)
    w.raycast_all_records(rt, offsets=ot)
    cnt = ot.cpu().numpy().view(np.uint32).copy()
    total = int(cnt[-1])
    assert n // 2 <= total < NONE
    ht = torch.full((total, 32), SENTINEL, dtype=torch.uint8, device=w.dev)
    w.raycast_all_records(rt, offsets=ot, hits=ht, capacity=total)
    off = ot.cpu().numpy().view(np.uint32).copy()
    # offsets complete and monotone, the total = offsets[count]
    assert off.tobytes() == cnt.tobytes() and off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all()
    # the first-record contract for all of them, on the device
    best = w.raycast_records(rt)
    o64 = torch.from_numpy(off.astype(np.int64)).to(w.dev)
    full = o64[1:] > o64[:-1]
    shape = best.view(torch.int32).reshape(n, 8)[:, 6]
    assert bool((shape[~full] == -1).all()), "empty segments where nh_raycast hits"
    assert bool((shape[full] != -1).all()), "nonempty segments where nh_raycast misses"
    assert bool((ht[o64[:-1][full]] == best[full]).all()), "first records differ from nh_raycast's"
    # t ascending within every segment, on the device
    t = ht.view(torch.float32).reshape(total, 8)[:, 0]
    inner = torch.ones(total, dtype=torch.bool, device=w.dev)
    inner[o64[:-1][full]] = False
    assert bool((t[1:] >= t[:-1])[inner[1:]].all())
    # a seeded sample of 2048 rays, byte for byte against the brute force over all 1,004,524 colliders
    pick = np.sort(rng.choice(n, size=2048, replace=False))
    ref_off, ref_hits, ref_total = CAST.cast_all(CAST.RAY, rec, w.nbox, rays[pick])
    assert np.array_equal(np.diff(ref_off.astype(np.int64)), np.diff(off.astype(np.int64))[pick])
    idx = np.concatenate([np.arange(off[i], off[i + 1], dtype=np.int64) for i in pick])
    seg = np.frombuffer(ht[torch.from_numpy(idx).to(w.dev)].cpu().numpy().tobytes(), dtype=E.RAY_HIT)
    assert ref_total == len(seg) and seg.tobytes() == ref_hits[:ref_total].tobytes()
    w.close()
