"""All-hits box and capsule casts on the GPU (pytest -m gpu): nh_boxcast_all / nh_capsulecast_all (include/nudge_hip.h, "scene queries").

The oracle is a brute force over every collider on the host with the same arithmetic (nudge_amd/csrc/nh_query.h through
tests/hostcast_util.py, itself checked against the existing single-collider oracles in tests/test_cpu_castall_shapes.py).  The answer is
defined without reference to the tree, so offsets and records must equal the brute force byte for byte, and so must every byte of `hits` behind the
written prefix.  The first record of every segment must be the closest-hit call's record on the GPU itself, the degenerate shapes must give the GPU's
own nh_raycast_all / nh_spherecast_all bytes, and the calls are observers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostcast_util as CAST                 # noqa: E402
import hostquery_util as Q                   # noqa: E402
from cast_util import (SENTINEL, all_hits as _gpu, as_balls as _as_balls, box_casts, capsule_casts, casts_through, coincident,      # noqa: E402
                       far_and_near_scene as _far_and_near_scene, host_all_hits as _host, mixed as _mixed, same_all_hits)
import list_util as LU                       # noqa: E402
from query_util import FUSED, OBSERVED, SMALL, bounds as _bounds, rays as _rays, records as _records, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = ("box", "capsule")


def _same(w, rec, casts, what, capacity=None):
    """cast_util.same_all_hits(); returns (offsets, hits)."""
    return same_all_hits(w, rec, casts, what, capacity)[:2]


def _batches(rng, n, rec):
    """One batch of box casts and one of capsule casts on mixed rays: sizes from 0 to several bodies, identity and random rotations, finite and infinite
    max_t, ignore_body, start overlaps, zero directions, invalid records."""
    lo, hi = _bounds(rec)
    return box_casts(rng, _mixed(rng, n, rec, lo, hi)), capsule_casts(rng, _mixed(rng, n, rec, lo, hi))


def _check_world(w, scene, rng, n, what, least=None):
    """Against the tree the world has now (the caller built or refitted it); returns every byte the GPU wrote.  `least`: the records a batch must
    list at least (n / 2 unless given), so that no comparison is one of empty lists."""
    rec = _records(w, scene)
    out = []
    for casts in _batches(rng, n, rec):
        off, hits = _same(w, rec, casts, f"{what} / {CAST.shape_of(casts).name} casts")
        assert int(off[-1]) > (n // 2 if least is None else least), (what, int(off[-1]))
        out += [off.tobytes(), hits.tobytes()]
    return out


@pytest.mark.parametrize("name", sorted(SMALL))
def test_all_hits_equal_the_brute_force_before_and_after_stepping_and_after_a_refit(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(600 + sorted(SMALL).index(name))
    w = E.World(scene, flags=FUSED)
    w.query_build()
    _check_world(w, scene, rng, 384, f"{name} initial")
    w.step(50)
    w.query_build()
    state = rng.bit_generator.state
    built = _check_world(w, scene, rng, 384, f"{name} after 50 steps")
    w.close()
    # the same with nh_query_refit in place of the second build: the same casts against the same oracle, and the build's bytes
    rng.bit_generator.state = state
    w = E.World(scene, flags=FUSED)
    w.query_build()
    w.step(50)
    w.query_refit()
    assert _check_world(w, scene, rng, 384, f"{name} after 50 steps and a refit") == built
    w.close()


@pytest.mark.parametrize("world", ["pile", "far_and_near"])
def test_degenerate_shapes_write_the_bytes_of_the_simpler_all_hits_call_on_the_gpu(world):
    scene = SMALL["pile"]() if world == "pile" else _far_and_near_scene()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(62)
    # (rays from all over a world of 1e-3 .. 1e4 units graze far colliders: what the ray pad of the walk is for; and rays inside the small cluster)
    rays = np.concatenate([_mixed(rng, 512, rec, lo, hi), _rays(rng, 256, (-0.05,) * 3, (0.05,) * 3, "random")])
    cap = 1 << 16
    ray_off, ray_hits = _gpu(w, rays, cap)
    assert 128 < int(ray_off[-1]) <= cap
    # a box of size 0, whatever its rotation
    casts = box_casts(rng, rays, sizes=np.float32([(0, 0, 0), (-0.0, 0.0, -0.0)]), invalid=False)
    casts["rotation"][::3] = np.nan
    off, hits = _gpu(w, casts, cap)
    assert off.tobytes() == ray_off.tobytes() and hits.tobytes() == ray_hits.tobytes(), "size 0 differs from nh_raycast_all"
    _same(w, rec, casts, f"{world} size 0")
    # a capsule of radius 0 and half height 0
    casts = capsule_casts(rng, rays, shapes=np.float32([(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0)]), invalid=False)
    casts["rotation"][::3] = np.nan
    off, hits = _gpu(w, casts, cap)
    assert off.tobytes() == ray_off.tobytes() and hits.tobytes() == ray_hits.tobytes(), "r = hh = 0 differs from nh_raycast_all"
    # a capsule of half height 0 is the ball of its radius (0 among the radii: the ball that is a ray)
    radii = (1e-4, 0.05, 0.75, 0.0) if world == "pile" else (1e-4, 5.0, 100.0, 0.0)
    casts = capsule_casts(rng, rays, shapes=np.float32([(r, 0.0) for r in radii]), invalid=False)
    casts["rotation"][::3] = np.nan
    casts["radius"][5::40], casts["radius"][6::40] = np.nan, -1.0
    cap = 1 << 18
    ball_off, ball_hits = _gpu(w, _as_balls(casts), cap)
    assert 256 < int(ball_off[-1]) <= cap
    off, hits = _gpu(w, casts, cap)
    assert off.tobytes() == ball_off.tobytes() and hits.tobytes() == ball_hits.tobytes(), "hh = 0 differs from nh_spherecast_all"
    _same(w, rec, casts, f"{world} hh 0")
    w.close()


def test_two_identical_calls_give_identical_bytes():
    scene = SMALL["grid_tiles"]()
    w = E.World(scene, flags=FUSED)
    w.step(20)
    w.query_build()
    rec = _records(w, scene)
    for casts in _batches(np.random.default_rng(63), 512, rec):
        total = _host(rec, w.nbox, casts, 0)[2]
        a, b = _gpu(w, casts, total), _gpu(w, casts, total)
        assert total > 256 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    w.close()


def test_tiny_worlds():
    scene = S.pile(300, 300, seed=3)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    rng = np.random.default_rng(64)
    w.set_counts(nb, 0, 0)                       # no collider at all: NH_OK, every offset 0, no record
    w.query_build()
    rays = _rays(rng, 256, (-5,) * 3, (5,) * 3, "random")
    for casts in (box_casts(rng, rays), capsule_casts(rng, rays)):
        off, hits = _gpu(w, casts, 16)
        assert not off.any() and (hits.view(np.uint8) == SENTINEL).all()
    w.set_counts(nb, 1, 0)                       # the ground slab alone (body 0)
    w.query_build()
    _check_world(w, scene, rng, 256, "one collider", least=16)
    w.set_counts(nb, 0, 300)
    w.query_build()
    _check_world(w, scene, rng, 256, "spheres only")
    w.set_counts(nb, 301, 0)
    w.query_build()
    _check_world(w, scene, rng, 256, "boxes only")
    w.close()


def test_sixty_four_casts_through_four_thousand_coincident_boxes():
    scene = coincident(4096)
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene)
    rng = np.random.default_rng(65)
    rays = casts_through((0.25, 3.0, -0.5), 64, rng)
    for casts in (box_casts(rng, rays, invalid=False), capsule_casts(rng, rays, invalid=False)):
        off, hits = _same(w, rec, casts, "64 casts through 4096 coincident boxes")
        assert np.array_equal(off, np.arange(65, dtype=np.uint32) * 4096)
        seg = hits.reshape(64, 4096)
        assert (seg["collider"] == np.arange(1, 4097)).all() and (seg["shape"] == E.NH_SHAPE_BOX).all()
        assert (seg["t"].copy().view(np.uint32) == seg["t"][:, :1].copy().view(np.uint32)).all()
    w.close()


def test_capacity_writes_whole_segments_and_nothing_behind_them():
    scene = SMALL["pile"]()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    for casts in _batches(np.random.default_rng(66), 384, rec):
        ref_off, _, total = _host(rec, w.nbox, casts, 0)
        nz = np.nonzero(np.diff(ref_off.astype(np.int64)) > 1)[0]
        boundary = int(ref_off[nz[len(nz) // 2]])                  # the start of a segment of at least two records
        assert 0 < boundary < total
        for cap in (total + 7, total - 1, boundary, boundary + 1, 1):
            _same(w, rec, casts, f"capacity {cap} of {total}", capacity=cap)
        # COUNT ONLY writes offsets alone; so does capacity 0 with a non-null hits buffer
        off, _ = _gpu(w, casts, None)
        assert off.tobytes() == ref_off.tobytes()
        off, hits = _gpu(w, casts, 0)
        assert off.tobytes() == ref_off.tobytes() and set(hits.tobytes()) == {SENTINEL}
    w.close()


def _bits(x):
    return int(x).bit_length()


@pytest.mark.parametrize("shape", SHAPES)
def test_a_million_casts_on_4097_colliders_take_the_two_sort_ordering(shape):
    scene = S.pile(4096, 0, seed=3)
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene)
    m = 1 << 20
    assert len(rec) == 4097 and _bits(m) + 32 + _bits(len(rec)) > 64          # nh_castall's arithmetic: one sort needs ibits + 32 + cbits <= 64
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(67)
    valid = np.linspace(0, m - 1, 64).astype(np.int64)                          # spread over the index range, the last index included
    assert valid[-1] == m - 1
    rays = _rays(rng, 64, lo, hi, "random")
    some = box_casts(rng, rays, invalid=False) if shape == "box" else capsule_casts(rng, rays, invalid=False)
    casts = np.zeros(m, dtype=some.dtype)
    casts["origin"] = np.nan                                                    # invalid: count 0, and free on the host
    casts[valid] = some
    off, hits = _same(w, rec, casts, f"2^20 {shape} casts, 64 of them valid")
    cnt = np.diff(off.astype(np.int64))
    assert int(off[-1]) > 256 and not cnt[np.setdiff1d(np.arange(m), valid)].any()
    assert (cnt[valid] > 1).sum() > 16
    w.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["nh_boxcast_all", "nh_capsulecast_all"])
def test_abi_edge_cases(entry):
    import torch
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    fn = getattr(w.L, entry)
    rec = Q.records(w.get_bodies()["transforms"], scene)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(68)
    rays = _mixed(rng, 256, rec, lo, hi)
    casts = box_casts(rng, rays) if entry == "nh_boxcast_all" else capsule_casts(rng, rays)
    ct = _upload(w, casts)
    buf = torch.zeros(4 * 264, dtype=torch.int32, device=w.dev)
    ot = buf[:257]
    cap = 16384
    ht = torch.zeros((cap, 32), dtype=torch.uint8, device=w.dev)
    cp, op, hp = C.c_void_p(ct.data_ptr()), C.c_void_p(ot.data_ptr()), C.c_void_p(ht.data_ptr())
    assert fn(w.ctx, cp, 256, op, hp, cap, 0) == 1                     # before any build: NH_ERR_INVALID
    assert fn(None, cp, 256, op, hp, cap, 0) == 1
    w.query_build()
    assert fn(w.ctx, cp, 256, op, hp, cap, E.NH_RAY_ANY_HIT) == 1      # flags = 1: NH_RAY_ANY_HIT has no meaning here
    assert fn(w.ctx, cp, 256, op, hp, cap, 2) == 1
    assert fn(w.ctx, None, 256, op, hp, cap, 0) == 1                   # null / misaligned casts
    assert fn(w.ctx, C.c_void_p(ct.data_ptr() + 4), 255, op, hp, cap, 0) == 1
    assert fn(w.ctx, cp, 256, None, hp, cap, 0) == 1                   # null / misaligned offsets
    assert fn(w.ctx, cp, 256, C.c_void_p(ot.data_ptr() + 2), hp, cap, 0) == 1
    assert fn(w.ctx, cp, 256, op, None, cap, 0) == 1                   # null hits with a capacity, misaligned hits
    assert fn(w.ctx, cp, 256, op, C.c_void_p(ht.data_ptr() + 8), cap - 1, 0) == 1
    assert fn(w.ctx, cp, 1 << 30, op, hp, cap, 0) == 1                 # count >= 2^30: refused on the host, nothing launched
    assert fn(w.ctx, cp, 0xFFFFFFFF, op, hp, cap, 0) == 1
    assert fn(w.ctx, cp, 0, op, hp, cap, 0) == 0                       # count 0: a no-op
    assert fn(w.ctx, None, 0, None, None, 0, 0) == 0
    w.torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0 and int(ht.sum()) == 0            # nothing was written
    # offsets need 4-byte alignment only
    ot4 = buf[1:258]
    assert fn(w.ctx, cp, 256, C.c_void_p(ot4.data_ptr()), hp, cap, 0) == 0
    ref_off, ref_hits, total = CAST.cast_all(CAST.shape_of(casts), rec, w.nbox, casts, capacity=cap)
    assert 0 < total <= cap
    assert ot4.cpu().numpy().view(np.uint32).tobytes() == ref_off.tobytes()
    got = np.frombuffer(ht.cpu().numpy().tobytes(), dtype=E.RAY_HIT)
    assert got[:total].tobytes() == ref_hits[:total].tobytes() and not got[total:].view(np.uint8).any()
    w.close()


def test_the_python_wrappers_write_the_records_they_describe():
    scene = SMALL["pile"]()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    rng = np.random.default_rng(69)
    box, cap = _batches(rng, 256, rec)
    for casts, r in ((box, w.boxcast_all(box["origin"], box["direction"], box["size"], box["rotation"], max_t=box["max_t"],
                                         ignore_body=box["ignore_body"].astype(np.int64), synchronize=True)),
                     (cap, w.capsulecast_all(cap["origin"], cap["direction"], cap["radius"], cap["half_height"], cap["rotation"], max_t=cap["max_t"],
                                             ignore_body=cap["ignore_body"].astype(np.int64), synchronize=True))):
        ref_off, ref_hits, total = CAST.cast_all(CAST.shape_of(casts), rec, w.nbox, casts)
        assert int(r["written"]) == total == int(r["offsets"][-1]) and np.array_equal(r["offsets"].cpu().numpy(), ref_off.astype(np.int64))
        assert r["raw"].cpu().numpy().tobytes()[:32 * total] == ref_hits[:total].tobytes()
    # a capacity that cuts the list: nothing waits, whole segments only
    r = w.boxcast_all(box["origin"], box["direction"], box["size"], box["rotation"], max_t=box["max_t"], ignore_body=box["ignore_body"].astype(np.int64),
                      capacity=total // 2, synchronize=True)
    assert 0 < int(r["written"]) <= total // 2
    w.close()


# ---- observers -----------------------------------------------------------------------------------------------------------------------------
def _query(w, bt, kt, ot, ht):
    w.query_build()
    w.boxcast_all_records(bt, offsets=ot)
    w.boxcast_all_records(bt, offsets=ot, hits=ht, capacity=ht.shape[0])
    w.capsulecast_all_records(kt, offsets=ot)
    w.capsulecast_all_records(kt, offsets=ot, hits=ht, capacity=ht.shape[0])


def _observer_batch(a):
    import torch
    rng = np.random.default_rng(70)
    rays = _rays(rng, 256, (-30, -12, -30), (30, 20, 30), "random")
    bt, kt = _upload(a, box_casts(rng, rays)), _upload(a, capsule_casts(rng, rays))
    ot = torch.empty(257, dtype=torch.int32, device=a.dev)
    ht = torch.empty((8192, 32), dtype=torch.uint8, device=a.dev)
    return bt, kt, ot, ht


# (the still counters of the two worlds agree with all their other counts: same_stepped_world compares every one)
def test_all_hits_casts_between_nh_step_calls_change_nothing():
    LU.queries_between_nh_step_calls_change_nothing(OBSERVED["grid_tiles"], lambda a, scene: _observer_batch(a), _query, "grid_tiles", still=True)


def test_all_hits_casts_between_every_call_of_the_fused_step_change_nothing():
    LU.queries_between_every_call_of_the_fused_step_change_nothing(OBSERVED["grid_tiles"], lambda a, scene: _observer_batch(a), _query, "grid_tiles", still=True)
