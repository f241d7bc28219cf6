"""All-hits box and capsule casts on the host (no GPU): nh_boxcast_all / nh_capsulecast_all of include/nudge_hip.h.

The all-hits brute force of tests/hostcast_util.py -- the oracle of the GPU's chain -- is checked here against oracles that share neither its
per-collider decision nor its list handling: the closest-hit brute force beside it (`only=c`), a loop of its own over the closest-hit predicates,
decides the set and every record, the same brute force over all colliders decides the first record, the all-hits ray and sphere lists decide the
degenerate shapes, and a plain Python re-statement decides offsets and the capacity prefix.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostcast_util as CAST                 # noqa: E402
import hostquery_util as Q                   # noqa: E402
from cast_util import (HOST_WORLDS as WORLDS, SENTINEL, as_balls as _as_balls, box_casts, capsule_casts, casts_through,      # noqa: E402
                       check_against_the_single_collider_oracle as _check_against_the_single_collider_oracle, coincident, every_kind_of_ray as _rays,
                       host_world as _world, restated as _restated)
from nudge_amd import engine as E           # noqa: E402


def test_both_entry_points_are_exported_with_their_prototypes():
    assert {"nh_boxcast_all", "nh_capsulecast_all"} <= set(E.EXPORTS)
    declared = open(os.path.join(ROOT, "include", "nudge_hip.h")).read()
    assert "int nh_boxcast_all(" in declared and "int nh_capsulecast_all(" in declared
    so = os.path.join(ROOT, "nudge_amd", "libnudge_hip.so")
    if not os.path.exists(so):
        pytest.fail("nudge_amd/libnudge_hip.so is not built")
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    for name in ("nh_boxcast_all", "nh_capsulecast_all"):
        assert f" T {name}\n" in syms, name
    for name in ("boxcast_all_records", "boxcast_all", "capsulecast_all_records", "capsulecast_all"):
        assert callable(getattr(E.World, name)), name
    src = open(os.path.join(ROOT, "nudge_amd", "engine.py")).read()
    proto = "argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]"
    assert f"L.nh_boxcast_all.{proto}" in src and f"L.nh_capsulecast_all.{proto}" in src


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_all_box_hits_equal_the_existing_single_collider_oracle(name):
    rec, nbox = _world(name)
    rng = np.random.default_rng(500 + sorted(WORLDS).index(name))
    casts = box_casts(rng, _rays(rng, 384, rec))
    got = CAST.cast_all(CAST.BOX, rec, nbox, casts)
    counts = _check_against_the_single_collider_oracle(rec, nbox, casts, got, lambda c: CAST.cast(CAST.BOX, rec, nbox, casts, only=c), CAST.cast(CAST.BOX, rec, nbox, casts),
                                                       f"{name} boxes")
    assert counts.max() >= 4 and (counts == 0).any()
    # start overlaps and zero directions are in the mix, and both list something
    hits = got[1]
    assert (hits["t"] == 0).sum() > 16 and np.isnan(hits["normal"]).any()


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_all_capsule_hits_equal_the_existing_single_collider_oracle(name):
    rec, nbox = _world(name)
    rng = np.random.default_rng(510 + sorted(WORLDS).index(name))
    casts = capsule_casts(rng, _rays(rng, 384, rec))
    got = CAST.cast_all(CAST.CAPSULE, rec, nbox, casts)
    counts = _check_against_the_single_collider_oracle(rec, nbox, casts, got, lambda c: CAST.cast(CAST.CAPSULE, rec, nbox, casts, only=c), CAST.cast(CAST.CAPSULE, rec, nbox, casts),
                                                       f"{name} capsules")
    assert counts.max() >= 4 and (counts == 0).any()
    hits = got[1]
    assert (hits["t"] == 0).sum() > 16 and np.isnan(hits["normal"]).any()


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_degenerate_shapes_write_the_bytes_of_the_simpler_all_hits_call(name):
    rec, nbox = _world(name)
    rng = np.random.default_rng(520 + sorted(WORLDS).index(name))
    rays = _rays(rng, 384, rec)
    rays["origin"][::9, 0] = np.nan                 # (some invalid heads)
    ray_off, ray_hits, total = CAST.cast_all(CAST.RAY, rec, nbox, rays)
    assert total > 384
    # a box of size 0 (and -0), whatever its rotation
    for zero in (0.0, -0.0):
        casts = box_casts(rng, rays, sizes=np.float32([(zero, zero, zero)]), invalid=False)
        casts["rotation"][::3] = np.nan
        off, hits, _ = CAST.cast_all(CAST.BOX, rec, nbox, casts)
        assert off.tobytes() == ray_off.tobytes() and hits.tobytes() == ray_hits.tobytes()
    # a capsule of radius and half height 0
    casts = capsule_casts(rng, rays, shapes=np.float32([(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0)]), invalid=False)
    casts["rotation"][::3] = np.nan
    off, hits, _ = CAST.cast_all(CAST.CAPSULE, rec, nbox, casts)
    assert off.tobytes() == ray_off.tobytes() and hits.tobytes() == ray_hits.tobytes()
    # a capsule of half height 0 is the ball of its radius
    casts = capsule_casts(rng, rays, shapes=np.float32([(0.05, 0.0), (0.75, 0.0), (2.0, -0.0), (0.0, 0.0)]), invalid=False)
    casts["rotation"][::3] = np.nan
    casts["radius"][5::40], casts["radius"][6::40] = np.nan, -1.0
    ball_off, ball_hits, total = CAST.cast_all(CAST.SPHERE, rec, nbox, _as_balls(casts))
    assert total > 384
    off, hits, _ = CAST.cast_all(CAST.CAPSULE, rec, nbox, casts)
    assert off.tobytes() == ball_off.tobytes() and hits.tobytes() == ball_hits.tobytes()


@pytest.mark.parametrize("shape", ["box", "capsule"])
def test_offsets_and_the_capacity_prefix_against_a_plain_restatement(shape):
    rec, nbox = _world("pile")
    rng = np.random.default_rng(530)
    rays = _rays(rng, 96, rec)
    casts = box_casts(rng, rays) if shape == "box" else capsule_casts(rng, rays)
    full_off, full_hits, total = CAST.cast_all(CAST.SHAPES[shape], rec, nbox, casts)
    counts = np.diff(full_off.astype(np.int64))
    assert total > 8 and (counts > 1).any() and (counts == 0).any()
    nz = np.nonzero(counts > 1)[0]
    boundary = int(full_off[nz[len(nz) // 2]])
    for cap in (total, total + 3, total - 1, boundary, boundary + 1, 1, 0):
        hits = np.frombuffer(bytes([SENTINEL]) * 32 * max(cap, 1), dtype=E.RAY_HIT).copy()
        off, hits, t2 = CAST.cast_all(CAST.SHAPES[shape], rec, nbox, casts, capacity=cap, hits=hits)
        ref_off, ref_bytes = _restated(counts, full_hits.tobytes(), cap)
        assert t2 == total and list(off) == ref_off, cap
        assert hits.tobytes() == ref_bytes, cap


def test_sixty_four_coincident_boxes_come_at_one_t_in_index_order():
    scene = coincident(64)
    rec = Q.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    rng = np.random.default_rng(540)
    rays = casts_through((0.25, 3.0, -0.5), 48, rng)
    for shape, casts in ((CAST.BOX, box_casts(rng, rays, invalid=False)), (CAST.CAPSULE, capsule_casts(rng, rays, invalid=False))):
        off, hits, total = CAST.cast_all(shape, rec, nbox, casts)
        assert np.array_equal(off, np.arange(49, dtype=np.uint32) * 64) and total == 48 * 64
        seg = hits.reshape(48, 64)
        assert (seg["t"].copy().view(np.uint32) == seg["t"][:, :1].copy().view(np.uint32)).all()
        assert (seg["collider"] == np.arange(1, 65)).all() and (seg["shape"] == E.NH_SHAPE_BOX).all()
        assert seg[:, 0].tobytes() == CAST.cast(shape, rec, nbox, casts).tobytes()
