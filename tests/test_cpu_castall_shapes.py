"""All-hits box and capsule casts on the host (no GPU): nh_boxcast_all / nh_capsulecast_all of include/nudge_hip.h.

The brute force of tests/hostcastall_shapes_util.py -- the oracle of the GPU's chain -- is checked here against oracles that share no code with the
feature: the EXISTING single-collider answers of tests/hostboxcast_util.py and tests/hostcapsule_util.py (`only=c`) decide the set and every record,
the existing closest-hit brute force decides the first record, the existing all-hits ray and sphere oracle decides the degenerate shapes, and a
plain Python re-statement decides offsets and the capacity prefix.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostboxcast_util as B                 # noqa: E402
import hostcapsule_util as K                 # noqa: E402
import hostcastall_shapes_util as A          # noqa: E402
import hostcastall_util as R                 # noqa: E402
import hostquery_util as Q                   # noqa: E402
from query_util import unit_quats            # noqa: E402
from test_cpu_castall import SENTINEL, _check_against_the_single_collider_oracle, _rays, _restated      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

NONE = 0xFFFFFFFF
IDENTITY = (0.0, 0.0, 0.0, 1.0)
WORLDS = {"pile": lambda: S.pile(200, 100, seed=11), "compound": lambda: S.compound(100, seed=12)}      # a few hundred mixed boxes and spheres
BOX_SIZES = np.float32([(0, 0, 0), (0.05, 0.05, 0.05), (0.5, 0.3, 0.2), (0.75, 0.75, 0.75), (3.0, 0.4, 2.0), (0.0, 0.6, 0.0)])      # up to several bodies across
CAPSULES = np.float32([(0, 0), (0.05, 0.5), (0.5, 0.5), (0.5, 0.0), (0.0, 1.0), (1.5, 2.5)])                                         # (radius, half height)


def _head(rays, dtype):
    c = np.zeros(len(rays), dtype=dtype)
    for k in ("origin", "max_t", "direction", "ignore_body"):
        c[k] = rays[k]
    c["rotation"] = IDENTITY
    return c


def box_casts(rng, rays, sizes=BOX_SIZES, invalid=True):
    """nh_BoxCast records on the rays' heads: the sizes in turn, every other rotation random, and a few invalid records."""
    n = len(rays)
    c = _head(rays, E.BOX_CAST)
    c["size"] = sizes[np.arange(n) % len(sizes)]
    turn = (np.arange(n) // len(sizes)) % 2 == 1
    c["rotation"][turn] = unit_quats(rng, int(turn.sum()))
    if invalid:
        bad = rng.choice(n, size=8, replace=False)
        c["size"][bad] = (0.5, 0.5, 0.5)
        c["origin"][bad[0], 2] = np.nan
        c["direction"][bad[1], 0] = np.inf
        c["size"][bad[2], 1] = -0.25
        c["size"][bad[3], 0] = np.nan
        c["size"][bad[4], 2] = np.inf
        c["rotation"][bad[5], 3] = np.nan
        c["max_t"][bad[6]] = np.nan
        c["rotation"][bad[7]] = np.nan              # ... which a size of 0 does not read: this one is a valid ray
        c["size"][bad[7]] = 0.0
    return c


def capsule_casts(rng, rays, shapes=CAPSULES, invalid=True):
    """nh_CapsuleCast records on the rays' heads: (radius, half height) in turn, every other rotation random, and a few invalid records."""
    n = len(rays)
    c = _head(rays, E.CAPSULE_CAST)
    s = shapes[np.arange(n) % len(shapes)]
    c["radius"], c["half_height"] = s[:, 0], s[:, 1]
    turn = (np.arange(n) // len(shapes)) % 2 == 1
    c["rotation"][turn] = unit_quats(rng, int(turn.sum()))
    if invalid:
        bad = rng.choice(n, size=8, replace=False)
        c["radius"][bad], c["half_height"][bad] = 0.5, 0.5
        c["origin"][bad[0], 1] = np.inf
        c["direction"][bad[1], 2] = np.nan
        c["radius"][bad[2]] = -0.5
        c["half_height"][bad[3]] = -1.0
        c["radius"][bad[4]] = np.nan
        c["rotation"][bad[5], 0] = np.inf
        c["max_t"][bad[6]] = np.nan
        c["rotation"][bad[7]] = np.nan              # ... which a half height of 0 does not read: this one is a valid ball
        c["half_height"][bad[7]] = 0.0
    return c


def _world(name):
    scene = WORLDS[name]()
    rec = Q.records(scene["body_transforms"], scene)
    return rec, len(scene["box_tags"])


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
    got = A.boxcast_all(rec, nbox, casts)
    counts = _check_against_the_single_collider_oracle(rec, nbox, casts, got, lambda c: B.boxcast(rec, nbox, casts, only=c), B.boxcast(rec, nbox, casts),
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
    got = A.capsulecast_all(rec, nbox, casts)
    counts = _check_against_the_single_collider_oracle(rec, nbox, casts, got, lambda c: K.capsulecast(rec, nbox, casts, only=c), K.capsulecast(rec, nbox, casts),
                                                       f"{name} capsules")
    assert counts.max() >= 4 and (counts == 0).any()
    hits = got[1]
    assert (hits["t"] == 0).sum() > 16 and np.isnan(hits["normal"]).any()


def _as_rays(casts):
    return np.ascontiguousarray(casts).view(np.uint8).reshape(len(casts), 64)[:, :32].copy().view(E.RAY).reshape(len(casts))


def _as_balls(casts):
    b = np.zeros(len(casts), dtype=E.SPHERE_CAST)
    for k in ("origin", "max_t", "direction", "ignore_body", "radius"):
        b[k] = casts[k]
    return b


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_degenerate_shapes_write_the_bytes_of_the_simpler_all_hits_call(name):
    rec, nbox = _world(name)
    rng = np.random.default_rng(520 + sorted(WORLDS).index(name))
    rays = _rays(rng, 384, rec)
    rays["origin"][::9, 0] = np.nan                 # (some invalid heads)
    ray_off, ray_hits, total = R.raycast_all(rec, nbox, rays)
    assert total > 384
    # a box of size 0 (and -0), whatever its rotation
    for zero in (0.0, -0.0):
        casts = box_casts(rng, rays, sizes=np.float32([(zero, zero, zero)]), invalid=False)
        casts["rotation"][::3] = np.nan
        off, hits, _ = A.boxcast_all(rec, nbox, casts)
        assert off.tobytes() == ray_off.tobytes() and hits.tobytes() == ray_hits.tobytes()
    # a capsule of radius and half height 0
    casts = capsule_casts(rng, rays, shapes=np.float32([(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0)]), invalid=False)
    casts["rotation"][::3] = np.nan
    off, hits, _ = A.capsulecast_all(rec, nbox, casts)
    assert off.tobytes() == ray_off.tobytes() and hits.tobytes() == ray_hits.tobytes()
    # a capsule of half height 0 is the ball of its radius
    casts = capsule_casts(rng, rays, shapes=np.float32([(0.05, 0.0), (0.75, 0.0), (2.0, -0.0), (0.0, 0.0)]), invalid=False)
    casts["rotation"][::3] = np.nan
    casts["radius"][5::40], casts["radius"][6::40] = np.nan, -1.0
    ball_off, ball_hits, total = R.spherecast_all(rec, nbox, _as_balls(casts))
    assert total > 384
    off, hits, _ = A.capsulecast_all(rec, nbox, casts)
    assert off.tobytes() == ball_off.tobytes() and hits.tobytes() == ball_hits.tobytes()


@pytest.mark.parametrize("shape", ["box", "capsule"])
def test_offsets_and_the_capacity_prefix_against_a_plain_restatement(shape):
    rec, nbox = _world("pile")
    rng = np.random.default_rng(530)
    rays = _rays(rng, 96, rec)
    casts, call = (box_casts(rng, rays), A.boxcast_all) if shape == "box" else (capsule_casts(rng, rays), A.capsulecast_all)
    full_off, full_hits, total = call(rec, nbox, casts)
    counts = np.diff(full_off.astype(np.int64))
    assert total > 8 and (counts > 1).any() and (counts == 0).any()
    nz = np.nonzero(counts > 1)[0]
    boundary = int(full_off[nz[len(nz) // 2]])
    for cap in (total, total + 3, total - 1, boundary, boundary + 1, 1, 0):
        hits = np.frombuffer(bytes([SENTINEL]) * 32 * max(cap, 1), dtype=E.RAY_HIT).copy()
        off, hits, t2 = call(rec, nbox, casts, capacity=cap, hits=hits)
        ref_off, ref_bytes = _restated(counts, full_hits.tobytes(), cap)
        assert t2 == total and list(off) == ref_off, cap
        assert hits.tobytes() == ref_bytes, cap


def coincident(n):
    """n equal upright boxes at one position (bodies 1 .. n; the ground slab, body 0, elsewhere)."""
    scene = S.pile(n, 0, seed=3)
    scene["body_transforms"]["position"][1:] = (0.25, 3.0, -0.5)
    scene["body_transforms"]["rotation"][1:] = IDENTITY
    scene["box_data"]["size"][1:] = scene["box_data"]["size"][1]
    return scene


def casts_through(centre, n, rng):
    """n rays towards `centre` from 20 units away, ignoring body 0."""
    r = np.zeros(n, dtype=E.RAY)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r["origin"], r["direction"], r["max_t"], r["ignore_body"] = np.float32(centre) - 20.0 * d, d, np.inf, 0
    return r


def test_sixty_four_coincident_boxes_come_at_one_t_in_index_order():
    scene = coincident(64)
    rec = Q.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    rng = np.random.default_rng(540)
    rays = casts_through((0.25, 3.0, -0.5), 48, rng)
    for casts, call, closest in ((box_casts(rng, rays, invalid=False), A.boxcast_all, B.boxcast),
                                 (capsule_casts(rng, rays, invalid=False), A.capsulecast_all, K.capsulecast)):
        off, hits, total = call(rec, nbox, casts)
        assert np.array_equal(off, np.arange(49, dtype=np.uint32) * 64) and total == 48 * 64
        seg = hits.reshape(48, 64)
        assert (seg["t"].copy().view(np.uint32) == seg["t"][:, :1].copy().view(np.uint32)).all()
        assert (seg["collider"] == np.arange(1, 65)).all() and (seg["shape"] == E.NH_SHAPE_BOX).all()
        assert seg[:, 0].tobytes() == closest(rec, nbox, casts).tobytes()
