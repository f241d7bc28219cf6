"""All-hits casts on the host (no GPU): nh_raycast_all / nh_spherecast_all of include/nudge_hip.h.

The all-hits brute force of tests/hostcast_util.py -- the oracle of the GPU's chain -- is checked here against oracles that share neither its
per-collider decision nor its list handling: the closest-hit brute force beside it (`only=c`), a loop of its own over the closest-hit predicates,
decides the set and every record, the same brute force over all colliders decides the first record, and a plain Python re-statement decides offsets, the capacity prefix and the marker.  Every
comparison is exact."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostcast_util as CAST                 # noqa: E402
import hostquery_util as Q                   # noqa: E402
from cast_util import (SENTINEL, check_against_the_single_collider_oracle as _check_against_the_single_collider_oracle, every_kind_of_ray as _rays,      # noqa: E402
                       restated as _restated, spheres as _casts)
from query_util import NONE, SMALL, bounds as _bounds      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402


def test_both_entry_points_are_exported_with_their_prototypes():
    assert {"nh_raycast_all", "nh_spherecast_all"} <= set(E.EXPORTS)
    declared = open(os.path.join(ROOT, "include", "nudge_hip.h")).read()
    assert "int nh_raycast_all(" in declared and "int nh_spherecast_all(" in declared
    so = os.path.join(ROOT, "nudge_amd", "libnudge_hip.so")
    if not os.path.exists(so):
        pytest.fail("nudge_amd/libnudge_hip.so is not built")
    import subprocess
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    for name in ("nh_raycast_all", "nh_spherecast_all"):
        assert f" T {name}\n" in syms, name
    for name in ("raycast_all_records", "raycast_all", "spherecast_all_records", "spherecast_all"):
        assert callable(getattr(E.World, name)), name
    src = open(os.path.join(ROOT, "nudge_amd", "engine.py")).read()
    proto = "argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]"
    assert f"L.nh_raycast_all.{proto}" in src and f"L.nh_spherecast_all.{proto}" in src


@pytest.mark.parametrize("name", sorted(SMALL))
def test_all_hits_equal_the_existing_single_collider_oracles(name):
    scene = SMALL[name]()
    rec = Q.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    rng = np.random.default_rng(300 + sorted(SMALL).index(name))
    rays = _rays(rng, 512, rec)
    got = CAST.cast_all(CAST.RAY, rec, nbox, rays)
    counts = _check_against_the_single_collider_oracle(rec, nbox, rays, got, lambda c: CAST.cast(CAST.RAY, rec, nbox, rays, only=c), CAST.cast(CAST.RAY, rec, nbox, rays), f"{name} rays")
    assert counts.max() >= 2 and (counts == 0).any()
    for radius in (0.05, 0.75):
        casts = _casts(rays, radius)
        got = CAST.cast_all(CAST.SPHERE, rec, nbox, casts)
        counts = _check_against_the_single_collider_oracle(rec, nbox, casts, got, lambda c: CAST.cast(CAST.SPHERE, rec, nbox, casts, only=c), CAST.cast(CAST.SPHERE, rec, nbox, casts),
                                                           f"{name} r {radius}")
        assert counts.max() >= 2
    # radius 0 (and -0) gives the ray bytes
    ray_off, ray_hits, _ = CAST.cast_all(CAST.RAY, rec, nbox, rays)
    for r0 in (0.0, -0.0):
        off, hits, _ = CAST.cast_all(CAST.SPHERE, rec, nbox, _casts(rays, r0))
        assert off.tobytes() == ray_off.tobytes() and hits.tobytes() == ray_hits.tobytes()


def _coincident(n=4096):
    scene = S.pile(n, 0, seed=3)
    scene["body_transforms"]["position"][1:] = (0.25, 3.0, -0.5)        # every box at one position; the ground slab elsewhere
    return scene


def test_four_thousand_boxes_at_one_position_come_at_one_t_in_index_order():
    scene = _coincident()
    scene["body_transforms"]["rotation"][1:] = (0.0, 0.0, 0.0, 1.0)
    scene["box_data"]["size"][1:] = scene["box_data"]["size"][1]
    rec = Q.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    ray = np.zeros(1, dtype=E.RAY)
    ray["origin"], ray["direction"], ray["max_t"], ray["ignore_body"] = (0.25, 3.0, -20.0), (0, 0, 1), np.inf, 0
    off, hits, total = CAST.cast_all(CAST.RAY, rec, nbox, ray)
    assert list(off) == [0, 4096] and total == 4096
    assert len(np.unique(hits["t"].copy().view(np.uint32))) == 1
    assert np.array_equal(hits["collider"], np.arange(1, 4097)) and (hits["shape"] == E.NH_SHAPE_BOX).all()
    assert hits[0].tobytes() == CAST.cast(CAST.RAY, rec, nbox, ray)[0].tobytes()
    cast = _casts(ray, 0.75)
    off, hits, total = CAST.cast_all(CAST.SPHERE, rec, nbox, cast)
    assert list(off) == [0, 4096] and np.array_equal(hits["collider"], np.arange(1, 4097)) and len(np.unique(hits["t"])) == 1
    assert hits[0].tobytes() == CAST.cast(CAST.SPHERE, rec, nbox, cast)[0].tobytes()


def test_invalid_records_count_zero():
    scene = SMALL["pile"]()
    rec = Q.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    lo, hi = _bounds(rec)
    good = np.zeros(1, dtype=E.SPHERE_CAST)
    good["origin"], good["direction"], good["max_t"], good["ignore_body"], good["radius"] = (0.5 * (lo + hi)) + (0, 50, 0), (0, -1, 0), np.inf, NONE, 0.5
    assert CAST.cast_all(CAST.SPHERE, rec, nbox, good)[2] > 0 and CAST.cast_all(CAST.RAY, rec, nbox, good.view(np.uint8).reshape(1, 48)[:, :32].copy().view(E.RAY).reshape(1))[2] > 0
    bad = np.repeat(good, 8)
    bad["origin"][0, 1] = np.nan
    bad["origin"][1, 0] = np.inf
    bad["direction"][2, 2] = np.nan
    bad["direction"][3, 1] = -np.inf
    bad["max_t"][4] = np.nan                       # (t <= NaN is false: nothing is listed)
    bad["radius"][5] = np.nan
    bad["radius"][6] = np.inf
    bad["radius"][7] = -0.25
    off, _, total = CAST.cast_all(CAST.SPHERE, rec, nbox, bad)
    assert total == 0 and not off.any()
    rays = bad.view(np.uint8).reshape(8, 48)[:5, :32].copy().view(E.RAY).reshape(5)
    off, _, total = CAST.cast_all(CAST.RAY, rec, nbox, rays)
    assert total == 0 and not off.any()


def test_offsets_the_capacity_prefix_and_the_marker_against_a_plain_restatement():
    scene = S.pile(24, 8, seed=3)
    rec = Q.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    rays = _rays(np.random.default_rng(5), 64, rec)
    full_off, full_hits, total = CAST.cast_all(CAST.RAY, rec, nbox, rays)
    counts = np.diff(full_off.astype(np.int64))
    assert total > 8 and (counts > 1).any() and (counts == 0).any()
    nz = np.nonzero(counts > 1)[0]
    boundary = int(full_off[nz[len(nz) // 2]])
    for cap in (total, total + 3, total - 1, boundary, boundary + 1, 1, 0):
        hits = np.frombuffer(bytes([SENTINEL]) * 32 * max(cap, 1), dtype=E.RAY_HIT).copy()
        off, hits, t2 = CAST.cast_all(CAST.RAY, rec, nbox, rays, capacity=cap, hits=hits)
        ref_off, ref_bytes = _restated(counts, full_hits.tobytes(), cap)
        assert t2 == total and list(off) == ref_off, cap
        assert hits.tobytes() == ref_bytes, cap
    # the marker: 2^20 rays through 4096 coincident boxes make 2^32 records; one fewer stays below it
    scene = _coincident()
    rec = Q.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    ray = np.zeros(1, dtype=E.RAY)
    ray["origin"], ray["direction"], ray["max_t"], ray["ignore_body"] = (0.25, 3.0, -0.5), (0, 0, 1), np.inf, 0
    assert CAST.cast_all(CAST.RAY, rec, nbox, ray)[2] == 4096
    ref_off, _ = _restated([4096] * (1 << 20), b"", 0)
    assert ref_off[-1] == NONE
    hits = np.frombuffer(bytes([SENTINEL]) * 32 * 8192, dtype=E.RAY_HIT).copy()
    off, hits, total = CAST.cast_all(CAST.RAY, rec, nbox, np.repeat(ray, 1 << 20), capacity=8192, hits=hits)
    assert total == 1 << 32 and off[-1] == NONE and set(hits.tobytes()) == {SENTINEL}
    few = np.repeat(ray, 33)
    hits = np.frombuffer(bytes([SENTINEL]) * 32 * 4096 * 33, dtype=E.RAY_HIT).copy()
    off, hits, total = CAST.cast_all(CAST.RAY, rec, nbox, few, capacity=4096 * 33, hits=hits)
    assert total == 4096 * 33 and np.array_equal(off, np.arange(34, dtype=np.uint32) * 4096)
    assert hits[:4096].tobytes() * 33 == hits.tobytes()
