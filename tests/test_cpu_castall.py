"""All-hits casts on the host (no GPU): nh_raycast_all / nh_spherecast_all of include/nudge_hip.h.

The brute force of tests/hostcastall_util.py -- the oracle of the GPU's chain -- is checked here against oracles that share no code with the feature:
the EXISTING single-collider answers of tests/hostquery_util.py and tests/hostsweep_util.py (`only=c`) decide the set and every record, the existing
closest-hit brute force decides the first record, and a plain Python re-statement decides offsets, the capacity prefix and the marker.  Every
comparison is exact."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostcastall_util as A                 # noqa: E402
import hostquery_util as Q                   # noqa: E402
import hostsweep_util as W                   # noqa: E402
from query_util import SMALL, bounds as _bounds      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

NONE = 0xFFFFFFFF
SENTINEL = 0xA5

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


def _rays(rng, n, rec):
    """The mix the query tests draw: through the scene's bounds, from inside colliders, axis-parallel, a zero direction, ignore_body set, finite and
    infinite max_t."""
    lo, hi = _bounds(rec)
    span = np.maximum(hi - lo, 1.0)
    live = np.nonzero(np.isfinite(rec["p"]).all(axis=1))[0]
    r = np.zeros(n, dtype=E.RAY)
    r["max_t"] = np.inf
    r["ignore_body"] = NONE
    r["origin"] = rng.uniform(lo - 0.2 * span, hi + 0.2 * span, size=(n, 3))
    aim = rng.uniform(lo, hi, size=(n, 3))
    d = aim - r["origin"]
    r["direction"] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.25, 4.0, size=(n, 1))
    kind = np.arange(n) % 8
    inside = kind == 1                                              # from inside a collider (its centre, a little off)
    r["origin"][inside] = rec["p"][rng.choice(live, size=int(inside.sum()))] + rng.normal(scale=0.05, size=(int(inside.sum()), 3)).astype(np.float32)
    axis = kind == 2                                                # axis-parallel: two direction components exactly zero
    d = np.zeros((int(axis.sum()), 3), dtype=np.float32)
    d[np.arange(len(d)), rng.integers(0, 3, size=len(d))] = rng.choice([-1.0, 1.0], size=len(d)) * rng.uniform(0.5, 2.0, size=len(d))
    r["direction"][axis] = d
    down = kind == 3                                                # straight down through the scene
    r["origin"][down, 1] = hi[1] + 5.0
    r["direction"][down] = (0.0, -1.0, 0.0)
    zero = kind == 4                                                # a zero direction, half of them from inside a collider
    r["direction"][zero] = 0.0
    zi = np.nonzero(zero)[0][::2]
    r["origin"][zi] = rec["p"][rng.choice(live, size=len(zi))]
    ign = kind == 5
    r["ignore_body"][ign] = rec["body"][rng.choice(live, size=int(ign.sum()))]
    r["max_t"][kind == 6] = rng.uniform(0.0, 0.5 * float(np.linalg.norm(span)), size=int((kind == 6).sum()))
    r["max_t"][kind == 7] = 0.0
    return r


def _casts(rays, radius):
    c = np.zeros(len(rays), dtype=E.SPHERE_CAST)
    for k in ("origin", "max_t", "direction", "ignore_body"):
        c[k] = rays[k]
    c["radius"] = radius
    return c


def _check_against_the_single_collider_oracle(rec, nbox, casts, got, single, closest, what):
    """`got` = (offsets, hits, total) of the all-hits brute force; `single(c)` = the existing oracle's records with collider c alone, `closest` = its
    closest-hit records."""
    off, hits, total = got
    n, m = len(casts), len(rec)
    assert int(off[n]) == total == len(hits) or total == 0
    only = np.stack([single(c) for c in range(m)])                     # (collider, cast) records
    hit = only["shape"] != NONE
    counts = hit.sum(axis=0)
    assert np.array_equal(np.diff(off.astype(np.int64)), counts), what
    comb = hits["collider"].astype(np.int64) + np.where(hits["shape"] == E.NH_SHAPE_BOX, 0, nbox)
    for i in range(n):
        seg = slice(int(off[i]), int(off[i + 1]))
        cs = comb[seg]
        # the set, one record per collider, and each record the single-collider call's bytes
        assert np.array_equal(np.sort(cs), np.nonzero(hit[:, i])[0]), (what, i)
        assert hits[seg].tobytes() == only[cs, i].tobytes(), (what, i)
        # the order: t non-decreasing as floats, equal t in ascending combined index
        t = hits["t"][seg]
        assert not np.isnan(t).any() and (np.diff(t) >= 0).all(), (what, i)
        tie = np.diff(t) == 0
        assert (np.diff(cs)[tie] > 0).all(), (what, i)
        # the first record is the closest hit; an empty segment is a miss there
        if len(cs):
            assert hits[seg][0].tobytes() == closest[i].tobytes(), (what, i)
        else:
            assert closest[i]["shape"] == NONE, (what, i)
    return counts


@pytest.mark.parametrize("name", sorted(SMALL))
def test_all_hits_equal_the_existing_single_collider_oracles(name):
    scene = SMALL[name]()
    rec = Q.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    rng = np.random.default_rng(300 + sorted(SMALL).index(name))
    rays = _rays(rng, 512, rec)
    got = A.raycast_all(rec, nbox, rays)
    counts = _check_against_the_single_collider_oracle(rec, nbox, rays, got, lambda c: Q.raycast(rec, nbox, rays, only=c), Q.raycast(rec, nbox, rays), f"{name} rays")
    assert counts.max() >= 2 and (counts == 0).any()
    for radius in (0.05, 0.75):
        casts = _casts(rays, radius)
        got = A.spherecast_all(rec, nbox, casts)
        counts = _check_against_the_single_collider_oracle(rec, nbox, casts, got, lambda c: W.spherecast(rec, nbox, casts, only=c), W.spherecast(rec, nbox, casts),
                                                           f"{name} r {radius}")
        assert counts.max() >= 2
    # radius 0 (and -0) gives the ray bytes
    ray_off, ray_hits, _ = A.raycast_all(rec, nbox, rays)
    for r0 in (0.0, -0.0):
        off, hits, _ = A.spherecast_all(rec, nbox, _casts(rays, r0))
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
    off, hits, total = A.raycast_all(rec, nbox, ray)
    assert list(off) == [0, 4096] and total == 4096
    assert len(np.unique(hits["t"].copy().view(np.uint32))) == 1
    assert np.array_equal(hits["collider"], np.arange(1, 4097)) and (hits["shape"] == E.NH_SHAPE_BOX).all()
    assert hits[0].tobytes() == Q.raycast(rec, nbox, ray)[0].tobytes()
    cast = _casts(ray, 0.75)
    off, hits, total = A.spherecast_all(rec, nbox, cast)
    assert list(off) == [0, 4096] and np.array_equal(hits["collider"], np.arange(1, 4097)) and len(np.unique(hits["t"])) == 1
    assert hits[0].tobytes() == W.spherecast(rec, nbox, cast)[0].tobytes()


def test_invalid_records_count_zero():
    scene = SMALL["pile"]()
    rec = Q.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    lo, hi = _bounds(rec)
    good = np.zeros(1, dtype=E.SPHERE_CAST)
    good["origin"], good["direction"], good["max_t"], good["ignore_body"], good["radius"] = (0.5 * (lo + hi)) + (0, 50, 0), (0, -1, 0), np.inf, NONE, 0.5
    assert A.spherecast_all(rec, nbox, good)[2] > 0 and A.raycast_all(rec, nbox, good.view(np.uint8).reshape(1, 48)[:, :32].copy().view(E.RAY).reshape(1))[2] > 0
    bad = np.repeat(good, 8)
    bad["origin"][0, 1] = np.nan
    bad["origin"][1, 0] = np.inf
    bad["direction"][2, 2] = np.nan
    bad["direction"][3, 1] = -np.inf
    bad["max_t"][4] = np.nan                       # (t <= NaN is false: nothing is listed)
    bad["radius"][5] = np.nan
    bad["radius"][6] = np.inf
    bad["radius"][7] = -0.25
    off, _, total = A.spherecast_all(rec, nbox, bad)
    assert total == 0 and not off.any()
    rays = bad.view(np.uint8).reshape(8, 48)[:5, :32].copy().view(E.RAY).reshape(5)
    off, _, total = A.raycast_all(rec, nbox, rays)
    assert total == 0 and not off.any()


def _restated(counts, records, capacity):
    """offsets, the written records and the bytes behind them, from the per-cast counts and the full list: the header's rules in plain Python."""
    total = int(sum(counts))
    off = [0]
    for k in counts:
        off.append((off[-1] + int(k)) & 0xFFFFFFFF)
    out = bytearray([SENTINEL]) * (32 * max(capacity, 1))
    if total >= 0xFFFFFFFF:
        off[-1] = NONE
        return off, bytes(out)
    for i in range(len(counts)):
        if off[i + 1] <= capacity:
            out[32 * off[i]: 32 * off[i + 1]] = records[32 * off[i]: 32 * off[i + 1]]
    return off, bytes(out)


def test_offsets_the_capacity_prefix_and_the_marker_against_a_plain_restatement():
    scene = S.pile(24, 8, seed=3)
    rec = Q.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    rays = _rays(np.random.default_rng(5), 64, rec)
    full_off, full_hits, total = A.raycast_all(rec, nbox, rays)
    counts = np.diff(full_off.astype(np.int64))
    assert total > 8 and (counts > 1).any() and (counts == 0).any()
    nz = np.nonzero(counts > 1)[0]
    boundary = int(full_off[nz[len(nz) // 2]])
    for cap in (total, total + 3, total - 1, boundary, boundary + 1, 1, 0):
        hits = np.frombuffer(bytes([SENTINEL]) * 32 * max(cap, 1), dtype=E.RAY_HIT).copy()
        off, hits, t2 = A.raycast_all(rec, nbox, rays, capacity=cap, hits=hits)
        ref_off, ref_bytes = _restated(counts, full_hits.tobytes(), cap)
        assert t2 == total and list(off) == ref_off, cap
        assert hits.tobytes() == ref_bytes, cap
    # the marker: 2^20 rays through 4096 coincident boxes make 2^32 records; one fewer stays below it
    scene = _coincident()
    rec = Q.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    ray = np.zeros(1, dtype=E.RAY)
    ray["origin"], ray["direction"], ray["max_t"], ray["ignore_body"] = (0.25, 3.0, -0.5), (0, 0, 1), np.inf, 0
    assert A.raycast_all(rec, nbox, ray)[2] == 4096
    ref_off, _ = _restated([4096] * (1 << 20), b"", 0)
    assert ref_off[-1] == NONE
    hits = np.frombuffer(bytes([SENTINEL]) * 32 * 8192, dtype=E.RAY_HIT).copy()
    off, hits, total = A.raycast_all(rec, nbox, np.repeat(ray, 1 << 20), capacity=8192, hits=hits)
    assert total == 1 << 32 and off[-1] == NONE and set(hits.tobytes()) == {SENTINEL}
    few = np.repeat(ray, 33)
    hits = np.frombuffer(bytes([SENTINEL]) * 32 * 4096 * 33, dtype=E.RAY_HIT).copy()
    off, hits, total = A.raycast_all(rec, nbox, few, capacity=4096 * 33, hits=hits)
    assert total == 4096 * 33 and np.array_equal(off, np.arange(34, dtype=np.uint32) * 4096)
    assert hits[:4096].tobytes() * 33 == hits.tobytes()
