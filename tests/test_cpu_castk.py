"""First-k casts on the host (no GPU): nh_raycast_k / nh_spherecast_k / nh_boxcast_k / nh_capsulecast_k of include/nudge_hip.h.

What the kernel rests on is checked here without it: the pruning premise of DESIGN 10.13 -- no collider is listed at a t below the entry of its own
leaf box under the k walk's node test -- counted by tests/hostoracle/hostcastk.cpp over every pair the all-hits brute forces list; the order of the
bounded list the kernel keeps (nh_q_nearest_insert through tests/hostnearest_util.py) against a plain sort by (bits of t + 0, index); the oracle of
tests/hostcastk_util.py against itself (PREFIX) and against the closest-hit brute forces (k = 1); the shares that keep the GPU comparisons from being
empty; and the declarations and exports.  Every comparison is exact."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import castk_batches as CB                   # noqa: E402
import hostcast_util as CAST                 # noqa: E402
import hostcastk_util as HK                  # noqa: E402
import hostnearest_util as N                 # noqa: E402
import hostquery_util as Q                   # noqa: E402
from cast_util import (HOST_WORLDS, box_casts, capsule_casts, every_kind_of_ray, far_and_near_scene as _far_and_near_scene, host_world, sphere_casts,      # noqa: E402
                       spheres, wide_casts)
from query_util import SMALL                 # noqa: E402
from nudge_amd import engine as E           # noqa: E402

NONE = 0xFFFFFFFF
NAMES = ("nh_raycast_k", "nh_spherecast_k", "nh_boxcast_k", "nh_capsulecast_k")


# ---- declarations and exports -----------------------------------------------------------------------------------------------------------------
def test_the_four_entry_points_are_declared_exported_and_built():
    header = open(os.path.join(ROOT, "include", "nudge_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S)).replace(" ,", ",")
    assert "#define NH_CAST_K_MAX 32u" in header
    tail = "uint32_t count, uint32_t k, uint32_t* counts, nh_RayHit* hits, uint32_t flags );"
    for name, record, arg in zip(NAMES, ("nh_Ray", "nh_SphereCast", "nh_BoxCast", "nh_CapsuleCast"), ("rays", "casts", "casts", "casts")):
        assert f"int {name}(nh_context* ctx, const {record}* {arg}, {tail}" in flat, name
    assert set(NAMES) <= set(E.EXPORTS)
    # note 9's list of observers names them, and nothing says any more that a hit limit is not built
    note9 = next(line for line in header.splitlines() if "The scene queries (nh_query_build" in line)
    assert all(name in note9 for name in NAMES)
    assert "a per-query hit limit" not in header
    so = os.path.join(ROOT, "nudge_amd", "libnudge_hip.so")
    if not os.path.exists(so):
        pytest.fail("nudge_amd/libnudge_hip.so is not built")
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    for name in NAMES:
        assert f" T {name}\n" in syms, name
    for name in NAMES:
        stem = name[3:]
        assert callable(getattr(E.World, stem)) and callable(getattr(E.World, stem + "_records")), name


# ---- the pruning premise ------------------------------------------------------------------------------------------------------------------------
def _premise(rec, nbox, casts, what, least=1):
    seg = HK.segments(rec, nbox, casts)
    assert len(seg[1]) >= least, (what, len(seg[1]))
    bad = HK.premise(rec, nbox, casts, seg)
    assert bad == 0, f"{what}: {bad} of {len(seg[1])} listed pairs enter their own leaf box after their t, or not at all"
    return len(seg[1])


@pytest.mark.parametrize("name", sorted(SMALL))
def test_premise_on_the_small_worlds_under_the_all_hits_tests_rays_and_balls(name):
    scene = SMALL[name]()
    rec = Q.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    rays = every_kind_of_ray(np.random.default_rng(300 + sorted(SMALL).index(name)), 512, rec)
    _premise(rec, nbox, rays, f"{name} rays", 512)
    for radius in (0.0, -0.0, 0.05, 0.75):
        _premise(rec, nbox, spheres(rays, radius), f"{name} r {radius}", 512)


@pytest.mark.parametrize("name", sorted(HOST_WORLDS))
def test_premise_on_the_small_worlds_under_the_all_hits_tests_boxes_and_capsules(name):
    rec, nbox = host_world(name)
    rng = np.random.default_rng(500 + sorted(HOST_WORLDS).index(name))
    _premise(rec, nbox, box_casts(rng, every_kind_of_ray(rng, 384, rec)), f"{name} boxes", 384)
    rng = np.random.default_rng(510 + sorted(HOST_WORLDS).index(name))
    _premise(rec, nbox, capsule_casts(rng, every_kind_of_ray(rng, 384, rec)), f"{name} capsules", 384)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_premise_and_the_shares_of_the_batches_the_gpu_tests_compare(name):
    scene = SMALL[name]()
    rec = Q.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    rng = np.random.default_rng(700 + sorted(SMALL).index(name))
    for shape, casts in CB.batches(rng, 1000, rec).items():
        seg = HK.segments(rec, nbox, casts)
        CB.assert_not_empty(seg[0], f"{name} {shape}")
        assert HK.premise(rec, nbox, casts, seg) == 0, (name, shape)


def sphere_column(height=300.0, n=600, seed=9):
    """hostlib.REC records of n spheres of radius 0.5 .. 1.5 in a column `height` tall around the y axis (DESIGN 10.8 measures the ray predicates'
    rounding on such a column: seen from 300 units up, a sphere is accepted a little outside its radius), and 2048 downward rays from above it,
    most of them near the rim of a sphere."""
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, dtype=HK.H.REC)
    rec["p"][:, 0], rec["p"][:, 2] = rng.uniform(-0.5, 0.5, size=n), rng.uniform(-0.5, 0.5, size=n)
    rec["p"][:, 1] = np.linspace(0.0, height, n)
    rec["q"][:, 3] = 1.0
    rec["h"] = rng.uniform(0.5, 1.5, size=(n, 1)).astype(np.float32)
    rec["body"], rec["tag"] = np.arange(1, n + 1), np.arange(n)
    m = 2048
    rays = np.zeros(m, dtype=E.RAY)
    rays["max_t"], rays["ignore_body"] = np.inf, NONE
    rays["direction"] = (0.0, -1.0, 0.0)
    at = rng.integers(0, n, size=m)
    phi = rng.uniform(0.0, 2.0 * np.pi, size=m)
    rim = rec["h"][at, 0] * (1.0 + rng.normal(scale=2e-4, size=m))          # grazing: within a few 1e-4 of the radius
    rim[::4] = rec["h"][at[::4], 0] * rng.uniform(0.0, 1.0, size=len(rim[::4]))
    rays["origin"][:, 0] = rec["p"][at, 0] + rim * np.cos(phi)
    rays["origin"][:, 1] = height + 5.0
    rays["origin"][:, 2] = rec["p"][at, 2] + rim * np.sin(phi)
    return rec, rays


def test_premise_on_downward_rays_over_a_300_unit_column_of_spheres():
    rec, rays = sphere_column()
    listed = _premise(rec, 0, rays, "column rays", 100000)
    # the same lines as a ball of r = 0, a box of size 0 and a capsule of r = hh = 0 (the ray-like shapes take the same pad), and with a size
    rng = np.random.default_rng(10)
    assert _premise(rec, 0, sphere_casts(rays, np.float32([0.0, -0.0]), invalid=False), "column r 0") == listed
    assert _premise(rec, 0, box_casts(rng, rays, sizes=np.float32([(0, 0, 0)]), invalid=False), "column size 0") == listed
    assert _premise(rec, 0, capsule_casts(rng, rays, shapes=np.float32([(0, 0)]), invalid=False), "column r hh 0") == listed
    _premise(rec, 0, sphere_casts(rays, np.float32([1e-3, 0.25]), invalid=False), "column balls", listed)
    _premise(rec, 0, box_casts(rng, rays, invalid=False), "column boxes", listed)
    _premise(rec, 0, capsule_casts(rng, rays, invalid=False), "column capsules", listed)


def wide_world():
    """(records, nbox) of a world of 1e-3 .. 1e4 units: half the bodies within 0.05 of the origin at size 1e-3, the others anywhere within 1e4."""
    scene = _far_and_near_scene()
    return Q.records(scene["body_transforms"], scene), len(scene["box_tags"])


def test_premise_on_a_world_spanning_a_thousandth_and_ten_thousand_units():
    rec, nbox = wide_world()
    for shape, casts in wide_casts(np.random.default_rng(11), rec).items():
        _premise(rec, nbox, casts, f"1e-3 .. 1e4 {shape}", 1024)


# ---- the order of the list ----------------------------------------------------------------------------------------------------------------------
def _tbits(t):
    return (np.float32(t) + np.float32(0.0)).view(np.uint32)


@pytest.mark.parametrize("stride", [1, 64])
def test_the_list_holds_the_first_k_by_t_bits_and_index(stride):
    rng = np.random.default_rng(12)
    max_t = np.float32(7.5)
    pool = np.float32([0.0, -0.0, 0.0, -0.0, 1.0, 1.0, 1.0, 2.5, 2.5, 7.5, 7.5, np.nextafter(np.float32(7.5), np.float32(8)), 8.0, np.inf, np.nan, 1e-38, 3.0])
    for k in range(1, 33):
        # (more than k candidates at exactly one t, and at +-0, among the others; every index once, in a random order)
        m = 3 * k + 40
        t = np.concatenate([np.full(k + 5, 2.5, np.float32), np.tile(np.float32([0.0, -0.0]), k // 2 + 3), rng.choice(pool, size=m).astype(np.float32),
                            rng.uniform(0.0, 9.0, size=m).astype(np.float32)])
        idx = rng.permutation(len(t)).astype(np.uint32)
        keys, held, changed = N.insert(t, idx, k, stride=stride, max_d=max_t)
        ok = t <= max_t                                    # (NaN and everything above max_t never goes in)
        order = np.lexsort((idx[ok], _tbits(t[ok])))
        want_t, want_c = t[ok][order][:k], idx[ok][order][:k]
        assert len(held) == min(k, int(ok.sum())) == len(want_c)
        assert np.array_equal(held, want_c), (k, stride)
        # the keys are the offered values themselves, -0 kept as -0: the order took them as floats
        assert keys.view(np.uint32).tobytes() == want_t.view(np.uint32).tobytes(), (k, stride)
        assert not changed[~ok].any()
        # every t of the list is at most the k-th: what the walk's bound reloads
        assert (keys <= keys[-1]).all()


# ---- the oracle against itself and against the closest-hit brute forces ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pile", "stacks"])
def test_prefix_in_k_and_k_1_is_the_closest_hit_brute_force(name):
    scene = SMALL[name]()
    rec = Q.records(scene["body_transforms"], scene)
    nbox = len(scene["box_tags"])
    rng = np.random.default_rng(720 + sorted(SMALL).index(name))
    for shape, casts in CB.batches(rng, 384, rec).items():
        seg = HK.segments(rec, nbox, casts)
        size = np.diff(seg[0].astype(np.int64))
        counts32, hits32 = HK.cast_k(rec, nbox, casts, 32, seg)
        assert np.array_equal(counts32, np.minimum(size, 32))
        for k in (1, 2, 3, 8, 9, 16, 17):
            counts, hits = HK.cast_k(rec, nbox, casts, k, seg)
            assert np.array_equal(counts, np.minimum(size, k)) and hits.shape == (len(casts), k)
            full = size >= k                               # (a row that is cut: the same records; a shorter one: the same, then misses)
            assert hits[full].tobytes() == np.ascontiguousarray(hits32[full, :k]).tobytes(), (shape, k)
            assert hits.tobytes() == np.ascontiguousarray(hits32[:, :k]).tobytes(), (shape, k)
            held = np.arange(k)[None, :] < counts[:, None]
            assert (hits["shape"][held] != NONE).all() and (hits["shape"][~held] == NONE).all()
        best = CAST.cast(CAST.SHAPES[shape], rec, nbox, casts)
        counts, hits = HK.cast_k(rec, nbox, casts, 1, seg)
        assert hits[:, 0].tobytes() == best.tobytes(), shape
        assert np.array_equal(counts, (best["shape"] != NONE).astype(np.uint32))
        # an invalid record counts 0 and its misses are NaN; a NaN max_t lists nothing and its misses carry the NaN
        nan_t = np.isnan(best["t"])
        assert nan_t.any() and (counts[nan_t] == 0).all() and np.isnan(hits32["t"][nan_t]).all()
