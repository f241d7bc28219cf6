"""nh_query_refit on the GPU (pytest -m gpu): the hierarchy of the last nh_query_build made current (include/nudge_hip.h, "scene queries").

The contract is exact: after a refit every query writes the bytes it writes after a build on the same arrays.  The queries' answers never depend on
the tree, so the oracle is the one the other query tests use -- a brute force over every collider on the host with the device's arithmetic, over the
CURRENT transforms -- and every comparison is byte for byte (any-hit rays: hit or miss).  A refit is an observer like the build."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostcapsule_util as HC                # noqa: E402
import hostcast_util as CAST                 # noqa: E402
import hostpoint_util as HP                  # noqa: E402
import hostquery_util as Q                   # noqa: E402
import test_gpu_closest as TP                # noqa: E402
import test_gpu_overlap as TO                # noqa: E402
from cast_util import boxes, capsules, closest as _cast, same_hits as _same_hits, spheres      # noqa: E402
from query_util import OBSERVED, SMALL, bounds as _bounds, rays as _rays, records as _records, same_stepped_world as _same_stepped_world, unit_quats, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
FUSED = E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP


def _batch(rng, n, rec):
    """One batch of every query type around the colliders of `rec`, from the existing tests' generators."""
    lo, hi = _bounds(rec)
    rays = np.concatenate([_rays(rng, n, lo, hi, kind) for kind in ("random", "axis", "down")])
    rays["max_t"] = rng.choice([np.inf, 5.0, 50.0], size=len(rays))
    m = len(rays)
    points = np.concatenate([TP._points(rng, n, rec, lo, hi, kind) for kind in ("inside", "uniform", "above")])
    return dict(
        rays=rays,
        spheres=spheres(rays, rng.choice(np.float32((0.05, 0.5, 2.0)), size=m)),
        boxes=boxes(rays, rng.choice(np.float32((0.05, 0.5, 2.0)), size=m), unit_quats(rng, m)),
        capsules=capsules(rays, rng.choice(np.float32([0.05, 0.5, 1.0]), size=m), rng.choice(np.float32([0.0, 0.5, 2.0]), size=m), unit_quats(rng, m)),
        points=TP._queries(points, max_distance=rng.choice(np.float32([np.inf, 0.5, 2.0]), size=len(points))),
        overlaps=np.concatenate([TO._queries(rng, n, rec, kind) for kind in ("sphere", "box", "mixed")]),
        capsule_overlaps=TO._capsule_queries(rng, n, rec))


def _host(rec, nbox, b):
    """The brute-force answers to a batch over the records `rec`: what a build on those transforms must answer, byte for byte."""
    ov_off, _, ov_total = TO.O.overlap(rec, nbox, b["overlaps"], capacity=0)
    cap_off, _, cap_total = HC.overlap(rec, nbox, b["capsule_overlaps"], capacity=0)
    return dict(rays=CAST.cast(CAST.RAY, rec, nbox, b["rays"]), spheres=CAST.cast(CAST.SPHERE, rec, nbox, b["spheres"]), boxes=CAST.cast(CAST.BOX, rec, nbox, b["boxes"]),
                capsules=CAST.cast(CAST.CAPSULE, rec, nbox, b["capsules"]), points=HP.closest(rec, nbox, b["points"]),
                overlap_counts=ov_off, overlap_list=TO.O.overlap(rec, nbox, b["overlaps"], capacity=ov_total, hits=TO.sentinel_hits(ov_total, E.OVERLAP_HIT))[:2],
                capsule_counts=cap_off, capsule_list=_capsule_host(rec, nbox, b["capsule_overlaps"], cap_total))


def _capsule_host(rec, nbox, queries, cap):
    hits = np.frombuffer(bytes([TO.SENTINEL]) * 16 * max(cap, 1), dtype=E.OVERLAP_HIT).copy()
    off, hits, _ = HC.overlap(rec, nbox, queries, capacity=cap, hits=hits)
    return off, hits


def _gpu(w, b, ref):
    """The GPU's answers to the batch, in the layout of _host (list calls with the capacity of `ref`'s lists)."""
    return dict(rays=_cast(w, b["rays"]), any_hit=_cast(w, b["rays"], any_hit=True), spheres=_cast(w, b["spheres"]), boxes=_cast(w, b["boxes"]),
                capsules=_cast(w, b["capsules"]), points=TP._closest(w, b["points"]),
                overlap_counts=TO._gpu(w, b["overlaps"], None)[0], overlap_list=TO._gpu(w, b["overlaps"], len(ref["overlap_list"][1])),
                capsule_counts=TO._gpu(w, b["capsule_overlaps"], None)[0], capsule_list=TO._gpu(w, b["capsule_overlaps"], len(ref["capsule_list"][1])))


def _differing(got, ref):
    """The names of the answers that differ in any byte (any-hit rays: in hit-or-miss)."""
    out = []
    for k, r in ref.items():
        g = got[k]
        same = all(x.tobytes() == y.tobytes() for x, y in zip(g, r)) if isinstance(r, tuple) else g.tobytes() == r.tobytes()
        if not same:
            out.append(k)
    if not np.array_equal(got["any_hit"]["shape"] == NONE, ref["rays"]["shape"] == NONE):
        out.append("any_hit")
    return out


def _check(w, rec, rng, n, what):
    """Every query type on the world's current hierarchy against the brute force over `rec`; returns the GPU's answers and the batch."""
    b = _batch(rng, n, rec)
    ref = _host(rec, w.nbox, b)
    got = _gpu(w, b, ref)
    assert _differing(got, ref) == [], f"{what}: differ from the brute force"
    return b, ref, got


# ---- the contract ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SMALL))
def test_every_query_type_after_a_refit_equals_the_brute_force(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(700 + sorted(SMALL).index(name))
    w = E.World(scene, flags=FUSED)
    w.query_build()
    _check(w, _records(w, scene), rng, 2048, f"{name} build at step 0")
    for k in (1, 2, 5, 50):                        # bodies fall, land, some fall asleep
        w.step(k)
        w.query_refit()
        rec = _records(w, scene)
        b, ref, got = _check(w, rec, rng, 2048, f"{name} refit after {k} more steps")
        assert (ref["rays"]["shape"] != NONE).mean() > 0.05 and ref["overlap_counts"][-1] > 0
    w.query_build()                                # a fresh build on the same state: the same bytes again
    again = _gpu(w, b, ref)
    assert _differing(again, ref) == [], f"{name}: the fresh build differs"
    for k in ("rays", "spheres", "boxes", "capsules", "points"):
        assert again[k].tobytes() == got[k].tobytes(), k
    w.close()


@pytest.mark.parametrize("name", ["pile", "grid_tiles"])
def test_the_refit_really_rereads_the_world(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(710)
    w = E.World(scene, flags=FUSED)
    w.query_build()
    old = _records(w, scene)
    b = _batch(rng, 2048, old)
    ref_old = _host(old, w.nbox, b)
    w.step(50)
    new = _records(w, scene)
    ref_new = _host(new, w.nbox, b)
    assert ref_old["rays"].tobytes() != ref_new["rays"].tobytes() and ref_old["points"].tobytes() != ref_new["points"].tobytes()
    # without a refit: the LAST build's world
    assert _differing(_gpu(w, b, ref_old), ref_old) == []
    w.query_refit()
    assert _differing(_gpu(w, b, ref_new), ref_new) == []
    w.close()


def test_a_teleported_body_is_found_at_its_new_place_only():
    scene = S.pile(256, 64, seed=1)
    w = E.World(scene, flags=FUSED)
    w.step(20)
    w.query_build()
    rec = _records(w, scene)
    lo, hi = _bounds(rec)
    body = int(scene["box_transforms"]["body"][w.nbox - 1])                 # the body of the last box
    assert body != 0
    old_p = w.get_bodies()["transforms"]["position"][body].astype(np.float64)
    bt = w.get_bodies()["transforms"].copy()
    new_p = hi + (hi - lo) * 10.0 + 1000.0                                    # far outside the bounds of the build
    bt["position"][body] = new_p
    w.set_bodies(transforms=bt)
    w.torch.cuda.synchronize()
    # one ray down onto the new place, one that starts at the old centre of the body's collider (inside it: a hit at t = 0 while it is there)
    rays = np.zeros(2, dtype=E.RAY)
    rays["origin"] = [rec["p"][w.nbox - 1].astype(np.float64) - old_p + new_p + (0.0, 50.0, 0.0), rec["p"][w.nbox - 1]]
    rays["direction"] = (0.0, -1.0, 0.0)
    rays["max_t"] = np.inf
    rays["ignore_body"] = NONE
    before = _cast(w, rays)
    assert before["shape"][0] == NONE and before["body"][1] == body           # the LAST build: still at the old place
    w.query_refit()
    rec = _records(w, scene)
    after = _cast(w, rays)
    _same_hits(after, CAST.cast(CAST.RAY, rec, w.nbox, rays), "teleported")
    assert after["body"][0] == body and after["body"][1] != body
    _check(w, rec, np.random.default_rng(711), 1024, "teleported, all types")
    w.close()


# ---- degenerate worlds ----------------------------------------------------------------------------------------------------------------------
def test_degenerate_worlds():
    rng = np.random.default_rng(720)
    scene = S.pile(300, 300, seed=3)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    for what, nbox, nsph in (("one collider", 1, 0), ("spheres only", 0, 300), ("boxes only", 301, 0)):
        w.set_counts(nb, nbox, nsph)
        w.query_build()
        w.set_counts(nb, 301, 300)                 # (the whole world steps; the hierarchy is of the part)
        w.step(7)
        w.set_counts(nb, nbox, nsph)
        w.query_refit()
        _check(w, _records(w, scene), rng, 1024, what)
    # zero colliders: NH_OK, and every query misses as after a build
    w.set_counts(nb, 0, 0)
    w.query_build()
    w.query_refit()
    q = TP._queries(rng.uniform(-5, 5, size=(256, 3)))
    got = TP._closest(w, q)
    assert (got["shape"] == NONE).all()
    TP._same_hits(got, HP.closest(np.zeros(0, dtype=Q.REC), 0, q), "no collider")
    w.close()


def test_four_thousand_boxes_at_one_position_then_moved_apart():
    scene = S.pile(4096, 0, seed=3)
    apart = scene["body_transforms"]["position"].copy()
    scene["body_transforms"]["position"][1:] = (0.25, 3.0, -0.5)             # every Morton key equal but the ground's
    w = E.World(scene, flags=FUSED)
    w.query_build()
    w.query_refit()
    rng = np.random.default_rng(721)
    _check(w, _records(w, scene), rng, 1024, "4096 coincident boxes, refitted in place")
    bt = w.get_bodies()["transforms"].copy()
    bt["position"] = apart
    w.set_bodies(transforms=bt)
    w.torch.cuda.synchronize()
    w.query_refit()                                                          # a tree sorted by collider index alone, over boxes that now lie apart
    _check(w, _records(w, scene), rng, 1024, "4096 boxes moved apart")
    w.close()


def test_nan_pose_colliders_before_and_after():
    scene = S.pile(256, 64, seed=1)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    rng = np.random.default_rng(722)
    w.set_counts(nb - 10, w.nbox, w.nsph)                  # the last 10 spheres belong to bodies that no longer exist: NaN poses
    w.query_build()
    w.set_counts(nb, w.nbox, w.nsph)                        # (the whole world steps)
    w.step(5)
    w.set_counts(nb - 10, w.nbox, w.nsph)
    w.query_refit()
    rec = Q.records(w.get_bodies()["transforms"][: nb - 10], scene, w.nbox, w.nsph)
    assert np.isnan(rec["p"][-10:]).all() and np.isfinite(rec["p"][:-10]).all()
    b, ref, got = _check(w, rec, rng, 1024, "NaN poses after the build")
    assert not ((got["points"]["shape"] == E.NH_SHAPE_SPHERE) & (got["points"]["collider"] >= w.nsph - 10)).any()
    # the bodies come back: same counts of colliders, so the refit takes them; and leave again
    w.set_counts(nb, w.nbox, w.nsph)
    w.query_refit()
    rec = _records(w, scene)
    assert np.isfinite(rec["p"]).all()
    _check(w, rec, rng, 1024, "the bodies are back")
    w.set_counts(nb - 10, w.nbox, w.nsph)
    w.query_refit()
    _check(w, Q.records(w.get_bodies()["transforms"][: nb - 10], scene, w.nbox, w.nsph), rng, 1024, "NaN poses again")
    w.close()


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_abi_edge_cases():
    scene = S.pile(600, 300, seed=3)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    L = w.L
    bodies, colliders = C.byref(w.bodies), C.byref(w.colliders)
    assert L.nh_query_refit(w.ctx, bodies, colliders) == 1                    # before any build: NH_ERR_INVALID
    w.set_counts(nb, 10, 4)
    w.query_build()
    assert L.nh_query_refit(None, bodies, colliders) == 1                     # null arguments
    assert L.nh_query_refit(w.ctx, None, colliders) == 1
    assert L.nh_query_refit(w.ctx, bodies, None) == 1
    rng = np.random.default_rng(730)
    rec = _records(w, scene)
    b, ref, got = _check(w, rec, rng, 512, "built")
    for nbox, nsph in ((9, 4), (10, 5), (11, 3), (0, 14)):                    # another count is another world, the same total included
        w.set_counts(nb, nbox, nsph)
        assert L.nh_query_refit(w.ctx, bodies, colliders) == 1, (nbox, nsph)
    w.set_counts(nb, 10, 4)
    assert _differing(_gpu(w, b, ref), ref) == []                             # the refused calls changed nothing
    assert L.nh_query_refit(w.ctx, bodies, colliders) == 0                    # two refits in a row: NH_OK, the same answers
    assert L.nh_query_refit(w.ctx, bodies, colliders) == 0
    assert _differing(_gpu(w, b, ref), ref) == []
    w.step(3)
    w.query_refit()
    _check(w, _records(w, scene), rng, 512, "refit")
    # a growing build (more colliders than the buffers hold), then a refit of the new tree
    w.set_counts(nb, 601, 300)
    assert L.nh_query_refit(w.ctx, bodies, colliders) == 1
    w.query_build()
    st = w.query_stats()
    assert st["colliders"] == 901 and st["runs"] == 1 and st["top_nodes"] == 0
    w.step(3)
    w.query_refit()
    _check(w, _records(w, scene), rng, 512, "refit of the grown tree")
    w.close()


def test_a_tree_of_several_runs_has_a_top_phase():
    scene = S.grid_tiles(2, side=64, sphere_fraction=0.5, seed=2)
    w = E.World(scene, flags=FUSED)
    w.query_build()
    st = w.query_stats()
    assert st["colliders"] == w.nbox + w.nsph and st["runs"] == -(-st["colliders"] // st["run_length"]) and st["runs"] >= 7
    assert st["runs"] - 1 <= st["top_nodes"] and 1 <= st["top_depth"] <= st["top_nodes"], st
    rng = np.random.default_rng(735)
    _check(w, _records(w, scene), rng, 1024, "8194 colliders, built")
    for k in (1, 20):
        w.step(k)
        w.query_refit()
        _check(w, _records(w, scene), rng, 1024, f"8194 colliders, refit after {k}")
    assert w.query_stats() == st                                               # the tree is the build's
    w.close()


def test_a_refit_does_not_leak_into_the_next_build():
    scene = SMALL["pile"]()
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    a.query_build()
    for _ in range(30):
        a.step(1)
        a.query_refit()
        b.step(1)
    a.query_build()
    b.query_build()
    rec = _records(b, scene)
    assert rec.tobytes() == _records(a, scene).tobytes()
    batch, ref, got_b = _check(b, rec, np.random.default_rng(740), 2048, "the world that never refitted")
    got_a = _gpu(a, batch, ref)
    assert _differing(got_a, ref) == []
    for k in ("rays", "spheres", "boxes", "capsules", "points"):              # nh_closest's seed reads the key frame the refits left alone
        assert got_a[k].tobytes() == got_b[k].tobytes(), k
    a.close(); b.close()


# ---- observers ------------------------------------------------------------------------------------------------------------------------------
def _query(w, rays_t, hits_t):
    w.query_refit()
    w.raycast_records(rays_t, hits=hits_t)


@pytest.mark.parametrize("name", sorted(OBSERVED))
def test_refits_between_calls_change_nothing(name):
    scene = OBSERVED[name]()
    rays = _rays(np.random.default_rng(750), 4096, (-30, -12, -30), (30, 20, 30), "random")
    # between nh_step calls
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    rt = _upload(a, rays)
    ht = a.torch.empty((4096, 32), dtype=a.torch.uint8, device=a.dev)
    a.query_build()
    done = 0
    for k in [1, 2, 3, 5, 7, 4, 8] * 10:
        k = min(k, 300 - done)
        if k <= 0:
            break
        _query(a, rt, ht)
        a.step(k)
        b.step(k)
        done += k
    _query(a, rt, ht)
    _same_stepped_world(a, b, f"{name} nh_step")
    if name == "grid_tiles":
        assert a.counts()["still_steps"] > 0, a.counts()
    a.close(); b.close()
    # between every call of the fused step
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    rt = _upload(a, rays)
    ht = a.torch.empty((4096, 32), dtype=a.torch.uint8, device=a.dev)
    a.query_build()
    for s in range(300):
        for call in ("collide", "gravity", "read_cache", "setup", "apply", "update", "write_cache", "advance"):
            _query(a, rt, ht)
            getattr(a, call)()
            getattr(b, call)()
        a.step_done(); b.step_done()
    _query(a, rt, ht)
    _same_stepped_world(a, b, f"{name} call by call")
    if name == "grid_tiles":
        assert a.counts()["still_steps"] > 0, a.counts()
    a.close(); b.close()


# ---- at size --------------------------------------------------------------------------------------------------------------------------------
def test_a_refit_of_the_landed_config_2_world():
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED, max_contacts=6 * nb)
    w.step(60)
    w.query_build()
    w.step(10)
    assert w.counts()["error"] == 0
    w.query_refit()
    st = w.query_stats()
    print(f"\n[config 2] {st}")
    assert st["colliders"] == 1004524 and st["top_nodes"] >= st["runs"] - 1
    rec = Q.records(w.get_bodies()["transforms"], scene)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(760)
    n = 1 << 20
    rays = np.concatenate([_rays(rng, n // 2, lo, hi, "down"), _rays(rng, n // 4, lo, hi, "random"), _rays(rng, n - n // 2 - n // 4, lo, hi, "axis")])
    k = n // 4
    live = rec["p"][1 + 124:].astype(np.float64)
    near = live[rng.integers(0, len(live), size=k)] + rng.normal(scale=0.5, size=(k, 3))
    q = np.concatenate([TP._queries(near, 2.0), TP._queries(TP._points(rng, k, rec, lo, hi, "uniform")), TP._queries(TP._points(rng, k, rec, lo, hi, "above")),
                        TP._queries(TP._points(rng, n - 3 * k, rec, lo, hi, "inside"), rng.choice(np.float32([np.inf, 0.0, 0.5]), size=n - 3 * k))])
    pick = np.linspace(0, n - 1, 2048).astype(np.int64)
    ref_rays, ref_points = CAST.cast(CAST.RAY, rec, w.nbox, rays[pick]), HP.closest(rec, w.nbox, q[pick])
    assert (ref_rays["shape"] != NONE).mean() > 0.3 and (ref_points["shape"] != NONE).mean() > 0.5
    hits, near_hits = _cast(w, rays), TP._closest(w, q)
    _same_hits(hits[pick], ref_rays, "config 2, 1 M rays after a refit")
    TP._same_hits(near_hits[pick], ref_points, "config 2, 1 M closest points after a refit")
    w.query_build()
    hits2, near2 = _cast(w, rays), TP._closest(w, q)
    _same_hits(hits2[pick], ref_rays, "config 2, 1 M rays after the fresh build")
    TP._same_hits(near2[pick], ref_points, "config 2, 1 M closest points after the fresh build")
    assert hits2.tobytes() == hits.tobytes() and near2.tobytes() == near_hits.tobytes()      # the whole batches, refit against build
    w.close()
