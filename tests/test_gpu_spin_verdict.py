"""The verdict of a still step taken by spin, in worlds where steps fail inside a call (nh_still_await_number, nudge_amd/csrc/nh_step.hip; pytest -m gpu).

Inside nh_step the host enqueues a still step's solver and only then takes the verdict of the step before it from the number that step's solver left in its pinned ring
slot; a step that failed did nothing, nor did the one enqueued behind it, and both are run again.  Small worlds in which that happens -- a body that lands inside a call, a
change list that overflows because 576 boxes come down in one step, a body sent sliding out of its inflated box -- and worlds of 64, 65 and 100 bodies at rest (a full wave,
a second wave with one lane, lanes past the end), each with a sphere's record behind the box-box records, are stepped in calls of 1, 2, 7 and 40 sub-steps and compared bit
for bit, after every call, with the same library under option no_still.  Worlds of fewer than 64 dynamic bodies are not here: the library was seen to start no still step in
them (0 of 100 with 1, 2 and 63 bodies), so they cannot reach the code this file is about."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_pair_begin import CALLS, _same, _world          # noqa: E402
from nudge_amd import scenes as S                            # noqa: E402

pytestmark = pytest.mark.gpu

LANDED = 100
DELTA_MAX = 256          # NH_DELTA_MAX (nh_internal.h): entries of a step's list of changed contact counts


def _slab_world(n, sphere=True, seed=7):
    """`n` dynamic bodies over one slab, cut out of a mixed drop tile: boxes, and (n >= 2, `sphere`) one sphere as the LAST body -- its record sits behind the box-box
    records in tag order.  Body 0 is the static world."""
    side = int(np.ceil(np.sqrt(2 * n + 2)))
    src = S.grid_tiles(1, side=side, sphere_fraction=0.5, seed=seed)
    nsph = 1 if (sphere and n >= 2) else 0
    nbox = n - nsph
    ns = int((src["box_transforms"]["body"] == 0).sum())
    nb_src = len(src["box_tags"]) - ns
    assert nbox <= nb_src and nsph <= len(src["sphere_tags"])
    bodies = np.concatenate([[0], 1 + np.arange(nbox), 1 + nb_src + np.arange(nsph)]).astype(np.int64)
    scene = dict(src)
    for k in ("body_transforms", "body_properties", "body_momentum", "idle_counters"):
        scene[k] = src[k][bodies].copy()
    for k in ("box_tags", "box_data", "box_transforms"):
        scene[k] = src[k][:ns + nbox].copy()
    for k in ("sphere_tags", "sphere_data", "sphere_transforms"):
        scene[k] = src[k][:nsph].copy()
    scene["sphere_transforms"]["body"] = nbox + 1 + np.arange(nsph, dtype=np.uint32)
    scene["sphere_tags"] = (ns + nbox + np.arange(nsph)).astype(np.uint32)
    scene.pop("tile_of_body", None); scene.pop("tile_of_static", None)
    scene["name"] = f"slab{n}"
    return scene


def _pair(scene):
    a, c = _world(scene), _world(scene, env=["NH_NO_STILL"])
    for w in (a, c):
        w.step(LANDED)
    _same(a, c, "landed")
    return a, c


def _edit(worlds, lift=(), dy=0.03, kick=None, v0=None):
    """On landed worlds: the bodies of `lift` raised by `dy` and left there at rest; body `kick` = (index, vx) sent sliding; body 0 given the velocity `v0`.  The idle
    counters are handed over unchanged, so the library is told (nh_bodies_changed) and lays its records out in a full step."""
    for w in worlds:
        bd = w.get_bodies()
        t, m = bd["transforms"].copy(), bd["momentum"].copy()
        for k in lift:
            t["position"][k][1] += np.float32(dy)
            m["velocity"][k] = 0
            m["angular_velocity"][k] = 0
        if kick is not None:
            m["velocity"][kick[0]][0] = np.float32(kick[1])
        if v0 is not None:
            m["velocity"][0] = np.asarray(v0, dtype=np.float32)
        w.set_bodies(transforms=t, momentum=m, idle=bd["idle"].copy())


def _calls(a, c, what, calls=CALLS):
    c0 = a.counts()
    done = 0
    for n in calls:
        a.step(n); c.step(n)
        done += n
        _same(a, c, f"{what}: call of {n}, step {done}")
    c1 = a.counts()
    d = {k: c1[k] - c0[k] for k in ("still_steps", "pair_steps", "still_replays")}
    print(f"\n[spin verdict] {what}: {d} in {done} steps")
    assert c1["error"] == 0 and c.counts()["still_steps"] == 0, (what, c1)
    return d


@pytest.mark.parametrize("n", [64, 65, 100])
def test_worlds_at_rest_with_a_record_behind_the_boxes(n):
    """(i) 64, 65 and 100 bodies at rest (a full wave; a second wave with one lane; lanes past the end), the last of them a sphere: every step of every call is a still
    step whose verdict the host took by spin, and the bits are the full step's."""
    a, c = _pair(_slab_world(n))
    d = _calls(a, c, f"{n} bodies at rest", CALLS + CALLS)
    assert d["still_steps"] == 2 * sum(CALLS) and d["still_replays"] == 0, d
    a.close(); c.close()


def test_a_body_without_a_record_lands_inside_a_call():
    """(ii) Body 1 of 65 hovers 3 cm over the slab when the records are laid out -- its kept pair has no contact, the body no record -- and comes down five steps later,
    inside the call of 7: its count goes 0 -> 4, every record behind it in tag order shifts through the change list, and the still step it happens in fails."""
    a, c = _pair(_slab_world(65))
    _edit((a, c), lift=[1])
    d = _calls(a, c, "65 bodies, body 1 hovering", CALLS + CALLS)
    assert d["still_steps"] > 0 and d["still_replays"] >= 1, d
    a.close(); c.close()


def test_more_changes_in_one_step_than_the_list_holds():
    """(iii) 576 boxes released from the same 50 cm.  They arrive at 3 m/s, 2.6 cm per step, so most of them touch down in the same step: more than NH_DELTA_MAX counts
    change at once (shown on a third context under no_still, stepped one step at a time), the list overflows, the still step behind it does not happen, and the world
    comes out as under no_still.  (Released from 3 cm the same boxes land over four steps, 137 records at most in one: the list holds that.)"""
    n = 576
    scene = _slab_world(n, sphere=False)
    a, c = _pair(scene)
    r = _world(scene, env=["NH_NO_STILL"])
    r.step(LANDED)
    _edit((a, c, r), lift=range(1, n + 1), dy=0.5)
    per_step = [r.get_contacts()["count"]]
    for _ in range(60):
        r.step(1)
        per_step.append(r.get_contacts()["count"])
    r.close()
    most = max(y - x for x, y in zip(per_step[:-1], per_step[1:]))
    print(f"\n[spin verdict] released together, contacts step by step (no_still): {per_step}")
    assert most > 4 * DELTA_MAX, per_step          # (four contacts per box: more than NH_DELTA_MAX records went 0 -> 4 in ONE step)
    d = _calls(a, c, f"{n} boxes released together", CALLS + CALLS)
    assert d["still_steps"] > 0 and d["still_replays"] >= 1, d          # (still steps while the boxes fall, and the one behind the overflow did not happen)
    a.close(); c.close()


def test_a_step_that_fails_inside_a_call_writes_nothing():
    """(iv) A resting box is sent sliding at 4 m/s before the calls: some sub-steps into a call it leaves its inflated box, that still step fails, and the solver the
    host has already enqueued behind it leaves at its top: bodies, contacts and cache as under no_still after every call."""
    a, c = _pair(_slab_world(65))
    _edit((a, c), kick=(1, 4.0))
    d = _calls(a, c, "body 1 sliding", CALLS + CALLS)
    assert d["still_steps"] > 0 and d["still_replays"] >= 1, d          # (a step did fail inside a call, with still steps around it)
    a.close(); c.close()


def test_body_zero_not_inert():
    """(v) Body 0 carries a velocity when the records are laid out: the host sees in that full step's counters that body 0 is not inert and never starts a still step
    (the solver's own check of body 0 is for a body 0 that changes on the device, which no entry point does without telling the library); the bits are the full step's."""
    a, c = _pair(_slab_world(65))
    _edit((a, c), v0=(0.0, 0.0, 0.25))
    d = _calls(a, c, "body 0 moving")
    assert d["still_steps"] == 0, d
    a.close(); c.close()
