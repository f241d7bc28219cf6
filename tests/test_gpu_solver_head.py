"""The head of the still solver (k_solve_one_body<.., STILL>, nudge_amd/csrc/nh_solve.hip; pytest -m gpu).

A wave of the still solver asks for everything the launch alone addresses in ONE trip, before it knows whether the step stands: the words of the device state, body 0, one
entry of the step's change list per lane at a fixed index, the lane's record, tag-order position, collider and idle counter at a clamped body index, and the body's state.
Behind it, one more trip brings everything the record addresses.  What can go wrong with that is an index -- a lane past the last body, a record behind the box-box records,
a body without a record, a list entry that is not listed, a list longer than a wave, a list that overflows, a launch that must leave having read only what it may -- so these worlds are as small as
those cases allow (still steps need 65 colliders), are stepped in calls of 1, 2, 7 and 40 sub-steps and are compared bit for bit, after every call, with the same library
under option no_still: bodies, contacts, cache.  The counts of still steps, of steps that started at the solver and of still steps that did not happen are held to those of
the parent library (PARENT_COUNTS)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_pair_begin import CALLS, _same, _world                                   # noqa: E402
from test_gpu_spin_verdict import DELTA_MAX, LANDED, _calls, _edit, _pair, _slab_world          # noqa: E402

pytestmark = pytest.mark.gpu

# (still steps, steps that started at the solver, still steps that did not happen) of each script below over its calls, as the PARENT library (commit 18c1d35, loaded through
# NUDGE_HIP_LIBRARY) reports them -- profiles/r11_solver_head_ab.log, "tests".  Taken once from that build; the solver's head must not change which steps stand.
PARENT_COUNTS = {
    "100 boxes": (50, 46, 0),
    "99 boxes and a sphere": (50, 46, 0),
    "body 70 hovering": (98, 92, 1),
    "0 take off": (100, 92, 0),
    "1 take off": (97, 1, 4),
    "64 take off": (70, 12, 11),
    "65 take off": (70, 12, 11),
    "256 take off": (70, 12, 11),
    "320 take off": (65, 12, 11),
    "body 70 sliding": (4, 4, 13),
    "body 0 moving": (0, 0, 0),
    "96 of 255 asleep": (99, 87, 0),
}


def _held_to_parent(name, d):
    got = (d["still_steps"], d["pair_steps"], d["still_replays"])
    print(f"[solver head] {name!r}: {got},")
    assert got == PARENT_COUNTS[name], (name, got, PARENT_COUNTS[name])


def test_lanes_past_the_last_body():
    """100 boxes on a slab: 101 bodies, the second wave has 37 lanes on bodies and 27 past the end -- their body index, record and tag-order position are clamped."""
    a, c = _pair(_slab_world(100, sphere=False))
    d = _calls(a, c, "100 boxes")
    assert d["still_steps"] == sum(CALLS) and d["still_replays"] == 0, d
    _held_to_parent("100 boxes", d)
    a.close(); c.close()


def test_a_record_behind_the_box_box_records():
    """99 boxes and one sphere: the sphere's record sits behind `pairs` box-box records and owns ONE slot -- where it is takes `pairs`, a word of the first trip."""
    a, c = _pair(_slab_world(100, sphere=True))
    d = _calls(a, c, "99 boxes and a sphere")
    assert d["still_steps"] == sum(CALLS) and d["still_replays"] == 0, d
    _held_to_parent("99 boxes and a sphere", d)
    a.close(); c.close()


def test_a_body_without_a_record():
    """Body 70 of 100 hovers 3 cm over the slab when the records are laid out: its lane holds NH_BODY_REC_NONE and fetches its second trip at record 0, for nothing.
    It comes down inside the call of 7, and that still step does not happen."""
    a, c = _pair(_slab_world(100, sphere=True))
    _edit((a, c), lift=[70])
    d = _calls(a, c, "body 70 hovering", CALLS + CALLS)
    assert d["still_steps"] > 0 and d["still_replays"] >= 1, d
    _held_to_parent("body 70 hovering", d)
    a.close(); c.close()


HOP = 3.0
# (The change list a still solver reads must come from bodies that HAVE records: a body without one that gains contacts fails the step before any solver looks.  So resting
# boxes, four contacts and a record each, are sent straight up at 3 m/s, 2.5 cm a step.  The step that follows the edit lays the records out while they still touch; after
# it they are 2.5 cm up -- further than the narrowphase finds a contact ahead of a touch, which was measured at up to 1.2 cm and below 1.9, and well inside their inflated
# boxes, a 32nd of a grid cell -- so in the NEXT step every one of them goes from four contacts to none, its record stays, and that step's list has one entry per box.)


def _hop(worlds, bodies):
    for w in worlds:
        m = w.get_bodies()["momentum"].copy()
        m["velocity"][bodies] = np.asarray((0.0, HOP, 0.0), dtype=np.float32)
        w.set_bodies(momentum=m)


def _contacts_per_body(w, n):
    b = w.get_contacts()["bodies"]
    return np.bincount(b.reshape(-1), minlength=n + 1)[1:n + 1]          # (body 0 is everybody's partner)


@pytest.mark.parametrize("k", [0, 1, 64, 65, 256, 320])
def test_change_lists_of_every_length(k):
    """`k` of 576 resting boxes, picked all over the tag order, take off together (above): the still step in which they lose their contacts reads a change list of k
    entries -- none, one, a lane each of a whole wave (64), one more than the first trip brings (65: the wave takes a trip for the rest), as many as the list holds (256) --
    and every record behind one of them shifts its start by what the list says; with 320 the list overflows and that still step must fail.  Neither is hoped for: a
    context under no_still, stepped singly beside the others, shows how many records changed their count in that step, and the speculating context, stepped singly too
    and asked for its counters only (which leaves the still regime alone), shows that the step stood as a still step -- or, on overflow, that it did not."""
    n = 576
    scene = _slab_world(n, sphere=False)
    a, c = _pair(scene)
    r = _world(scene, env=["NH_NO_STILL"])
    r.step(LANDED)
    bodies = np.sort(np.random.default_rng(5).permutation(n)[:k] + 1)
    _hop((a, c, r), bodies)
    for w in (a, c, r):
        w.step(1)          # (the full step that lays the records out: the boxes still touch)
    was = _contacts_per_body(r, n)
    assert (was[bodies - 1] > 0).all(), was[bodies - 1]          # (every one of them has contacts, so a record)
    c0 = a.counts()
    for w in (a, c, r):
        w.step(1)          # (the step in which they lose them)
    c1 = a.counts()
    now = _contacts_per_body(r, n)
    changed = int((now != was).sum())
    took = (c1["still_steps"] - c0["still_steps"], c1["still_replays"] - c0["still_replays"])
    print(f"\n[solver head] {k} boxes take off: {changed} records changed their count in the step (no_still); (still steps, failed) of that step: {took}")
    assert changed == k and (now[bodies - 1] == 0).all(), (k, changed)          # (a list of exactly k entries)
    _same(a, c, f"{k} boxes take off: the step of the list")
    if k <= DELTA_MAX:
        assert took == (1, 0), (k, took)          # (a still step read that list, and stood)
    else:
        assert took[0] == 0 and took[1] >= 1, (k, took)          # (more than the list holds, and no count scan in a world this small: the still step failed)
    d = _calls(a, c, f"{k} of {n} boxes in the air", CALLS + CALLS)
    assert d["still_steps"] > 0, d
    _held_to_parent(f"{k} take off", d)
    a.close(); c.close()


def test_a_step_behind_a_failed_one_leaves_at_its_top():
    """A resting box sent sliding at 4 m/s leaves its inflated box some sub-steps into a call: that still step fails, and the solver already enqueued behind it -- which has
    asked for its whole first trip by the time it knows -- leaves having written nothing: bodies, contacts and cache as under no_still after every call."""
    a, c = _pair(_slab_world(100, sphere=True))
    _edit((a, c), kick=(70, 4.0))
    d = _calls(a, c, "body 70 sliding", CALLS + CALLS)
    assert d["still_steps"] > 0 and d["still_replays"] >= 1, d
    _held_to_parent("body 70 sliding", d)
    a.close(); c.close()


def test_body_zero_not_inert():
    """Body 0 carries a velocity.  This case does NOT run the still solver: the host sees in the full step's counters that body 0 is not inert and offers no still step
    (0 of 50, as on the parent), so the head's own check of body 0 -- for a body 0 that changes on the device, which no entry point does without telling the library -- is
    not reached by any script a caller can write.  What is checked is that nothing is launched and the bits are the full step's."""
    a, c = _pair(_slab_world(100, sphere=True))
    _edit((a, c), v0=(0.0, 0.0, 0.25))
    d = _calls(a, c, "body 0 moving")
    assert d["still_steps"] == 0, d
    _held_to_parent("body 0 moving", d)
    a.close(); c.close()


def test_a_whole_wave_asleep_next_to_a_mixed_wave():
    """Sleepers form.  255 boxes fall asleep; the caller wakes all but bodies 64..159: the solver's second workgroup (bodies 64..127) is asleep as a whole and leaves on its
    one early load, the third (128..191) is half asleep -- its sleeping lanes are nobody's, its waking lanes take both trips."""
    n = 255
    scene = _slab_world(n, sphere=False)
    a, c = _world(scene), _world(scene, env=["NH_NO_STILL"])
    for w in (a, c):
        w.step(420)
        assert w.counts()["active_bodies"] == 0, "the world was meant to be asleep"
        idle = w.get_bodies()["idle"].copy()
        awake = np.ones(n + 1, dtype=bool)
        awake[0] = False; awake[64:160] = False
        idle[awake] = 0
        w.set_bodies(idle=idle)
    c0 = a.counts()
    done = 0
    for k in CALLS + CALLS:
        a.step(k); c.step(k)
        done += k
        what = f"96 of {n} asleep: call of {k}, step {done}"
        _same(a, c, what)
        ka, kc = a.get_contacts(), c.get_contacts()
        assert np.array_equal(ka["sleeping_pairs"], kc["sleeping_pairs"]), f"{what}: sleeping pairs differ"
        assert np.array_equal(a.get_active(), c.get_active()), f"{what}: active bodies differ"
        idle = a.get_bodies()["idle"]
        assert (idle[64:160] == 0xff).all() and (idle[1:64] != 0xff).all() and (idle[160:] != 0xff).all(), what
    c1 = a.counts()
    d = {k: c1[k] - c0[k] for k in ("still_steps", "pair_steps", "still_replays")}
    assert c1["error"] == 0 and c.counts()["still_steps"] == 0, c1
    assert d["still_steps"] > 0 and 0 < c1["active_bodies"] < n and c1["sleeping_pairs"] > 0, (d, c1)
    _held_to_parent("96 of 255 asleep", d)
    a.close(); c.close()
