"""The prologue of a still step that starts at the solver (k_pair_begin, nudge_amd/csrc/nh_collide.hip) and the ring events behind it (pytest -m gpu).

k_pair_begin does the step-wide checks and evaluates the kept pairs that are NO body's own: two neighbours whose inflated boxes overlap, a box hovering over ground it does
not touch yet.  Worlds that hold both kinds are stepped in calls of several lengths and compared bit for bit with the same library without pair ahead (the narrowphase
evaluates those pairs) and without still steps; a landing inside a call must be seen in the step in which it happens; and which way the call's last verdict reaches the
host -- the early-counter spin, the ring event, a round trip in every step -- must not show."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

FLAGS = E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP
SIDE = 12
CALLS = (1, 2, 7, 40)

# (ii): still steps that did not happen (failed, or launched behind one that failed) in the landing sequence below, as the PARENT library (commit 8f1c5f4, loaded through
# NUDGE_HIP_LIBRARY) reports them on this world -- profiles/r09_steady_step_ab.log, "tests".  k_pair_begin must fail the steps the old prologue failed, no more, no fewer.
PARENT_REPLAYS = 4


def _world(scene, flags=FLAGS, env=()):
    for k in env:
        os.environ[k] = "1"
    try:
        return E.World(scene, flags=flags)
    finally:
        for k in env:
            os.environ.pop(k, None)


def _same(a, b, what):
    ba, bb = a.get_bodies(), b.get_bodies()
    assert P.bits_equal(ba["transforms"], bb["transforms"]), f"{what}: transforms differ"
    assert P.bits_equal(ba["momentum"], bb["momentum"]), f"{what}: momentum differs"
    assert np.array_equal(ba["idle"], bb["idle"]), f"{what}: idle counters differ"
    ca, cb = a.get_cache(), b.get_cache()
    assert ca["count"] == cb["count"], f"{what}: cache count {ca['count']} vs {cb['count']}"
    assert np.array_equal(ca["tags"], cb["tags"]) and np.array_equal(ca["features"], cb["features"]), f"{what}: cache tags differ"
    assert P.bits_equal(ca["data"]["impulse"], cb["data"]["impulse"]), f"{what}: cached impulses differ"
    ka, kb = a.get_contacts(), b.get_contacts()
    assert ka["count"] == kb["count"], f"{what}: contact count"
    assert np.array_equal(ka["tags"], kb["tags"]) and np.array_equal(ka["features"], kb["features"]) and np.array_equal(ka["bodies"], kb["bodies"]), f"{what}: contact identities differ"
    assert P.bits_equal(ka["data"], kb["data"]), f"{what}: contact data differ"
    na, nb = a.counts(), b.counts()
    for k in ("contacts", "sleeping_pairs", "active_bodies", "cache", "error"):
        assert na[k] == nb[k], f"{what}: counter {k}: {na[k]} vs {nb[k]}"


def _half_x(q, size):
    """Half extent along x of the world AABB of a box with half extents `size` and rotation q = (x, y, z, w)."""
    x, y, z, w = (float(v) for v in q)
    r0 = (1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w))
    return sum(abs(r) * float(s) for r, s in zip(r0, size))


B_BODY, A_BODY = 1 + 5 * SIDE + 5, 1 + 5 * SIDE + 6          # two neighbours in tile 0
H_BODY = 1 + SIDE * SIDE + 2 * SIDE + 6                        # the box that hovers, tile 1
D_BODY = 1 + 8 * SIDE + 2                                      # the box that is dropped, tile 0
LANDED = 100


def _scene():
    """Two 12 x 12 drop tiles in which box A starts 2 cm (between the world AABBs) beside its neighbour B: they land side by side, their inflated boxes overlap for good,
    nothing touches -- a kept pair that is no body's own in every layout."""
    scene = S.grid_tiles(2, side=SIDE, seed=91, lattice_cols=2)
    size = _box_sizes(scene)
    t = scene["body_transforms"]
    gap = _half_x(t["rotation"][A_BODY], size[A_BODY]) + _half_x(t["rotation"][B_BODY], size[B_BODY]) + 0.02
    t["position"][A_BODY][0] = np.float32(float(t["position"][B_BODY][0]) + gap)
    t["position"][A_BODY][2] = t["position"][B_BODY][2]
    return scene


def _arrange(worlds, drop=0.0):
    """On landed worlds: box H is lifted 3 cm off the ground it rested on and left there without velocity (and with `drop` box D that far).  The idle counters are handed
    over with it (unchanged), so the library is told (nh_bodies_changed) and lays the records out in a full step WHILE H hovers: its kept pair with the ground has no
    contact and is no body's own -- k_pair_begin's to evaluate in the steps that start at the solver, until the box is down (3 cm: five steps)."""
    for w in worlds:
        bd = w.get_bodies()
        t, m = bd["transforms"].copy(), bd["momentum"].copy()
        t["position"][H_BODY][1] += np.float32(0.03)
        moved = [H_BODY]
        if drop:
            t["position"][D_BODY][1] += np.float32(drop)
            moved.append(D_BODY)
        for k in moved:
            m["velocity"][k] = 0
            m["angular_velocity"][k] = 0
        w.set_bodies(transforms=t, momentum=m, idle=bd["idle"].copy())


def _box_sizes(scene):
    """Half extents of every dynamic body's one box, by body index (grid_tiles without spheres: the static slabs' boxes come first and sit on body 0)."""
    body = scene["box_transforms"]["body"]
    size = np.zeros((len(scene["body_transforms"]), 3), dtype=np.float32)
    size[body[body > 0]] = scene["box_data"]["size"][body > 0]
    assert (size[1:] > 0).all()
    return size


def test_pairs_that_are_nobodys_through_calls_of_every_length():
    """(i) A landed world with a box hovering over the ground and two neighbours within each other's inflated boxes, in nh_step calls of 1, 2, 7 and 40 sub-steps (twice:
    the hovering box comes down inside the first call of 7, which k_pair_begin has to see): the bits of the library with option no_pair_ahead and of the one that
    never speculates; and the default run does start steps at the solver."""
    scene = _scene()
    a, b, c = _world(scene), _world(scene, env=["NH_NO_PAIR_AHEAD"]), _world(scene, env=["NH_NO_STILL"])
    for w in (a, b, c):
        w.step(LANDED)
    _same(a, b, "landed (no_pair_ahead)"); _same(a, c, "landed (no_still)")
    _arrange((a, b, c))
    c0 = a.counts()
    done = 0
    for n in CALLS + CALLS:
        for w in (a, b, c):
            w.step(n)
        done += n
        _same(a, b, f"call of {n}, step {done} (pair ahead vs narrowphase launched)"); _same(a, c, f"call of {n}, step {done} (pair ahead vs never speculating)")
    c1 = a.counts()
    print(f"\n[pair begin, calls] pair {c1['pair_steps'] - c0['pair_steps']} of {c1['still_steps'] - c0['still_steps']} still steps in {done}; replays {c1['still_replays'] - c0['still_replays']}")
    assert c1["error"] == 0 and c1["pair_steps"] > c0["pair_steps"], (c0, c1)
    # (the hovering box's pair is on k_pair_begin's list and nobody else evaluates it in a step that starts at the solver: its landing fails exactly such a step.  Without
    # a listed pair that a pair lane evaluated there is no replay here, and the test would not have run the code it is about)
    assert c1["still_replays"] - c0["still_replays"] >= 1, (c0, c1)
    assert b.counts()["pair_steps"] == 0 and c.counts()["still_steps"] == 0
    a.close(); b.close(); c.close()


def test_a_landing_inside_a_call_is_seen_in_its_step():
    """(ii) The same world with one more box lifted, by 5 cm: both come down inside the 20-step call.  The bits of the library that never speculates after every
    call, and as many still steps failed or replayed as the parent library reports on this world."""
    scene = _scene()
    a, c = _world(scene), _world(scene, env=["NH_NO_STILL"])
    for w in (a, c):
        w.step(LANDED)
    _arrange((a, c), drop=0.05)
    c0 = a.counts()
    done = 0
    for n in (3, 20, 10):
        a.step(n); c.step(n)
        done += n
        _same(a, c, f"call of {n}, step {done}")
    c1 = a.counts()
    replays = c1["still_replays"] - c0["still_replays"]
    print(f"\n[pair begin, landing] replays {replays}; pair {c1['pair_steps'] - c0['pair_steps']} of {c1['still_steps'] - c0['still_steps']} still steps in {done}")
    assert c1["error"] == 0 and c1["pair_steps"] > c0["pair_steps"], (c0, c1)
    assert replays == PARENT_REPLAYS, (replays, PARENT_REPLAYS)
    a.close(); c.close()


def test_the_way_the_last_verdict_is_read_does_not_show():
    """(iii) The last verdict of a call read through the early-counter spin (default), through the ring event alone (option no_early_counts: the fallback) and by a round
    trip in every step (NH_FLAG_SYNC_COUNTS): same bits after every call."""
    scene = _scene()
    a, e, s = _world(scene), _world(scene), _world(scene, flags=FLAGS | E.NH_FLAG_SYNC_COUNTS)
    e.set_option("no_early_counts", 1)
    for w in (a, e, s):
        w.step(LANDED)
    _arrange((a, e, s))
    done = 0
    for n in CALLS + CALLS:
        for w in (a, e, s):
            w.step(n)
        done += n
        _same(a, e, f"call of {n}, step {done} (spin vs event)"); _same(a, s, f"call of {n}, step {done} (spin vs a round trip per step)")
    assert a.counts()["error"] == 0 and a.counts()["pair_steps"] > 0 and e.counts()["pair_steps"] > 0
    a.close(); e.close(); s.close()
