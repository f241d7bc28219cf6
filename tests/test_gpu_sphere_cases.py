"""The crafted sphere worlds of tests/sphere_cases_util.py on the GPU, bit for bit against the compiled reference: every branch of nh_sphere_sphere and
nh_box_sphere (nudge_amd/csrc/nh_narrowphase.h) with the short device reciprocal wired in, the role handling of the three call sites (k_narrowphase, the listed
pairs of the still narrowphase, the solver's pair ahead), sphere colliders on the static body, and -- in the DIRECT search, option no_kept_pairs -- the
surely-apart skip of nh_collide.hip: no pair the reference gives a contact may go missing, however close to the boundary, far from the origin or unequal in size."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                      # noqa: E402
import sphere_cases_util as U                # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from oracle import refworld                 # noqa: E402
from test_gpu_sat_cases import EXACT, FAST, _needs_ref, _same_world, _world       # noqa: E402

pytestmark = pytest.mark.gpu
LATER = (1, 2, 5, 20)


@pytest.mark.parametrize("search", ["kept_pairs", "direct"])
@pytest.mark.parametrize("case", U.CASES)
def test_sphere_contacts_match_reference(case, search):
    """The contacts of one collide() at step 0 and at a few later steps of the reference's run, against the reference; with the default broadphase and with the
    DIRECT search (option no_kept_pairs), which searches at every collide() and drops pairs of awake spheres it finds surely apart."""
    _needs_ref()
    scene = U.sphere_world(case)
    ref = refworld.RefWorld(scene)
    for k in (["NH_NO_KEPT_PAIRS"] if search == "direct" else []):
        os.environ[k] = "1"
    try:
        w = E.World(scene, flags=FAST)
    finally:
        os.environ.pop("NH_NO_KEPT_PAIRS", None)
    done, seen = 0, 0
    for n, warm in enumerate((0,) + LATER):
        ref.step(warm - done)
        done = warm
        b = ref.bodies()
        w.set_bodies(b["transforms"], b["momentum"], b["idle"])
        ref.collide()
        w.collide()
        od, ob, ok, of, _ = P.oracle_contacts_sorted(ref.contacts())
        if warm == 0:
            print(f"\n[{case}, {search}] pairs (reference gives a contact, gives none):", U.check_straddles(case, scene, ok, od))
        c = w.get_contacts()
        if case == "ss_grazing":
            missing = U.contact_pairs(ok) - U.contact_pairs(c["tags"])
            assert not missing, f"{case}, {search}, step {warm}: pairs the reference gives a contact have none here: {sorted(missing)}"
        assert c["count"] == len(ok), (case, search, warm)
        assert np.array_equal(c["tags"], ok) and np.array_equal(c["features"], of) and np.array_equal(c["bodies"], ob), (case, search, warm)
        assert P.bits_equal(c["data"], od), (case, search, warm)
        seen += len(ok)
        counts = w.counts()
        assert counts["error"] == 0
        if search == "direct":
            assert counts["broadphase_rebuilds"] == n + 1, (counts["broadphase_rebuilds"], n + 1)          # (it searched, this time too)
    assert seen > 0
    if search == "direct" and case == "ss_grazing":
        # the spheres of radius 30 were members of the grid, where the skip is applied (sphere_cases_util._ss_grazing)
        print(f"[{case}, {search}] large colliders: {counts['large_colliders']}")
        assert counts["large_colliders"] < 60, counts
    w.close()


@pytest.mark.parametrize("case", U.CASES)
def test_sphere_worlds_step_like_reference(case):
    _needs_ref()
    scene = U.sphere_world(case)
    ref = refworld.RefWorld(scene)
    w = E.World(scene, flags=EXACT)
    for _ in range(3):
        w.step(40); ref.step(40)
        a, b = w.get_bodies(), ref.bodies()
        assert w.counts()["error"] == 0
        assert P.bits_equal(a["transforms"], b["transforms"]), case
        assert P.bits_equal(a["momentum"]["velocity"], b["momentum"]["velocity"]), case
        assert np.array_equal(a["idle"], b["idle"]), case
    w.close()


def test_sphere_pair_ahead_and_still_match_full_steps():
    """nh_step with the bench flags on "rest" -- a world at rest from its first step, with bodies whose only partner is a static SPHERE (a sphere and a box
    balanced on the apex of one) and listed pairs that never touch (a resting sphere beside a static sphere, two resting spheres side by side) -- against option
    no_pair_ahead (every still step launches its narrowphase) and against option no_still (every step a full one): bodies, contact identities and contact data,
    at checkpoints from the first step across the moment the world goes still and on into sleep.  The default world must have taken still steps, and its solver
    must have evaluated pairs ahead (observed: 253 still steps of 300, 243 of them pair steps, 2 replays).
    Static spheres do not keep a world from still steps.  What does is its size: with fewer than 65 colliders k_grid_setup keeps every collider out of the grid
    (its budget of large colliders), the cell and with it the margin of the kept pair list are tiny, every resting body leaves its inflated box every step and the
    list is rebuilt -- a first, 26-body form of "rest" took no still step for that reason.  A consequence of the budget, not a refusal written down anywhere; such a
    world is a few launches either way, so "rest" carries a field of resting bodies instead."""
    scene = U.sphere_world("rest")
    a, b, c = _world(scene), _world(scene, env=["NH_NO_PAIR_AHEAD"]), _world(scene, env=["NH_NO_STILL"])
    done = 0
    for cp in (1, 2, 3, 5, 10, 40, 41, 45, 80, 120, 200, 300):
        for w in (a, b, c):
            w.step(cp - done)
        done = cp
        _same_world(a, b, f"rest, step {cp}, against no_pair_ahead")
        _same_world(a, c, f"rest, step {cp}, against no_still")
    ca, cb, cc = a.counts(), b.counts(), c.counts()
    print(f"\n[rest] still steps {ca['still_steps']} (replays {ca['still_replays']}, pair steps {ca['pair_steps']}); no_pair_ahead: {cb['still_steps']} still, {cb['pair_steps']} pair steps; "
          f"no_still: {cc['still_steps']}; pair diag {[ca[k] for k in ('pair_diag_roles', 'pair_diag_record', 'pair_diag_scale', 'pair_diag_owned')]}")
    assert ca["error"] == 0 and cb["error"] == 0 and cc["error"] == 0
    assert cc["still_steps"] == 0
    assert ca["still_steps"] > 0 and cb["still_steps"] > 0, (ca, cb)
    assert ca["pair_steps"] > 0 and cb["pair_steps"] == 0, (ca, cb)          # (the solver did evaluate pairs ahead -- the static spheres' among them)
    if refworld.available("exact"):
        r = refworld.RefWorld(scene)
        r.step(done)
        rb, gb = r.bodies(), a.get_bodies()
        assert P.bits_equal(gb["transforms"], rb["transforms"]) and P.bits_equal(gb["momentum"]["velocity"], rb["momentum"]["velocity"])
        assert np.array_equal(gb["idle"], rb["idle"])
    for w in (a, b, c):
        w.close()
