"""The one-body solver's sweeps divide with the short sequences and take ONE verdict per body solve (nudge_amd/csrc/nh_solver.h: nh_div_deferred): a wave in
which some lane met an argument the short forms do not cover solves again from the start with the exact forms.  These tests put such arguments into the sweeps --
friction clamps whose reciprocal root has an argument in (0, 2^-64), exact zeros of both signs, one such body in a wave of ordinary ones -- and hold the still
path and the full-step path to the compiled reference, bit for bit (pytest -m gpu).  How many waves of these worlds solve again, per path, is recorded in
profiles/r08_deferred_verdict_ab.log.

Why the speeds: for a tangential speed t below 1e-3 at a contact the friction factor is capped at 1e6 (nudge.cpp:4759), so the contact's new friction impulse is
old - t^3 * 1e6.  A contact with no friction impulse to start from -- a fresh one, where a body lands -- and t in [4e-10, 6e-6] gives the clamp's root an argument
in (0, 2^-64)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402
from oracle import refworld                 # noqa: E402

pytestmark = pytest.mark.gpu

FLAGS = E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP
CASES = ["hops", "zeros", "one_lane"]


def _world(scene, still):
    if not still:
        os.environ["NH_NO_STILL"] = "1"
    try:
        return E.World(scene, flags=FLAGS)
    finally:
        os.environ.pop("NH_NO_STILL", None)


def _edit(momentum, case):
    v, w = momentum["velocity"], momentum["angular_velocity"]
    if case == "hops":                   # from rest, every 9th body hops and comes down on fresh contacts with a tiny sideways speed
        v[4::9, 1] = 1.0
        v[4::9, 0] = 1e-7
        v[8::18, 2] = -3e-8
    elif case == "zeros":                  # exact zeros of both signs: the short forms' own case, no replay
        v[1::3, 0] = 0.0
        v[1::3, 2] = -0.0
        w[2::3, :] = 0.0
        w[3::5, 1] = -0.0
    else:                                  # one body hops in a world at rest
        v[70, 1] = 1.0
        v[70, 0] = 1e-7
    return momentum


def scenario(case, still, ref):
    """The world (and the reference beside it when `ref`), the counters before the edit, and a generator of checkpoints: (steps done since the edit)."""
    scene = S.grid_tiles(1, side=32, seed=37)
    g = _world(scene, still)
    r = refworld.RefWorld(scene, max_contacts=8 * len(scene["body_transforms"])) if ref else None
    g.step(120)
    if r is not None:
        r.step(120)
    c0 = g.counts()
    m = _edit(g.get_bodies()["momentum"].copy(), case)
    g.set_bodies(momentum=m)
    if r is not None:
        r.set_bodies(momentum=m.copy())

    def checkpoints():
        done = 0
        for n in (2, 5, 10, 20, 30, 40):
            g.step(n - done)
            if r is not None:
                r.step(n - done)
            done = n
            yield n
    return g, r, c0, checkpoints()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("still", [True, False], ids=["still", "full"])
def test_short_divisions_that_fail_their_guard_are_solved_again_exactly(case, still):
    assert refworld.available("exact"), "oracle/_ref/libnudge_ref_exact.so did not travel to this box: the parity tests need the compiled reference"
    g, r, c0, cps = scenario(case, still, True)
    for n in cps:
        gb, rb = g.get_bodies(), r.bodies()
        assert P.bits_equal(gb["transforms"], rb["transforms"]), f"{case}, step {n}: transforms differ from the reference"
        for f in ("velocity", "angular_velocity"):
            assert P.bits_equal(gb["momentum"][f], rb["momentum"][f]), f"{case}, step {n}: {f} differs from the reference"
        assert np.array_equal(gb["idle"], rb["idle"])
    c = g.counts()
    assert c["error"] == 0
    if still:          # steps after the edit went through the still solver
        assert c["still_steps"] > c0["still_steps"], (c0, c)
    g.close()
