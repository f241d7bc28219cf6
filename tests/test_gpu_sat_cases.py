"""Crafted box-box worlds for every branch of the narrowphase SAT (nudge_amd/csrc/nh_narrowphase.h: nh_box_box_eval), on the GPU, bit for bit
against the compiled reference and, for the still path, the solver's next-step narrowphase (pair ahead) against the launched one:

  * boxes resting on each of their three face axes, so that a_face and b_face take 0, 1 and 2 in both roles (sizes differ per axis);
  * exact quarter turns (quaternions with components 0, +-0.5, +-1), which give +-0 entries in the relative rotation, the clip's edge
    slopes (1 / +-0 = +-inf) and its z-plane denominator;
  * rotations whose edge-axis lengths straddle the reference's 1e-3 NaN threshold;
  * tilted boxes falling onto the slab and onto each other (edge-edge contacts)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_util as P                      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from oracle import refworld                 # noqa: E402
from sat_cases_util import CASES, sat_world   # noqa: E402

pytestmark = pytest.mark.gpu
FAST = E.NH_FLAG_SYNC_COUNTS
EXACT = E.NH_FLAG_SYNC_COUNTS | E.NH_FLAG_EXACT_ORDER
BENCH_FLAGS = E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP



def _needs_ref():
    assert refworld.available("exact"), "oracle/_ref/libnudge_ref_exact.so did not travel to this box: the SAT cases need the compiled reference"


@pytest.mark.parametrize("case", CASES + ["random"])
def test_sat_contacts_match_reference(case):
    """The contacts of one collide() -- positions, normals, penetrations, feature tags, order -- at several points of the run, against the reference."""
    _needs_ref()
    scene = sat_world(case)
    ref = refworld.RefWorld(scene)
    w = E.World(scene, flags=FAST)
    done, seen = 0, 0
    for warm in (0, 1, 5, 20, 60, 150):
        ref.step(warm - done)
        done = warm
        b = ref.bodies()
        w.set_bodies(b["transforms"], b["momentum"], b["idle"])
        ref.collide()
        w.collide()
        od, ob, ok, of, _ = P.oracle_contacts_sorted(ref.contacts())
        c = w.get_contacts()
        assert c["count"] == len(ok), (case, warm)
        assert np.array_equal(c["tags"], ok) and np.array_equal(c["features"], of) and np.array_equal(c["bodies"], ob), (case, warm)
        assert P.bits_equal(c["data"], od), (case, warm)
        seen += len(ok)
    assert seen > 0
    w.close()


@pytest.mark.parametrize("case", CASES + ["random"])
def test_sat_worlds_step_like_reference(case):
    _needs_ref()
    scene = sat_world(case)
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


def _world(scene, env=()):
    for k in env:
        os.environ[k] = "1"
    try:
        return E.World(scene, flags=BENCH_FLAGS)
    finally:
        for k in env:
            os.environ.pop(k, None)


def _same_world(a, b, what):
    ba, bb = a.get_bodies(), b.get_bodies()
    assert P.bits_equal(ba["transforms"], bb["transforms"]), f"{what}: transforms differ"
    assert P.bits_equal(ba["momentum"], bb["momentum"]), f"{what}: momentum differs"
    assert np.array_equal(ba["idle"], bb["idle"]), f"{what}: idle counters differ"
    ka, kb = a.get_contacts(), b.get_contacts()
    assert ka["count"] == kb["count"], f"{what}: contact count"
    assert np.array_equal(ka["tags"], kb["tags"]) and np.array_equal(ka["features"], kb["features"]), f"{what}: contact identities differ"
    assert P.bits_equal(ka["data"], kb["data"]), f"{what}: contact data differ"


@pytest.mark.parametrize("case", CASES)
def test_sat_pair_ahead_matches_launched_narrowphase(case):
    """nh_step with the solver evaluating each body's pair for the next sub-step (pair ahead) against option no_pair_ahead, bit for bit."""
    scene = sat_world(case)
    a, b = _world(scene), _world(scene, env=["NH_NO_PAIR_AHEAD"])
    done = 0
    for cp in (1, 10, 40, 41, 45, 80, 120, 200):
        a.step(cp - done); b.step(cp - done)
        done = cp
        _same_world(a, b, f"{case}, step {cp}")
    assert a.counts()["error"] == 0 and b.counts()["error"] == 0
    a.close(); b.close()
