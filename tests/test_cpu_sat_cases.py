"""The crafted SAT worlds of tests/sat_cases_util.py through the host build of the narrowphase (tests/hostsim: nh_narrowphase.h compiled by g++),
contacts bit for bit against the compiled reference.  The host build takes the exact division and root forms, so this checks the restructuring of
nh_box_box_eval (per-lane selects, late permutation of the clip candidates); the short device forms are checked by tests/test_gpu_sat_cases.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostsim_util as H                    # noqa: E402
import parity_util as P                     # noqa: E402
from oracle import refworld                 # noqa: E402
from sat_cases_util import CASES, sat_world   # noqa: E402

needs_ref = pytest.mark.skipif(not refworld.available("exact"), reason="oracle/_ref not built (needs the reference sources: make -C oracle)")


@needs_ref
@pytest.mark.parametrize("case", CASES + ["random"])
def test_sat_cases_host_narrowphase_bit_exact(case):
    scene = sat_world(case)
    w = refworld.RefWorld(scene)
    done, seen = 0, 0
    for warm in (0, 1, 5, 20, 60, 150):
        w.step(warm - done)
        done = warm
        b = w.bodies()
        w.collide()
        od, ob, ok, of, _ = P.oracle_contacts_sorted(w.contacts())
        h = H.collide(b["transforms"], scene)
        assert h["count"] == len(ok), (case, warm)
        assert np.array_equal(h["keys"], ok) and np.array_equal(h["features"], of), (case, warm)
        assert np.array_equal(h["bodies"], ob), (case, warm)
        assert P.bits_equal(h["data"], od), (case, warm)
        seen += len(ok)
    assert seen > 0
