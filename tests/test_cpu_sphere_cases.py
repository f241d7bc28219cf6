"""The crafted sphere worlds of tests/sphere_cases_util.py through the host build of the narrowphase (tests/hostsim: nh_narrowphase.h compiled by g++), contacts
bit for bit against the compiled reference: every branch of nh_sphere_sphere and nh_box_sphere, spheres on the static body included.  The host build takes the
exact reciprocal, so this checks the branches and the roles of the two functions; the short device reciprocal as wired into them, the role handling of the three
device call sites and the surely-apart skip of the DIRECT search are checked by tests/test_gpu_sphere_cases.py.  The boundary families of the util are checked
here on the reference alone (check_straddles)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostsim_util as H                    # noqa: E402
import parity_util as P                     # noqa: E402
import sphere_cases_util as U               # noqa: E402
from oracle import refworld                 # noqa: E402

needs_ref = pytest.mark.skipif(not refworld.available("exact"), reason="oracle/_ref not built (needs the reference sources: make -C oracle)")
LATER = {"ss_grazing": (), "ss_deep": (1, 2, 5, 20), "bs_faces": (1, 2, 5, 20), "rest": ()}


def test_sphere_worlds_are_well_formed():
    """No dynamic body without a collider, one collider per dynamic body, static spheres on body 0, a few hundred bodies at most."""
    for case in U.CASES:
        scene = U.sphere_world(case)
        nb = len(scene["body_transforms"])
        owners = np.concatenate([scene["box_transforms"]["body"], scene["sphere_transforms"]["body"]])
        assert np.array_equal(np.sort(owners[owners != 0]), np.arange(1, nb)), case
        assert nb <= 500, (case, nb)
        assert (scene["sphere_transforms"]["body"] == 0).any(), case
        tags = np.concatenate([scene["box_tags"], scene["sphere_tags"]])
        assert np.array_equal(tags, np.arange(len(tags))), case
        for prs in scene["groups"].values():
            assert all(0 <= a < len(tags) and 0 <= b < len(tags) and a != b for a, b in prs), case


@needs_ref
@pytest.mark.parametrize("case", U.CASES)
def test_sphere_cases_host_narrowphase_bit_exact(case):
    scene = U.sphere_world(case)
    w = refworld.RefWorld(scene)
    done, seen = 0, 0
    for warm in (0,) + LATER[case]:
        w.step(warm - done)
        done = warm
        b = w.bodies()
        w.collide()
        od, ob, ok, of, _ = P.oracle_contacts_sorted(w.contacts())
        assert np.isfinite(od.view(np.float32)).all(), (case, warm)          # (a world in which the reference itself gives NaN or infinity proves nothing)
        if warm == 0:
            print(case, U.check_straddles(case, scene, ok, od))
        h = H.collide(b["transforms"], scene)
        assert h["count"] == len(ok), (case, warm)
        assert np.array_equal(h["keys"], ok) and np.array_equal(h["features"], of), (case, warm)
        assert np.array_equal(h["bodies"], ob), (case, warm)
        assert P.bits_equal(h["data"], od), (case, warm)
        seen += len(ok)
    assert seen > 0


@needs_ref
def test_rest_world_comes_to_rest_in_reference():
    """What tests/test_gpu_sphere_cases.py relies on for its still steps: in the reference every body of "rest" idles from the first step on, and the sphere and the
    box balanced on the apex of a static sphere keep x and z to the bit."""
    scene = U.sphere_world("rest")
    w = refworld.RefWorld(scene)
    start = w.bodies()["transforms"]["position"].copy()
    apex = [int(scene["sphere_transforms"]["body"][b - len(scene["box_tags"])]) for _, b in scene["groups"]["apex_sphere"]]
    apex += [int(scene["box_transforms"]["body"][a]) for a, _ in scene["groups"]["apex_box"]]
    assert len(apex) == 4 and all(apex)
    last = 0
    for _ in range(6):
        w.step(50)
        b = w.bodies()
        idle = b["idle"][1:]
        assert idle.min() > last or idle.min() == 255, (last, idle)
        last = int(idle.min())
        assert P.bits_equal(b["transforms"]["position"][apex][:, [0, 2]], start[apex][:, [0, 2]])
    assert last == 255
