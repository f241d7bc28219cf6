"""One context whose world grows during its life (pytest -m gpu): the library-owned buffers of nh_collide are sized by what a step is given -- body count,
collider count, pair capacity -- and every one of them has a branch that frees and allocates it again, with flags that void what the old buffers held.

World A starts as a prefix of its scene with a small pair capacity, steps, and is then given the whole scene and a larger pair capacity: every buffer grows
in a context that has stepped.  World B is a fresh context at the final sizes that takes over A's state at the moment of growth (snapshot / restore).  From
there on the two must agree bit for bit, like two worlds that were never different."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from query_util import FUSED, same_stepped_world as _same_stepped_world      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (scene, the prefix A starts with: (bodies, boxes, spheres), pair capacity before and after, steps each side of the growth)
#  pile: body 0 and the ground, 300 boxes, then 300 spheres -- the prefix leaves out the last 150 spheres and their bodies.  Falling bodies: full steps only.
#  grid_tiles: two slabs (boxes 0 and 1, body 0), then tile 0's 400 boxes, then tile 1's -- the prefix is tile 0 over both slabs.  A tile lands and rests
#  within a hundred steps, so A takes still steps before it grows, and both worlds take them again once tile 1 has landed too.
GROWN = {"pile": (lambda: S.pile(300, 300), (451, 301, 150), (2048, 6144), 40),
         "grid_tiles": (lambda: S.grid_tiles(2, side=20, seed=2), (401, 402, 0), (2048, 6144), 120)}


@pytest.mark.parametrize("name", sorted(GROWN))
def test_a_world_that_grows_steps_like_a_fresh_world_of_the_final_size(name):
    make, prefix, (pairs0, pairs1), steps = GROWN[name]
    scene = make()
    nb, nbox, nsph = len(scene["body_transforms"]), len(scene["box_tags"]), len(scene["sphere_tags"])
    assert prefix[0] < nb and prefix[1] + prefix[2] < nbox + nsph and pairs0 < pairs1
    b = E.World(scene, flags=FUSED, max_pairs=pairs1)
    a = E.World(scene, flags=FUSED, max_pairs=pairs0, capacity=dict(bodies=nb, boxes=nbox, spheres=nsph), arena_bytes=b.arena.size)
    a.set_counts(*prefix)
    a.step(steps)
    c0 = a.counts()
    assert c0["error"] == 0 and c0["contacts"] > 0 and c0["colliders"] == prefix[1] + prefix[2], c0
    # the growth: bodies, colliders and pair capacity all beyond anything A's context has seen (the new bodies are where the scene put them)
    snap = a.snapshot()
    a.set_counts(nb, nbox, nsph)
    E._check(a.L, a.L.nh_set_pair_capacity(a.ctx, pairs1), "nh_set_pair_capacity")
    b.restore(snap)
    a.step(steps); b.step(steps)
    _same_stepped_world(a, b, f"{name} grown", history=False)
    c1, cb = a.counts(), b.counts()
    print(f"\n[{name}] contacts {c0['contacts']} -> {c1['contacts']} (fresh world {cb['contacts']}), still steps {c0['still_steps']} -> {c1['still_steps']} (fresh world {cb['still_steps']}), "
          f"pairs {c0['pairs']} -> {c1['pairs']}")
    assert c1["error"] == 0 and c1["contacts"] == cb["contacts"] and c1["contacts"] > 0 and c1["colliders"] == nbox + nsph, (c1, cb)
    if name == "grid_tiles":                        # (the own_*, still_awake and body_col buffers belong to still steps; a pile never takes any: tests/test_gpu_still.py)
        assert c0["still_steps"] > 0 and c1["still_steps"] > c0["still_steps"] and cb["still_steps"] > 0, (c0, c1, cb)
    a.close(); b.close()
