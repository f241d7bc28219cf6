"""Which branch of the solve host path a scene takes (nudge_amd/csrc/nh_solve.hip: finish_setup, first_apply, nh_apply_impulses) -- pytest -m gpu.

The other GPU suites compare bits along most of these paths, but none says which branch a scene took: a stage that is silently skipped, or run twice, can pass
them.  Every row here builds one small world, brings it to the state that reaches the branch, then steps it through a short window with every launch timed and
reads the launch counts by timer name: the names that identify the branch were launched, those of the alternative were not.  The same world is stepped again
with timing off -- full timing switches the early counters off, so the two runs take different host paths -- and against a partner that reaches the same
arithmetic by another host path (option no_resident, option no_early_counts, no still steps, the eight calls made by hand, the compiled reference in exact
order); transforms, momentum, idle counters, cache count, cache tags and cached impulses must agree bit for bit.

`run_row(name)` returns the launch counts and the states without asserting anything: dev scripts use it to compare two builds of the library row by row."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from nudge_amd import scenes as S                  # noqa: E402
from nudge_amd import engine as E                  # noqa: E402
import parity_util as P                            # noqa: E402
import make_golden as G                            # noqa: E402
from oracle import refworld                        # noqa: E402

pytestmark = pytest.mark.gpu

BENCH = E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP
EXACT = E.NH_FLAG_SYNC_COUNTS | E.NH_FLAG_EXACT_ORDER


def _world(scene, env=None, flags=BENCH, **kw):
    env = {k: str(v) for k, v in (env or {}).items()}
    os.environ.update(env)
    try:
        return E.World(scene, flags=flags, **kw)
    finally:
        for k in env:
            os.environ.pop(k, None)


def _eight_calls(w, steps, between=None):
    for _ in range(steps):
        w.collide(); w.gravity(); w.read_cache(); w.setup()
        if between:
            between(w)
        w.apply(); w.update(); w.write_cache(); w.advance(); w.step_done()


def _timed(w, advance):
    """Launch counts by timer name over `advance(w)`."""
    w.synchronize()
    w.enable_timing(True)
    w.kernel_times()
    advance(w)
    w.synchronize()
    kt = w.kernel_times()
    w.enable_timing(False)
    return {k: int(n) for k, (_, n) in kt.items() if n}


def _state(w):
    b, c = w.get_bodies(), w.get_cache()
    return dict(transforms=b["transforms"], velocity=b["momentum"]["velocity"], angular_velocity=b["momentum"]["angular_velocity"], momentum=b["momentum"],
                idle=b["idle"], cache_count=np.array([c["count"]], dtype=np.uint32), cache_tags=c["tags"], cache_features=c["features"], cache_impulses=c["data"]["impulse"])


def _ref_state(r):
    b, c = r.bodies(), r.cache()
    return dict(transforms=b["transforms"], velocity=b["momentum"]["velocity"], angular_velocity=b["momentum"]["angular_velocity"], idle=b["idle"],
                cache_count=np.array([c["count"]], dtype=np.uint32), cache_impulses=c["data"]["impulse"])          # (the reference's tags are the narrow ones)


def _windowed(scene, env, partner_env, warm, window, flags=BENCH, partner_flags=None, by_hand=False, advance=None, **kw):
    """The usual row: a timed world, the same world untimed and one partner, all brought `warm` steps in; then the window."""
    advance = advance or (lambda w: w.step(window))
    t, u = _world(scene, env, flags, **kw), _world(scene, env, flags, **kw)
    p = _world(scene, partner_env, flags if partner_flags is None else partner_flags, **kw)
    for w in (t, u, p):
        if warm:
            w.step(warm)
    before = t.counts()
    launches = _timed(t, advance)
    advance(u)
    if by_hand:
        _eight_calls(p, t.steps_done - p.steps_done)
    else:
        advance(p)
    out = dict(launches=launches, before=before, after=t.counts(), states=dict(timed=_state(t), untimed=_state(u), partner=_state(p)))
    for w in (t, u, p):
        assert w.counts()["error"] == 0
        w.close()
    return out


PIT12 = dict(nx=12, ny=12, nz=12, seed=4)
PIT_CAPS = dict(max_contacts=8 * 12 ** 3, max_pairs=10 * 12 ** 3)


def _row_resident():
    # a pile of 256 boxes: a few hundred general contacts, full rows -- colouring and level order by one workgroup, rows resident in LDS
    return _windowed(S.pile(n_boxes=256, seed=1), None, dict(NH_NO_RESIDENT=1), 100, 20)


def _row_resident_by_hand():
    # ... and the same branch with the eight calls made by the caller instead of nh_step
    return _windowed(S.pile(n_boxes=256, seed=1), None, None, 100, 20, by_hand=True)


def _row_resident_bodies():
    # the 12^3 pit: more rows than one compute unit's LDS holds, but a small world -- every body's momentum resident
    return _windowed(S.ball_pit(**PIT12), None, dict(NH_NO_RESIDENT=1), 130, 20)


def _row_levels():
    # the same pit without the one-workgroup solvers: colouring rounds, level order, one launch per level and sweep
    return _windowed(S.ball_pit(**PIT12), dict(NH_NO_RESIDENT=1), None, 130, 20)


def _row_levels_exact():
    # exact order: relaxation instead of colouring, against the compiled reference
    scene = S.ball_pit(nx=6, ny=6, nz=6, seed=4)
    t, u = _world(scene, dict(NH_NO_RESIDENT=1), EXACT), _world(scene, dict(NH_NO_RESIDENT=1), EXACT)
    launches = _timed(t, lambda w: w.step(100))
    u.step(100)
    r = refworld.RefWorld(scene)
    r.step(100)
    out = dict(launches=launches, after=t.counts(), states=dict(timed=_state(t), untimed=_state(u), partner=_ref_state(r)))
    t.close(); u.close()
    return out


def _row_compact():
    # while the pit falls in, a colouring round leaves at most half of the list: the later rounds walk a compacted one
    return _windowed(S.ball_pit(**PIT12), dict(NH_NO_RESIDENT=1), None, 0, 60)


BLK = dict(NH_BLK_MIN=1, NH_BLK_TARGET=120)


def _row_blocked_local():
    # several blocks that colour their own contacts: no world-wide colouring, one adjacency fill
    return _windowed(S.ball_pit(**PIT12), BLK, BLK, 130, 20, by_hand=True, **PIT_CAPS)


def _row_blocked_global():
    # the world-wide colouring, then ONE block that walks the colours like the per-level launches do
    env = dict(NH_BLK_MIN=1, NH_BLK_TARGET=1000000, NH_BLK_GLOBAL_COLOURS=1, NH_NO_RESIDENT=1)
    return _windowed(S.ball_pit(**PIT12), env, dict(NH_NO_BLOCKS=1, NH_NO_RESIDENT=1), 130, 20, **PIT_CAPS)


def _row_blocked_declined():
    # a heap of boxes and spheres of very different sizes falling into tiny blocks: on some steps a contact is nobody's, the per-block colouring gives up and the
    # lists of the general bodies that the adjacency build had left out are filled behind it
    scene = S.pile(1000, 500, seed=33, iterations=8)
    env = dict(NH_BLK_MIN=1, NH_BLK_TARGET=8)
    return _windowed(scene, env, env, 0, 40, by_hand=True, max_contacts=16 * 1500, max_pairs=20 * 1500)


def _row_static8():
    # compound bodies while they land: some rest on the static world with five to eight contacts
    scene, _ = G.build("compound")
    return _windowed(scene, None, dict(NH_NO_EARLY_COUNTS=1), 40, 60)


def _row_gravity_rest_pile():
    # bodies outside the fused class: their gravity is a launch of its own, once the round trip has told that there are any
    return _windowed(S.pile(n_boxes=256, seed=1), None, dict(NH_NO_EARLY_COUNTS=1), 100, 20)


def _row_gravity_rest_landed():
    # a landed grid: every body is the fused solver's (full steps: a still step never reaches finish_setup; the partner takes still steps)
    scene, _ = G.build("grid30_awake")
    return _windowed(scene, dict(NH_NO_STILL=1), None, 120, 20)


def _row_flush():
    # counts() between setup and apply: the flush runs first_apply with zero sweeps and the blocked warm start; the apply that follows only sweeps
    scene = S.ball_pit(**PIT12)
    t, u, p = _world(scene, BLK, **PIT_CAPS), _world(scene, BLK, **PIT_CAPS), _world(scene, BLK, **PIT_CAPS)
    for w in (t, u, p):
        w.step(130)

    def look(w):
        assert w.counts()["error"] == 0
    launches = _timed(t, lambda w: _eight_calls(w, 20, look))
    _eight_calls(u, 20, look)
    partner_launches = _timed(p, lambda w: _eight_calls(w, 20))          # (the world that applied directly)
    out = dict(launches=launches, partner_launches=partner_launches, after=t.counts(), states=dict(timed=_state(t), untimed=_state(u), partner=_state(p)))
    for w in (t, u, p):
        w.close()
    return out


TILES = dict(n_tiles=2, side=12, seed=2, lattice_cols=2)


def _row_still_ring():
    # two landed tiles under step(n): the verdict of a still step is read one step late, from the ring; the event path is the partner
    return _windowed(S.grid_tiles(**TILES), None, dict(NH_NO_EARLY_COUNTS=1), 120, 24)


def _row_still_ring_full():
    # ... and against the world that never speculates
    return _windowed(S.grid_tiles(**TILES), None, dict(NH_NO_STILL=1), 120, 24)


def _row_still_round_trip():
    # one call per step: every still step is confirmed by its own round trip
    def one_by_one(w):
        for _ in range(24):
            w.step(1)
    return _windowed(S.grid_tiles(**TILES), None, dict(NH_NO_STILL=1), 120, 24, advance=one_by_one)


GENERAL_OFF = ("colour_small", "colour_seed", "level_relax", "rows_general", "solve_resident", "solve_resident_bodies", "warm_level", "apply_level", "blk_prepare")
# row -> (function, needs the compiled reference, names that must have been launched, names that must not)
ROWS = {
    "resident": (_row_resident, False, ("solve_one_body", "adjacency_fill", "colour_small", "rows_general", "solve_resident"),
                 ("solve_still", "solve_resident_bodies", "colour_seed", "colour_try", "level_relax", "level_hist", "warm_level", "apply_level", "blk_prepare")),
    "resident_by_hand": (_row_resident_by_hand, False, ("solve_one_body", "colour_small", "rows_general", "solve_resident"),
                         ("solve_resident_bodies", "colour_seed", "level_hist", "warm_level", "apply_level", "blk_prepare")),
    "resident_bodies": (_row_resident_bodies, False, ("colour_small", "rows_general", "solve_resident_bodies"),
                        ("solve_resident", "colour_seed", "colour_try", "level_relax", "level_hist", "warm_level", "apply_level", "blk_prepare")),
    "levels": (_row_levels, False, ("level_reset", "colour_seed", "colour_validate", "colour_try", "colour_settle", "level_hist", "level_offsets", "level_scatter", "rows_general",
                                    "warm_level", "apply_level"), ("colour_small", "level_relax", "solve_resident", "solve_resident_bodies", "blk_prepare")),
    "levels_exact": (_row_levels_exact, True, ("level_reset", "level_relax", "level_hist", "level_offsets", "level_scatter", "rows_general", "warm_level", "apply_level"),
                     ("colour_small", "colour_seed", "colour_validate", "colour_try", "colour_settle", "colour_compact", "solve_resident", "solve_resident_bodies", "blk_prepare")),
    "compact": (_row_compact, False, ("colour_try", "colour_settle", "colour_compact", "warm_level", "apply_level"), ("colour_small", "level_relax", "blk_prepare")),
    "blocked_local": (_row_blocked_local, False, ("adjacency_fill", "blk_contact", "blk_scatter", "blk_prepare", "blk_slots", "rows_general", "blk_gather", "blk_warm", "blk_sweep", "blk_scatter_back"),
                      ("colour_small", "colour_seed", "colour_try", "level_hist", "solve_resident", "solve_resident_bodies", "warm_level", "apply_level")),
    "blocked_global": (_row_blocked_global, False, ("level_reset", "colour_seed", "colour_validate", "blk_prepare", "rows_general", "blk_gather", "blk_warm", "blk_sweep", "blk_scatter_back"),
                       ("colour_small", "blk_slots", "level_hist", "level_scatter", "solve_resident", "solve_resident_bodies")),
    "blocked_declined": (_row_blocked_declined, False, ("adjacency_fill", "adjacency_sort", "blk_prepare", "blk_slots", "blk_warm", "blk_sweep"), ()),
    "static8": (_row_static8, False, ("solve_one_body", "solve_one_body8", "gravity_rest"), ("apply_static", "apply_static8", "setup_staticN", "apply_staticN")),
    "gravity_rest_pile": (_row_gravity_rest_pile, False, ("solve_one_body", "gravity_rest"), ("solve_still", "gravity_damping")),
    "gravity_rest_landed": (_row_gravity_rest_landed, False, ("solve_one_body",), ("solve_still", "gravity_rest", "gravity_damping", "adjacency_fill") + GENERAL_OFF),
    "flush": (_row_flush, False, ("solve_one_body", "blk_prepare", "blk_warm", "blk_sweep"), ("colour_small", "solve_resident", "solve_resident_bodies")),
    "still_ring": (_row_still_ring, False, ("solve_still",), ("solve_one_body", "solve_one_body8", "gravity_rest", "gravity_damping", "adjacency_fill") + GENERAL_OFF),
    "still_ring_full": (_row_still_ring_full, False, ("solve_still",), ("solve_one_body", "gravity_rest", "adjacency_fill") + GENERAL_OFF),
    "still_round_trip": (_row_still_round_trip, False, ("solve_still",), ("solve_one_body", "gravity_rest", "adjacency_fill") + GENERAL_OFF),
}


def run_row(name):
    return ROWS[name][0]()


@pytest.mark.parametrize("name", sorted(ROWS))
def test_the_branch_a_scene_takes_and_the_bits_it_leaves(name):
    fn, needs_ref, must, must_not = ROWS[name]
    if needs_ref and not refworld.available("exact"):
        pytest.skip("oracle/_ref did not travel to this box")
    out = fn()
    n = out["launches"]
    print(f"\n[{name}] " + " ".join(f"{k}={v}" for k, v in sorted(n.items())))
    for k in must:
        assert n.get(k, 0) > 0, f"{name}: {k} was not launched"
    for k in must_not:
        assert n.get(k, 0) == 0, f"{name}: {k} was launched {n.get(k)} times"
    if name == "blocked_declined":
        # one adjacency build per step with general contacts, and on the steps whose per-block colouring gave up a second fill: the lists it had left out
        assert n["adjacency_sort"] < n["adjacency_fill"] <= 2 * n["adjacency_sort"], n
    if name == "blocked_local":
        assert n["adjacency_fill"] == n["adjacency_sort"], n
    if name == "flush":
        # the warm start runs once per step, in the flush or in the apply, and the sweeps once
        m = out["partner_launches"]
        for k in ("blk_prepare", "blk_warm", "blk_sweep", "rows_general"):
            assert n[k] == m[k], (k, n[k], m[k])
        for k in ("blk_gather", "blk_scatter_back"):          # (the flush's warm start is a blk_run of its own: the momentum goes into block order and back twice)
            assert n[k] == 2 * m[k], (k, n[k], m[k])
        assert n["solve_one_body"] == m["solve_one_body"] + 20          # (... and the apply that follows launches the late one-body classes itself)
    if name.startswith("still"):
        # every solver of the window was a still step's, and every one of them was confirmed
        assert out["after"]["still_replays"] == out["before"]["still_replays"]
        assert out["after"]["still_steps"] - out["before"]["still_steps"] == n["solve_still"] > 0, (out["before"]["still_steps"], out["after"]["still_steps"], n["solve_still"])
    ref = out["states"]["partner"]
    for who in ("timed", "untimed"):
        s = out["states"][who]
        for k, v in ref.items():
            if k == "idle" or k.startswith("cache_count") or k in ("cache_tags", "cache_features"):
                assert np.array_equal(s[k], v), f"{name}: {k} of the {who} world differs from the partner's"
            else:
                assert P.bits_equal(s[k], v), f"{name}: {k} of the {who} world differs from the partner's"
