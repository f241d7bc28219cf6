"""GPU parity tests at BASELINE.json's full sizes (pytest -m gpu): configs[1] (1,004,400 boxes), configs[2] (2,008,800
mixed boxes + spheres) and configs[3] (4,096,000-sphere ball pit), SURVEY 8(d).

The reference cannot hold these worlds (<= 8192 colliders, nudge.cpp:3010), so
  * drop scenes (c2, c3) are unions of independent tiles: the GPU steps the union as ONE world in the bench's mode, the
    compiled reference steps EVERY tile on its own (all host threads), and the bar is the north star's -- body state within
    1e-4 relative after 1000 steps.  The bound is shown in two parts: (1) a tile stepped alone on the GPU is BIT-identical to
    the reference stepping that tile; (2) union versus tile -- the only thing that differs is the batch slot of a contact, which
    depends on how many contacts precede it in the world (nudge.cpp:4206-4339) -- stays within the bound, and the reference
    shows the same effect against itself (tests/test_cpu_oracle.py::test_reference_union_vs_tile_self_deviation);
  * the ball pit (c4) is one connected, chaotic island: invariants of the full scene inside bands taken from the reference's
    own runs of instances it can hold (a 20^3 pit for the contact statistics, a 7x7x160 column -- the same pile height, hence
    the same pressure -- for penetration and the energy decay).
These tests need the compiled reference on the box (oracle/_ref travels with the repository): without it they FAIL."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from nudge_amd import scenes as S                  # noqa: E402
from nudge_amd import engine as E                  # noqa: E402
import hostlib                                     # noqa: E402
import parity_util as P                            # noqa: E402
from oracle import refworld                        # noqa: E402

pytestmark = pytest.mark.gpu

POS_TOL = 1e-4          # the north star's bar: ||p - p_ref|| / max(||p_ref||, 1) for EVERY body; and, sharper, relative to the
                        # body's TILE ORIGIN, ||p - p_ref|| / max(||p_ref - tile origin||, 1), for 99.99 % of the bodies
POS_TOL_TILE_MAX = 2e-4 # ... with the worst body within twice that.  Union vs tile is not bit-exact in the reference either: over 446,400 bodies it
                        # moves 9.1e-5 (max) / 4.8e-5 (99.99 %) away from ITSELF, |dv| up to 2.0e-4 (profiles/r02_reference_self_deviation.json,
                        # tests/golden/reference_self_deviation.py); the tail grows with the number of bodies looked at
VEL_TOL_UNION = 3e-4    # union vs tile, absolute, bodies at rest (|v| < 1)


BENCH_FLAGS = E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP      # bench.py's World(...) flags at N = 1


def _require_reference():
    assert refworld.available("exact"), "oracle/_ref/libnudge_ref_exact.so did not travel to this box: the at-size parity tests need it"


def _tiled_reference(scene, n_tiles, steps):
    """Every tile of the union stepped on its own by the compiled reference, one tile per host thread."""
    worlds, maps = [], []
    for t in range(n_tiles):
        sub, body_map = S.extract_tile(scene, t)
        worlds.append(refworld.RefWorld(sub, max_contacts=6 * len(sub["body_transforms"])))
        maps.append(body_map)
    refworld.step_tiles(worlds, steps, threads=hostlib.threads(), ftz=False)
    return worlds, maps


def _union_vs_tiled_reference(scene, n_tiles, steps, sample_tiles):
    n = len(scene["body_transforms"]) - 1
    w = E.World(scene, flags=BENCH_FLAGS, max_contacts=6 * n)            # exactly the flags bench.py runs: one host round trip per step, one apply call, gravity / advance fused
    w.step(steps)
    c = w.counts()
    assert c["error"] == 0
    gb = w.get_bodies()
    w.close()
    assert np.isfinite(gb["transforms"]["position"]).all() and np.isfinite(gb["momentum"]["velocity"]).all()
    worlds, maps = _tiled_reference(scene, n_tiles, steps)
    worst_p, worst_v, worst_w, asleep, errs = 0.0, 0.0, 0.0, 0, []
    for t in range(n_tiles):
        rb, body_map = worlds[t].bodies(), maps[t]
        origin = scene["box_transforms"]["position"][t].astype(np.float64)
        err = P.rel_err(gb["transforms"]["position"][body_map[1:]], rb["transforms"]["position"][1:], origin=origin)
        errs.append(err)
        worst_p = max(worst_p, float(P.rel_err(gb["transforms"]["position"][body_map[1:]], rb["transforms"]["position"][1:]).max()))
        worst_v = max(worst_v, float(np.abs(gb["momentum"]["velocity"][body_map[1:]] - rb["momentum"]["velocity"][1:]).max()))
        worst_w = max(worst_w, float(np.abs(gb["momentum"]["angular_velocity"][body_map[1:]] - rb["momentum"]["angular_velocity"][1:]).max()))
        assert np.array_equal(gb["idle"][body_map[1:]] == 0xff, rb["idle"][1:] == 0xff), f"tile {t}: different bodies asleep"
        asleep += int((rb["idle"][1:] == 0xff).sum())
        assert np.abs(rb["momentum"]["velocity"][1:]).max() < 1.0        # at rest: the velocity bound is absolute
    errs = np.concatenate(errs)
    q9999, tile_max = float(np.quantile(errs, 0.9999)), float(errs.max())
    print(f"\n[{scene['name']}] union vs tiled reference, ALL {n_tiles} tiles, {steps} steps: position error relative to |p| max {worst_p:.3e} (bar {POS_TOL:.0e}); "
          f"relative to the tile origin 99.99 % {q9999:.3e} (bar {POS_TOL:.0e}), max {tile_max:.3e} (bar {POS_TOL_TILE_MAX:.0e}), {int((errs > POS_TOL).sum())} bodies above 1e-4; "
          f"max |dv| {worst_v:.3e}, max |dw| {worst_w:.3e} (bar {VEL_TOL_UNION:.0e}); {asleep} of {n} bodies asleep")
    assert asleep > 0.9 * n, "the scene was meant to have gone to sleep: islands, sleeping pairs and cache culling all ran"
    assert c["sleeping_pairs"] > 0.9 * n, c
    assert worst_p <= POS_TOL, worst_p
    assert q9999 <= POS_TOL and tile_max <= POS_TOL_TILE_MAX, (q9999, tile_max)
    assert worst_v <= VEL_TOL_UNION and worst_w <= 10 * VEL_TOL_UNION, (worst_v, worst_w)
    # the two-part bound on sampled tiles: GPU(tile) == reference(tile) bit for bit, GPU(union) vs GPU(tile) within the bar
    for t in sample_tiles:
        sub, body_map = S.extract_tile(scene, t)
        wt = E.World(sub, flags=BENCH_FLAGS)
        wt.step(steps)
        tb, rb = wt.get_bodies(), worlds[t].bodies()
        wt.close()
        assert P.bits_equal(tb["transforms"], rb["transforms"]), f"tile {t} alone on the GPU differs from the reference"
        assert P.bits_equal(tb["momentum"]["velocity"], rb["momentum"]["velocity"]) and P.bits_equal(tb["momentum"]["angular_velocity"], rb["momentum"]["angular_velocity"])
        assert np.array_equal(tb["idle"], rb["idle"])
    return worst_p, worst_v


def test_c2_million_boxes_1000_steps_every_tile_vs_reference():
    """BASELINE.json configs[1] / north star: 1,004,400 boxes, 8 iterations, 1000 steps, all 124 tiles against the reference."""
    _require_reference()
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    assert len(scene["body_transforms"]) - 1 == 1004400
    _union_vs_tiled_reference(scene, 124, 1000, sample_tiles=(0, 61, 123))


def test_c3_two_million_mixed_1000_steps_every_tile_vs_reference():
    """BASELINE.json configs[2]: 2,008,800 bodies, boxes and spheres 50/50 (all three narrowphase kernels), 8 iterations, 1000 steps,
    all 248 tiles against the reference."""
    _require_reference()
    scene = S.grid_tiles(248, side=90, sphere_fraction=0.5, seed=3, lattice_cols=16)
    assert len(scene["body_transforms"]) - 1 == 2008800
    _union_vs_tiled_reference(scene, 248, 1000, sample_tiles=(0, 100, 247))


@pytest.mark.parametrize("spheres", [0.0, 0.5])
def test_union_the_reference_can_hold_is_bit_exact_in_the_bench_mode(spheres):
    """Two tiles of 63 x 63 bodies (7938 + two ground slabs: the largest union under the reference's 8192-collider limit, nudge.cpp:3010) stepped as
    ONE world by both sides for 1000 steps -- fall, landing, rest, sleep.  In a union a contact's batch slot depends on how many contacts precede
    it in the world (nudge.cpp:4206-4339); that is why union-vs-TILE comparisons carry a 1e-4 bar.  Union against the SAME union has no such
    excuse: the GPU in the bench's exact flags (default order, one apply call, fused gravity / advance, kept pair list, re-used tag sort) must give
    the reference's bits, cache and sleeping pairs included."""
    _require_reference()
    scene = S.grid_tiles(2, side=63, sphere_fraction=spheres, seed=11, lattice_cols=2)
    n = len(scene["body_transforms"]) - 1
    assert n == 7938
    ref = refworld.RefWorld(scene, max_contacts=6 * n)
    w = E.World(scene, flags=BENCH_FLAGS, max_contacts=6 * n)
    for upto in (100, 400, 1000):
        ref.step(upto - w.steps_done); w.step(upto - w.steps_done)
        gb, rb = w.get_bodies(), ref.bodies()
        assert P.bits_equal(gb["transforms"]["position"], rb["transforms"]["position"]) and P.bits_equal(gb["transforms"]["rotation"], rb["transforms"]["rotation"]), upto
        assert P.bits_equal(gb["momentum"]["velocity"], rb["momentum"]["velocity"]) and P.bits_equal(gb["momentum"]["angular_velocity"], rb["momentum"]["angular_velocity"]), upto
        assert np.array_equal(gb["idle"], rb["idle"]), upto
    c = w.counts()
    assert c["error"] == 0 and c["general_contacts"] == 0
    assert int((rb["idle"][1:] == 0xff).sum()) > 0.9 * n, "the union was meant to have gone to sleep"
    kc, rc = w.get_cache(), ref.cache()
    assert kc["count"] == rc["count"] and P.bits_equal(kc["data"]["impulse"], rc["data"]["impulse"])
    w.close()


def test_c2_exact_order_equals_bench_flags_at_size():
    """Pins the CLOSED-FORM solver order at the size the metric is quoted on.  The bench runs the default order -- batch(i) = (i >> 7) * 16 + (i & 15),
    what the reference's greedy scheduler (nudge.cpp:4206-4339) produces when it meets no lane conflict.  NH_FLAG_EXACT_ORDER checks every step for a conflict and
    replays the scheduler if there is one.  1,004,400 boxes, 300 steps -- free fall, landing, rest -- in the bench's flags and under NH_FLAG_EXACT_ORDER: the same bits
    (bodies, idle counters, contacts, cache), nothing on the general path.  What remains un-pinned at size is then ONLY the reference's own union-versus-tile effect
    (the bars above)."""
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    n = len(scene["body_transforms"]) - 1
    assert n == 1004400
    a = E.World(scene, flags=BENCH_FLAGS, max_contacts=6 * n)
    b = E.World(scene, flags=E.NH_FLAG_EXACT_ORDER, max_contacts=6 * n)
    done = 0
    for cp in (40, 70, 150, 300):
        a.step(cp - done); b.step(cp - done); done = cp
        ba, bb = a.get_bodies(), b.get_bodies()
        assert P.bits_equal(ba["transforms"], bb["transforms"]) and P.bits_equal(ba["momentum"], bb["momentum"]) and np.array_equal(ba["idle"], bb["idle"]), f"step {cp}: bodies differ"
        ca, cb = a.counts(), b.counts()
        assert ca["error"] == 0 and cb["error"] == 0
        assert ca["general_contacts"] == 0 and cb["general_contacts"] == 0, (ca["general_contacts"], cb["general_contacts"])
        assert ca["contacts"] == cb["contacts"]
    ka, kb = a.get_contacts(), b.get_contacts()
    assert np.array_equal(ka["tags"], kb["tags"]) and np.array_equal(ka["features"], kb["features"]) and P.bits_equal(ka["data"], kb["data"])
    xa, xb = a.get_cache(), b.get_cache()
    assert xa["count"] == xb["count"] and np.array_equal(xa["tags"], xb["tags"]) and np.array_equal(xa["features"], xb["features"])
    # (the cached impulse's fourth word: zero under NH_FLAG_EXACT_ORDER, the colour of the last sweep in default order -- include/nudge_hip.h; the impulses are the bits)
    assert P.bits_equal(xa["data"]["impulse"], xb["data"]["impulse"])
    assert a.counts()["still_steps"] > 150          # (the bench's flags went through the still regime on the way)
    a.close(); b.close()


def test_c2_half_asleep_and_movers_at_size_are_the_bits_of_full_steps(monkeypatch):
    """Local speculation at the size the metric is quoted on: 1,004,400 boxes fall asleep; the caller wakes the left half (idle counters rewritten) and throws 64 of the
    woken boxes into the air.  For 120 steps the world is half asleep with bodies in flight -- still steps in sleepers AND movers form -- against a library that runs every
    step in full (no still steps, no asleep steps): bodies, idle counters, contacts, sleeping pairs, active list, cache and counters bit for bit."""
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    n = len(scene["body_transforms"]) - 1
    a = E.World(scene, flags=BENCH_FLAGS, max_contacts=6 * n)
    monkeypatch.setenv("NH_NO_STILL", "1"); monkeypatch.setenv("NH_NO_ASLEEP", "1")
    b = E.World(scene, flags=BENCH_FLAGS, max_contacts=6 * n)
    monkeypatch.delenv("NH_NO_STILL"); monkeypatch.delenv("NH_NO_ASLEEP")
    a.step(400); b.step(400)
    assert a.counts()["active_bodies"] == 0 and b.counts()["active_bodies"] == 0
    order = np.argsort(scene["body_transforms"]["position"][1:, 0], kind="stable") + 1
    woken = order[: n // 2]
    rng = np.random.default_rng(9)
    fliers = rng.choice(woken, size=64, replace=False)
    for w in (a, b):
        bd = w.get_bodies()
        idle, m = bd["idle"].copy(), bd["momentum"].copy()
        idle[woken] = 0
        m["velocity"][fliers, 1] = 25.0
        w.set_bodies(momentum=m, idle=idle)
    c0 = a.counts()
    done = 0
    for cp in (1, 2, 30, 120):
        a.step(cp - done); b.step(cp - done); done = cp
        ba, bb = a.get_bodies(), b.get_bodies()
        assert P.bits_equal(ba["transforms"], bb["transforms"]) and P.bits_equal(ba["momentum"], bb["momentum"]) and np.array_equal(ba["idle"], bb["idle"]), f"step {cp}: bodies differ"
        ca, cb = a.counts(), b.counts()
        for k in ("contacts", "sleeping_pairs", "active_bodies", "cache", "error"):
            assert ca[k] == cb[k], (cp, k, ca[k], cb[k])
    ka, kb = a.get_contacts(), b.get_contacts()
    assert np.array_equal(ka["tags"], kb["tags"]) and np.array_equal(ka["features"], kb["features"]) and P.bits_equal(ka["data"], kb["data"])
    assert np.array_equal(ka["sleeping_pairs"], kb["sleeping_pairs"]) and len(ka["sleeping_pairs"]) >= n // 2 - 1
    assert np.array_equal(a.get_active(), b.get_active())
    xa, xb = a.get_cache(), b.get_cache()
    assert xa["count"] == xb["count"] and np.array_equal(xa["tags"], xb["tags"]) and np.array_equal(xa["features"], xb["features"]) and P.bits_equal(xa["data"]["impulse"], xb["data"]["impulse"])
    c1 = a.counts()
    print(f"\n[c2 half asleep + 64 fliers] {c1['still_steps'] - c0['still_steps']} still steps of {done} ({c1['still_replays'] - c0['still_replays']} replayed), {c1['broadphase_inserts'] - c0['broadphase_inserts']} re-insertions")
    assert c1["still_steps"] - c0["still_steps"] >= 100 and c1["broadphase_inserts"] > c0["broadphase_inserts"]
    a.close(); b.close()


def test_c2_landed_window_properties():
    """The window the bench times: every box rests on 4 face contacts, everybody awake, nothing on the general path, two runs agree
    bit for bit."""
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    n = len(scene["body_transforms"]) - 1
    finals = []
    for rep in range(2):
        w = E.World(scene, flags=E.NH_FLAG_SYNC_COUNTS, max_contacts=6 * n)
        w.step(70)
        c = w.counts()
        finals.append(w.get_bodies())
        if rep == 0:
            assert c["error"] == 0
            assert 3.9 * n <= c["contacts"] <= 4 * n, c
            assert c["active_bodies"] == n and c["general_contacts"] == 0
        w.close()
    a, b = finals
    assert np.isfinite(a["transforms"]["position"]).all() and np.isfinite(a["momentum"]["velocity"]).all()
    assert P.bits_equal(a["transforms"], b["transforms"]) and P.bits_equal(a["momentum"], b["momentum"])


@pytest.mark.parametrize("config", ["c2", "c3"])
def test_temporal_coherence_paths_are_bit_identical_at_size(config, monkeypatch):
    """The broadphase's kept pair list, the re-used tag sort and the fused gravity / advance are what the bench runs.  At BASELINE's sizes they must give
    the very bits of a world that searches the grid, sorts the records and runs the separate kernels every step -- through the fall, the landing (rebuilds,
    key changes) and the rest (hundreds of steps on one kept list) -- and they must actually have been taken."""
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11) if config == "c2" else S.grid_tiles(248, side=90, sphere_fraction=0.5, seed=3, lattice_cols=16)
    nb = len(scene["body_transforms"])
    a = E.World(scene, flags=E.NH_FLAG_FUSED_STEP, max_contacts=6 * nb)
    monkeypatch.setenv("NH_NO_KEPT_PAIRS", "1"); monkeypatch.setenv("NH_NO_SORT_REUSE", "1")
    b = E.World(scene, flags=0, max_contacts=6 * nb)
    monkeypatch.delenv("NH_NO_KEPT_PAIRS"); monkeypatch.delenv("NH_NO_SORT_REUSE")
    for upto in (40, 80, 200):
        done = a.steps_done
        a.step(upto - done); b.step(upto - done)
        x, y = a.get_bodies(), b.get_bodies()
        assert P.bits_equal(x["transforms"], y["transforms"]) and P.bits_equal(x["momentum"], y["momentum"]) and np.array_equal(x["idle"], y["idle"]), (config, upto)
    ka, kb = a.get_cache(), b.get_cache()
    assert ka["count"] == kb["count"] and np.array_equal(ka["tags"], kb["tags"]) and P.bits_equal(ka["data"]["impulse"], kb["data"]["impulse"])
    ca, cb = a.counts(), b.counts()
    assert cb["sort_reuses"] == 0 and cb["broadphase_rebuilds"] >= 200
    # (a step either re-uses the tag order of the sort before it, or -- at rest -- is a still step that does not even ask: include/nudge_hip.h note 9)
    assert ca["broadphase_rebuilds"] < 40 and ca["sort_reuses"] + ca["still_steps"] > 80 and ca["still_steps"] > 60, ca
    a.close(); b.close()


def test_movers_in_a_million_boxes_at_rest_are_reinserted_bit_identically(monkeypatch):
    """The regime re-insertion into the kept pair list is for, at BASELINE's size: the 1,004,400 boxes of config 2 have landed; 300 of them are thrown across
    their neighbours (some fly for the whole window and leave their inflated boxes on every step, some hop and land on other boxes, a few are teleported).
    The default world re-inserts the leavers (no rebuild while they move); a world that searches the grid every step must give the very same bits."""
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
    a = E.World(scene, flags=E.NH_FLAG_FUSED_STEP, max_contacts=6 * nb)
    monkeypatch.setenv("NH_NO_KEPT_PAIRS", "1")
    b = E.World(scene, flags=E.NH_FLAG_FUSED_STEP, max_contacts=6 * nb)
    monkeypatch.delenv("NH_NO_KEPT_PAIRS")
    a.step(75); b.step(75)
    rng = np.random.default_rng(11)
    movers = rng.choice(np.arange(1, nb), size=300, replace=False)
    kick = rng.uniform(-3.0, 3.0, size=(300, 3)).astype(np.float32)
    kick[:100, 1] = 30.0; kick[100:, 1] = rng.uniform(1.0, 4.0, size=200).astype(np.float32)
    c0 = a.counts()
    for w in (a, b):
        bd = w.get_bodies()
        m = bd["momentum"].copy(); m["velocity"][movers] = kick
        t = bd["transforms"].copy(); t["position"][movers[-5:], 1] += np.float32(1.5); t["position"][movers[-5:], 0] += np.float32(0.7)
        w.set_bodies(transforms=t, momentum=m)
    for upto in (20, 60, 120):
        a.step(upto - (a.steps_done - 75)); b.step(upto - (b.steps_done - 75))
        x, y = a.get_bodies(), b.get_bodies()
        assert P.bits_equal(x["transforms"], y["transforms"]) and P.bits_equal(x["momentum"], y["momentum"]) and np.array_equal(x["idle"], y["idle"]), upto
    ka, kb = a.get_cache(), b.get_cache()
    assert ka["count"] == kb["count"] and np.array_equal(ka["tags"], kb["tags"]) and P.bits_equal(ka["data"]["impulse"], kb["data"]["impulse"])
    ca, cb = a.counts(), b.counts()
    assert ca["error"] == 0 and cb["error"] == 0
    print(f"\n[1 M boxes, 300 movers, 120 steps] re-insertions {ca['broadphase_inserts'] - c0['broadphase_inserts']}, rebuilds {ca['broadphase_rebuilds'] - c0['broadphase_rebuilds']} (search every step: {cb['broadphase_rebuilds']})")
    assert ca["broadphase_inserts"] - c0["broadphase_inserts"] > 5000 and ca["broadphase_rebuilds"] - c0["broadphase_rebuilds"] <= 6, ca
    a.close(); b.close()


# ---- config 4: the ball pit -------------------------------------------------------------------------------------------------------
def _pit_stats(scene, pos, vel, contact_bodies, penetration, wall_margin=2.0):
    """Invariants of a pit of r = 0.5 spheres: max penetration, kinetic energy per sphere, contact degree of INTERIOR spheres
    (at least `wall_margin` from floor / walls and 3 below the free surface), share of spheres inside the container."""
    nb = len(pos)
    st = scene["box_transforms"]["position"]
    sz = scene["box_data"]["size"]
    wx = float(st[2][0] - sz[2][0])                   # inner face of the +x wall
    wz = float(st[4][2] - sz[4][2])
    m = 1.0 / float(scene["body_properties"]["mass_inverse"][1])
    ke = 0.5 * m * float((vel.astype(np.float64) ** 2).sum(axis=1).mean())
    deg = np.bincount(contact_bodies.reshape(-1).astype(np.int64), minlength=nb + 1)[1:nb + 1]
    top = float(np.percentile(pos[:, 1], 99.0))
    interior = (np.abs(pos[:, 0]) < wx - wall_margin) & (np.abs(pos[:, 2]) < wz - wall_margin) & (pos[:, 1] > wall_margin + 0.5) & (pos[:, 1] < top - 3.0)
    inside = (np.abs(pos[:, 0]) <= wx) & (np.abs(pos[:, 2]) <= wz) & (pos[:, 1] >= 0.0)       # no sphere CENTRE beyond an inner face of the container
    d = deg[interior]
    hist = np.bincount(np.minimum(d, 12), minlength=13) / max(1, len(d))
    return dict(max_pen=float(penetration.max()) if len(penetration) else 0.0, ke=ke, mean_degree=float(d.mean()) if len(d) else 0.0,
                hist=hist, n_interior=int(interior.sum()), inside=float(inside.mean()), top=top, contacts_per_sphere=len(penetration) / nb)


def _reference_pit(nx, ny, nz, seed, checkpoints):
    scene = S.ball_pit(nx, ny, nz, seed=seed)
    ref = refworld.RefWorld(scene, max_contacts=8 * nx * ny * nz)
    out, done = {}, 0
    for s in checkpoints:
        ref.step(s - done); done = s
        b = ref.bodies()
        ref.collide()
        c = ref.contacts()
        out[s] = _pit_stats(scene, b["transforms"]["position"][1:], b["momentum"]["velocity"][1:], c["bodies"], c["data"]["penetration"])
    return out


def _gpu_pit_stats(w, scene):
    c = w.counts()
    assert c["error"] == 0, c
    b = w.get_bodies()
    pos, vel = b["transforms"]["position"][1:], b["momentum"]["velocity"][1:]
    assert np.isfinite(pos).all() and np.isfinite(vel).all() and np.isfinite(b["transforms"]["rotation"]).all()
    k = c["contacts"]                                  # contacts of the step just taken (the list nh_collide left behind)
    g = _pit_stats(scene, pos, vel, w._down("cb", np.uint32, 2 * k).reshape(-1, 2), w._down("cd", S.CONTACT, k)["penetration"])
    g.update(contacts=k, general=c["general_contacts"], colours=c["levels"])
    return g


def test_c4_column_of_160_layers_default_order_vs_reference():
    """The coloured (default) sweep at config 4's PILE HEIGHT on an instance the reference can hold: a 7 x 7 column of 160 layers
    (7840 spheres), checkpoint by checkpoint against the reference stepping the same column.  Chaotic, different Gauss-Seidel order:
    invariants inside bands of the reference's own numbers."""
    _require_reference()
    checkpoints = (150, 300, 450, 600, 800)
    ref = _reference_pit(7, 160, 7, 14, checkpoints)
    scene = S.ball_pit(7, 160, 7, seed=14)
    w = E.World(scene, flags=BENCH_FLAGS, max_contacts=8 * 7840, max_pairs=10 * 7840)            # bench.py's flags (--scene pit)
    done = 0
    for s in checkpoints:
        w.step(s - done); done = s
        g, r = _gpu_pit_stats(w, scene), ref[s]
        print(f"\n[column 7x160x7 step {s}] contacts {g['contacts']} (reference {int(round(r['contacts_per_sphere'] * 7840))}); max penetration {g['max_pen']:.4f} ({r['max_pen']:.4f}); "
              f"KE/sphere {g['ke']:.4e} ({r['ke']:.4e}); top {g['top']:.2f} ({r['top']:.2f}); colours {g['colours']}")
        assert g["inside"] == 1.0 and r["inside"] == 1.0
        # measured (profiles/r02_gpu_tests.log): top within 0.3 %, contacts within 2.5 %, kinetic energy within 12 %, penetration within 1.5 x
        assert abs(g["top"] - r["top"]) <= 0.005 * r["top"] + 0.1, (g["top"], r["top"])
        assert g["max_pen"] <= 1.5 * r["max_pen"] + 0.01, (g["max_pen"], r["max_pen"])
        assert r["ke"] / 1.5 - 1e-3 <= g["ke"] <= 1.5 * r["ke"] + 1e-3, (g["ke"], r["ke"])
        assert abs(g["contacts"] - r["contacts_per_sphere"] * 7840) <= 0.03 * r["contacts_per_sphere"] * 7840 + 50
    w.close()


def test_c4_four_million_sphere_pit_invariants_default_order():
    """BASELINE.json configs[3]: 4,096,000 spheres, 16 iterations, default (graph-coloured) solver order -- a different Gauss-Seidel
    sweep than the reference's, on a chaotic island: parity is statistical.  No instance the reference
    can hold is both as WIDE and as TALL as this pit (a narrow column carries part of its weight on the walls), so the full scene is
    checked through what does transfer: nothing NaN, nobody leaves the container, the pile settles to the reference's packing density,
    interior spheres have the reference's contact-degree distribution, the energy decays, and the residual penetration stays within what
    the reference leaves under the same load per contact (it is proportional to the load: 160 layers here, 20 in the reference's cube)."""
    _require_reference()
    checkpoints = (150, 300, 450, 600, 750)
    cube = _reference_pit(20, 20, 20, 9, (300, 450, 600))        # enough interior spheres for the contact statistics; settled by step 300
    scene = S.ball_pit(160, 160, 160, seed=4)
    nb = len(scene["body_transforms"]) - 1
    assert nb == 4096000
    w = E.World(scene, flags=BENCH_FLAGS, max_contacts=5 * nb, max_pairs=7 * nb)                 # exactly bench.py --scene pit: SINGLE_APPLY | FUSED_STEP
    done, kes, g = 0, [], None
    for s in checkpoints:
        w.step(s - done); done = s
        g = _gpu_pit_stats(w, scene)
        kes.append(g["ke"])
        print(f"\n[pit 160^3 step {s}] contacts {g['contacts']} ({g['contacts_per_sphere']:.3f}/sphere), general {g['general']}, colours {g['colours']}; "
              f"max penetration {g['max_pen']:.4f}; KE/sphere {g['ke']:.4e}; interior degree {g['mean_degree']:.3f} over {g['n_interior']}; top {g['top']:.2f}; inside {g['inside']:.7f}")
        assert g["inside"] == 1.0, "a sphere left the container"
        assert g["max_pen"] <= 0.25, g["max_pen"]                 # never deeper than half a radius, even while 160 layers collapse onto the floor
    rq = cube[600]
    # packing: spheres per unit volume of the settled pile (top = 99th percentile of the centre heights)
    wx = float(scene["box_transforms"]["position"][2][0] - scene["box_data"]["size"][2][0])
    wz = float(scene["box_transforms"]["position"][4][2] - scene["box_data"]["size"][4][2])
    cs = S.ball_pit(20, 20, 20, seed=9)
    cwx = float(cs["box_transforms"]["position"][2][0] - cs["box_data"]["size"][2][0])
    cwz = float(cs["box_transforms"]["position"][4][2] - cs["box_data"]["size"][4][2])
    rho_g, rho_r = 0.99 * nb / (4 * wx * wz * g["top"]), 0.99 * 8000 / (4 * cwx * cwz * rq["top"])
    print(f"\n[pit 160^3 settled] density {rho_g:.4f} spheres per unit volume (reference cube {rho_r:.4f}); interior degree {g['mean_degree']:.3f} (cube {rq['mean_degree']:.3f}); "
          f"max penetration {g['max_pen']:.4f} (cube {rq['max_pen']:.4f} under 1/8 of the load); KE/sphere {kes}")
    assert kes[-1] < 0.02 * max(kes) and kes[-1] < kes[-2], kes      # the collapse is over and the pile keeps calming down
    # density: the 160-layer pile is compressed by its own weight (contacts overlap by up to 13 % of a diameter at the bottom, against 0.6 % in the
    # reference's 20-layer cube): measured 8.7 % denser than the cube; at the SAME pile height the coloured sweep matches the reference's top
    # within 0.3 % (test_c4_column_of_160_layers_default_order_vs_reference)
    assert rho_r <= rho_g <= 1.12 * rho_r, (rho_g, rho_r)
    assert abs(g["mean_degree"] - rq["mean_degree"]) <= 0.05 * rq["mean_degree"], (g["mean_degree"], rq["mean_degree"])     # measured 1.1 %
    assert np.abs(g["hist"] - rq["hist"]).max() <= 0.08, (g["hist"], rq["hist"])
    assert g["max_pen"] <= 0.15, g["max_pen"]                          # calming down: measured 0.13 (0.23 at the height of the collapse)
    w.close()
