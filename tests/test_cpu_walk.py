"""nh_walk's phase machine on the CPU (include/nudge_hip.h, "nh_walk"; nudge_amd/csrc/nh_query.h, "walk"): the host oracle of tests/hostoracle/hostmover.cpp --
the same NH_HD functions the kernel runs, around a brute-force capsule cast -- on the hand-built terrain of tests/walk_batches.py, whose answers are known,
on every invalid-record rule, on the identities against the move oracle (nh_move's bytes; the REPLAY phase by phase), on the shares that keep the GPU
tests' batches honest, and on THE INVARIANT of a random world: a walk that starts free ends no deeper than its skin in anything."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostcapsule_util as HC               # noqa: E402
import hostcast_util as CAST                 # noqa: E402
import hostlib as H                         # noqa: E402
import hostmover_util as MV                 # noqa: E402
import hostpen_util as HP                   # noqa: E402
import hostquery_util as Q                  # noqa: E402
import walk_batches as WB                   # noqa: E402
from hostmover_util import CAPSULE as HW    # noqa: E402
from mover_util import NONE                 # noqa: E402
from query_util import SMALL, unit_quats as _unit_quats      # noqa: E402
from nudge_amd import engine as E          # noqa: E402

R, HH, SKIN = 0.25, 0.5, WB.SKIN            # the upright capsule of the hand-built answers
TOL = 2.0 ** -16 * 64                       # every coordinate of the terrain stays below 64
STAND = SKIN + R + HH                       # the height of its centre above what it stands on
# the shares a batch must reach (conditions on the inputs, the issue's): terrain_walks, and world_walks on the worlds of SMALL
TERRAIN_SHARES = dict(stepped=0.05, snapped=0.05, steep=0.02, grounded=0.40, airborne=0.05)
WORLD_SHARES = dict(grounded=0.25, stepped=0.02)
BALL_PIT_SHARES = dict(grounded=0.10)
# the worlds of SMALL whose bodies rest on the slab or on each other as built: the landed worlds STEPPED >= 2 % is asked of.  The pile is not one of them as
# built or after 50 steps -- its bodies fall from up to 300 units and nothing stands beside anything (STEPPED 0.6 % and 0.5 %) -- so no STEPPED share is
# asserted for it here; tests/test_gpu_walk.py asserts it on the pile once it has landed (1,500 more steps), which needs the GPU to get there.
RESTING = ("compound", "grid_tiles", "stacks")
TERRAIN_SEED, WORLD_SEED = 800, 810


@pytest.fixture(scope="module")
def terrain():
    scene = WB.terrain()
    return Q.records(scene["body_transforms"], scene), len(scene["box_tags"])


def one(terrain, lane, x=1.0, top=0.0, d=(2.0, 0.0, 0.0), **kw):
    """The result of one walk of the capsule (R, HH) standing at x on a top of height `top` in `lane`."""
    rec, nbox = terrain
    w = HW.walks(WB.stand(x, top, WB.LANE[lane], R, HH), d, R, HH, skin=SKIN, **kw)
    return HW.walk(rec, nbox, w)[0]


def has(r, bit):
    return (int(r["flags"]) & bit) != 0


def is_miss(h, t=1.0):
    return h["shape"] == NONE and h["body"] == NONE and h["collider"] == NONE and h["tag"] == NONE and h["t"] == t and (h["normal"] == 0).all()


def test_records_are_the_headers():
    assert E.WALK.itemsize == 96 and E.WALK_RESULT.itemsize == 112
    assert [E.WALK.fields[k][1] for k in E.MOVE.names] == [E.MOVE.fields[k][1] for k in E.MOVE.names]
    assert [E.WALK.fields[k][1] for k in ("up", "step_height", "snap_distance", "min_ground_up", "options", "reserved2")] == [64, 76, 80, 84, 88, 92]
    assert [E.WALK_RESULT.fields[k][1] for k in ("position", "flags", "remaining", "slides", "last_hit", "ground", "step_up", "drop", "casts", "reserved")] == \
           [0, 12, 16, 28, 32, 64, 96, 100, 104, 108]
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "nudge_hip.h")).read()
    assert "#define NH_WALK_MAX_CASTS (2u * (NH_MOVE_MAX_SLIDES + 1u) + 3u)" in text
    assert ("NH_WALK_STEPPED = 0x10u, NH_WALK_GROUNDED = 0x20u, NH_WALK_SNAPPED = 0x40u, NH_WALK_STEEP = 0x80u, NH_WALK_ON_STEEP = 0x100u, "
            "NH_WALK_INVALID = 0x80000000u") in text
    assert "NH_WALK_PROBE_ONLY = 1u" in text
    assert "int nh_walk(nh_context* ctx, const nh_Walk* walks, uint32_t count, nh_WalkResult* results, uint32_t flags /* 0 */);" in text
    assert (E.NH_WALK_STEPPED, E.NH_WALK_GROUNDED, E.NH_WALK_SNAPPED, E.NH_WALK_STEEP, E.NH_WALK_ON_STEEP, E.NH_WALK_INVALID, E.NH_WALK_PROBE_ONLY,
            E.NH_WALK_MAX_CASTS) == (0x10, 0x20, 0x40, 0x80, 0x100, 0x80000000, 1, 21)
    assert "nh_walk" in E.EXPORTS


# ---- hand-built answers on the terrain ------------------------------------------------------------------------------------------------------------------
def test_stairs_are_climbed_with_a_step_height_and_not_without(terrain):
    # four walks of 1.2 along x from the floor in front of the stairs (risers of 0.3 at x = 2, 3, 4, ...): each takes one stair
    p = WB.stand(1.0, 0.0, WB.LANE["stairs"], R, HH)[0]
    rec, nbox = terrain
    for k in range(1, 4):
        w = HW.walks(p, (1.2, 0.0, 0.0), R, HH, skin=SKIN, step_height=0.4, snap_distance=0.3)
        r = HW.walk(rec, nbox, w)[0]
        assert has(r, E.NH_WALK_GROUNDED) and not has(r, E.NH_MOVE_START_OVERLAP)
        p = r["position"]
    assert abs(p[1] - (0.9 + STAND)) <= TOL and p[0] > 4.0                     # on the third tread, 0.9 up, one skin above it
    flat = one(terrain, "stairs", d=(3.0, 0.0, 0.0), step_height=0.0, snap_distance=0.3)
    assert not has(flat, E.NH_WALK_STEPPED) and has(flat, E.NH_MOVE_HIT) and has(flat, E.NH_WALK_GROUNDED)
    assert abs(flat["position"][0] - (2.0 - R - SKIN)) <= TOL and abs(flat["position"][1] - STAND) <= TOL      # stopped by the first riser, on the floor
    up = one(terrain, "stairs", d=(1.2, 0.0, 0.0), step_height=0.4, snap_distance=0.3)
    assert has(up, E.NH_WALK_STEPPED) and has(up, E.NH_WALK_GROUNDED) and up["step_up"] > 0.25 and up["position"][0] > flat["position"][0] + 0.1
    assert up["ground"]["shape"] == E.NH_SHAPE_BOX and up["ground"]["collider"] in (1, 2) and up["casts"] <= 21


def test_the_high_riser_blocks_a_low_step_and_is_climbed_by_a_high_one(terrain):
    low = one(terrain, "riser", step_height=0.4, snap_distance=0.3)
    assert not has(low, E.NH_WALK_STEPPED) and has(low, E.NH_MOVE_HIT) and low["step_up"] == 0
    assert abs(low["position"][0] - (2.0 - R - SKIN)) <= TOL and abs(low["position"][1] - STAND) <= TOL
    assert low["casts"] == 5                                                # A, U, F, D and the probe: the step was tried
    high = one(terrain, "riser", step_height=1.0, snap_distance=0.3)
    assert has(high, E.NH_WALK_STEPPED) and has(high, E.NH_WALK_GROUNDED) and not has(high, E.NH_WALK_SNAPPED)
    assert abs(high["position"][0] - 3.0) <= TOL and abs(high["position"][1] - (0.8 + STAND)) <= TOL and abs(high["step_up"] - 0.8) <= TOL
    assert high["ground"]["collider"] == 6 and abs(high["ground"]["normal"][1] - 1.0) <= TOL and (high["remaining"] == 0).all()
    assert high["casts"] == 4 and high["drop"] == 0                         # A, U, F (free), D: no probe behind a step


def test_the_low_ceiling_vetoes_the_step(terrain):
    for limit in (0.0, float(MV.cos_deg(45.0))):
        r = one(terrain, "ceiling", step_height=0.4, snap_distance=0.3, min_ground_up=limit)
        assert not has(r, E.NH_WALK_STEPPED) and r["step_up"] == 0 and has(r, E.NH_WALK_GROUNDED)
        assert abs(r["position"][0] - (2.0 - R - SKIN)) <= TOL and abs(r["position"][1] - STAND) <= TOL
        assert r["casts"] == 5
    # the same step without the ceiling (the stairs' first riser is the same 0.3) is taken
    assert has(one(terrain, "stairs", step_height=0.4, snap_distance=0.3), E.NH_WALK_STEPPED)


def test_ramps_and_the_slope_limit(terrain):
    lim45 = float(MV.cos_deg(45.0))
    gentle = one(terrain, "ramp20", d=(3.0, 0.0, 0.0), step_height=0.4, snap_distance=0.3, min_ground_up=lim45)
    assert has(gentle, E.NH_WALK_GROUNDED) and not has(gentle, E.NH_WALK_STEEP) and not has(gentle, E.NH_WALK_ON_STEEP)
    assert gentle["position"][1] > STAND + 0.3 and gentle["position"][0] > 3.0
    n = gentle["ground"]["normal"]
    assert abs(n[0] + np.sin(np.deg2rad(20))) <= TOL and abs(n[1] - np.cos(np.deg2rad(20))) <= TOL
    steep = one(terrain, "ramp60", d=(3.0, 0.0, 0.0), snap_distance=0.3, min_ground_up=lim45)
    assert has(steep, E.NH_WALK_STEEP) and not has(steep, E.NH_WALK_STEPPED)
    assert abs(steep["position"][1] - STAND) <= TOL                         # no height gained: the push off the face is horizontal no more than the snap takes back
    assert has(steep, E.NH_WALK_GROUNDED) and abs(steep["ground"]["normal"][1] - 1.0) <= TOL        # it stands on the floor in front of the ramp
    free = one(terrain, "ramp60", d=(3.0, 0.0, 0.0), snap_distance=0.3, min_ground_up=0.0)
    assert not has(free, E.NH_WALK_STEEP) and free["position"][1] > STAND + 0.5 and has(free, E.NH_WALK_GROUNDED)
    assert abs(free["ground"]["normal"][1] - 0.5) <= TOL                    # with the limit off a 60 degree face is ground
    # standing on the 60 degree face under the limit: the probe finds it and says ON_STEEP
    on = HW.walks(free["position"], (0.0, 0.0, 0.0), R, HH, skin=SKIN, snap_distance=0.3, min_ground_up=lim45)
    rec, nbox = terrain
    r = HW.walk(rec, nbox, on)[0]
    assert has(r, E.NH_WALK_ON_STEEP) and not has(r, E.NH_WALK_GROUNDED) and (r["position"] == free["position"]).all() and r["casts"] == 1


def test_ledge_drop_and_probe_only(terrain):
    snap = one(terrain, "ledge", x=1.5, top=0.2, d=(1.5, 0.0, 0.0), snap_distance=0.3)
    assert int(snap["flags"]) == E.NH_WALK_GROUNDED | E.NH_WALK_SNAPPED and snap["slides"] == 0 and snap["casts"] == 2
    # drop is the way down to the contact: the ledge's 0.2 and the skin the capsule stood above the platform; the snap then leaves skin above the floor
    assert abs(snap["drop"] - (0.2 + SKIN)) <= TOL and abs(snap["position"][1] - STAND) <= TOL and abs(snap["position"][0] - 3.0) <= TOL
    assert snap["ground"]["collider"] == 0 and is_miss(snap["last_hit"])
    air = one(terrain, "drop", x=1.5, top=2.0, d=(1.5, 0.0, 0.0), snap_distance=0.3)
    assert int(air["flags"]) == 0 and is_miss(air["ground"]) and air["drop"] == 0 and abs(air["position"][1] - (2.0 + STAND)) <= TOL and air["casts"] == 2
    probe = one(terrain, "ledge", x=1.5, top=0.2, d=(1.5, 0.0, 0.0), snap_distance=0.3, options=E.NH_WALK_PROBE_ONLY)
    assert int(probe["flags"]) == E.NH_WALK_GROUNDED and probe["drop"] == 0 and abs(probe["position"][1] - (0.2 + STAND)) <= TOL
    assert probe["ground"].tobytes() == snap["ground"].tobytes()
    still = one(terrain, "open", d=(0.0, 0.0, 0.0))
    assert int(still["flags"]) == 0 and still["casts"] == 0 and is_miss(still["ground"]) and is_miss(still["last_hit"])


# ---- invalid records ----------------------------------------------------------------------------------------------------------------------------------
def _invalid_cases():
    base = HW.walks(WB.stand(1.0, 0.0, WB.LANE["open"], R, HH), (1.0, 0.0, 0.0), R, HH, skin=SKIN, step_height=0.4, snap_distance=0.3, min_ground_up=0.5)[0]
    cases = []

    def case(name, field, value, index=None):
        w = base.copy()
        if index is None:
            w[field] = value
        else:
            w[field][index] = value
        cases.append((name, w))
    for bad in (np.nan, np.inf, -np.inf):
        case(f"origin {bad}", "origin", bad, 1)
        case(f"displacement {bad}", "displacement", bad, 0)
        case(f"up {bad}", "up", bad, 2)
        case(f"step_height {bad}", "step_height", bad)
        case(f"snap_distance {bad}", "snap_distance", bad)
        case(f"min_ground_up {bad}", "min_ground_up", bad)
        case(f"radius {bad}", "radius", bad)
        case(f"skin {bad}", "skin", bad)
    case("rotation nan", "rotation", np.nan, 0)
    case("radius < 0", "radius", -0.1)
    case("half_height < 0", "half_height", -0.1)
    case("skin < 0", "skin", -0.01)
    case("max_slides 9", "max_slides", 9)
    case("up too long", "up", 1.001, 1)
    case("up too short", "up", 0.999, 1)
    case("up zero", "up", 0.0, 1)
    case("step_height < 0", "step_height", -0.1)
    case("snap_distance < 0", "snap_distance", -0.1)
    case("min_ground_up < 0", "min_ground_up", -0.01)
    case("min_ground_up > 1", "min_ground_up", 1.0000001)
    for bit in (2, 4, 0x80000000, 3):
        case(f"options {bit:#x}", "options", bit)
    return base, cases


def test_invalid_records(terrain):
    rec, nbox = terrain
    base, cases = _invalid_cases()
    w = np.array([c for _, c in cases], dtype=E.WALK)
    out = HW.walk(rec, nbox, w)
    for (name, c), r in zip(cases, out):
        assert r["flags"] == E.NH_WALK_INVALID, name
        assert r["position"].tobytes() == c["origin"].tobytes() and r["remaining"].tobytes() == c["displacement"].tobytes(), name
        assert r["slides"] == 0 and r["casts"] == 0 and r["step_up"] == 0 and r["drop"] == 0 and r["reserved"] == 0, name
        for h in (r["last_hit"], r["ground"]):
            assert h["shape"] == NONE and h["body"] == NONE and np.isnan(h["t"]) and (h["normal"] == 0).all(), name


def test_valid_edges(terrain):
    rec, nbox = terrain
    base, _ = _invalid_cases()
    edges = []
    for field, value, index in (("up", 1.0 + 2.0 ** -12, 1), ("up", 1.0 - 2.0 ** -12, 1), ("min_ground_up", 0.0, None), ("min_ground_up", 1.0, None),
                                ("step_height", 0.0, None), ("snap_distance", 0.0, None), ("options", 1, None), ("max_slides", 8, None), ("max_slides", 0, None),
                                ("reserved", 0xFFFFFFFF, None), ("reserved2", 0xFFFFFFFF, None), ("skin", 0.0, None)):
        w = base.copy()
        if index is None:
            w[field] = value
        else:
            w[field][index] = value
        edges.append(w)
    w = base.copy()
    w["half_height"], w["rotation"] = 0.0, np.nan                          # a ball does not read its rotation
    edges.append(w)
    out = HW.walk(rec, nbox, np.array(edges, dtype=E.WALK))
    assert ((out["flags"] & E.NH_WALK_INVALID) == 0).all()
    ref = HW.walk(rec, nbox, np.array([base], dtype=E.WALK))[0]
    assert out[9].tobytes() == ref.tobytes() and out[10].tobytes() == ref.tobytes()          # `reserved` and `reserved2` are not read


# ---- the batches: shares, identities -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def terrain_run(terrain):
    rec, nbox = terrain
    w = WB.terrain_walks(np.random.default_rng(TERRAIN_SEED), 2048)
    return w, HW.walk(rec, nbox, w)


def check_shares(w, out, need, what):
    got = MV.shares(w, out)
    print(what, {k: round(v, 4) for k, v in got.items()})
    for k, least in need.items():
        assert got[k] >= least, (what, k, got[k], least)
    return got


def test_batch_conditions(terrain_run):
    """What keeps the bit-for-bit tests honest: the batches of tests/test_gpu_walk.py (the same generators, the same seeds) step, snap, meet steep faces,
    stand on ground and walk off ledges often enough.  Conditions on the inputs, asserted on the oracle's output."""
    w, out = terrain_run
    check_shares(w, out, TERRAIN_SHARES, "terrain")
    assert ((out["flags"] & E.NH_WALK_INVALID) == 0).all() and (out["slides"] >= 1).mean() >= 0.25
    for name in sorted(SMALL):
        scene = SMALL[name]()
        rec, nbox = Q.records(scene["body_transforms"], scene), len(scene["box_tags"])
        ww = WB.world_walks(np.random.default_rng(WORLD_SEED + sorted(SMALL).index(name)), rec, nbox, 2048)
        res = HW.walk(rec, nbox, ww)
        need = BALL_PIT_SHARES if name == "ball_pit" else WORLD_SHARES if name in RESTING else dict(grounded=WORLD_SHARES["grounded"])
        check_shares(ww, res, need, name)


def test_results_keep_their_promises(terrain_run):
    """Identity 5: casts never above 21; a GROUNDED result's ground normal is walkable; and what the flags say about each other."""
    w, out = terrain_run
    f = out["flags"]
    assert (out["casts"] <= E.NH_WALK_MAX_CASTS).all() and (out["casts"] >= out["slides"]).all()
    g = (f & E.NH_WALK_GROUNDED) != 0
    u = (out["ground"]["normal"].astype(np.float64) * w["up"]).sum(axis=1)
    assert (u[g] > 0).all() and (u[g] >= w["min_ground_up"][g] - 2.0 ** -22).all() and (out["ground"]["shape"][g] != NONE).all()
    stepped, snapped = (f & E.NH_WALK_STEPPED) != 0, (f & E.NH_WALK_SNAPPED) != 0
    assert (g[stepped]).all() and (g[snapped]).all() and not (stepped & snapped).any()
    assert (out["step_up"][~stepped] == 0).all() and (out["drop"][~snapped] == 0).all() and (out["drop"][snapped] > 0).all()
    assert not (snapped & ((w["options"] & E.NH_WALK_PROBE_ONLY) != 0)).any()
    assert not (stepped & (w["step_height"] == 0)).any() and not (((f & E.NH_WALK_STEEP) != 0) & (w["min_ground_up"] == 0)).any()
    assert not (g & ((f & E.NH_WALK_ON_STEEP) != 0)).any()


def test_without_its_rules_a_walk_is_nh_move(terrain, terrain_run):
    """Identity 1: step_height = snap_distance = min_ground_up = 0 writes nh_move's 64 bytes, and the miss record as ground."""
    rec, nbox = terrain
    w = terrain_run[0].copy()
    w["step_height"], w["snap_distance"], w["min_ground_up"] = 0.0, 0.0, 0.0
    out = HW.walk(rec, nbox, w)
    ref, made = HW.move(rec, nbox, HW.head(w), casts=True)
    assert out.view(np.uint8).reshape(-1, 112)[:, :64].tobytes() == ref.tobytes()
    assert all(is_miss(h) for h in out["ground"]) and (out["step_up"] == 0).all() and (out["drop"] == 0).all() and (out["casts"] == made).all()
    assert (ref["slides"] >= 1).mean() >= 0.25


def test_replay_phase_by_phase(terrain, terrain_run):
    """Identity 2 on the CPU: the phases run one call at a time -- the move oracle for A, U, F and D, the capsule cast oracle for C, nh_query.h's decisions
    between them -- give the walk oracle's 112 bytes."""
    rec, nbox = terrain
    w = terrain_run[0].copy()
    w["min_ground_up"] = 0.0
    out = HW.walk(rec, nbox, w)
    got, calls = HW.replay_walk(w, lambda m: HW.move(rec, nbox, m), lambda c: CAST.cast(CAST.CAPSULE, rec, nbox, c))
    bad = (got.view(np.uint8).reshape(-1, 112) != out.view(np.uint8).reshape(-1, 112)).any(axis=1)
    assert not bad.any(), (int(bad.sum()), out[np.argmax(bad)], got[np.argmax(bad)])
    s = MV.shares(w, out)
    assert s["stepped"] >= 0.05 and s["snapped"] >= 0.05 and calls >= 6


# ---- THE INVARIANT --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_run():
    """test_cpu_move's random world -- boxes and spheres of size 0.2 - 2 under random rotations in a cube of side 40 -- and walks of upright capsules from
    uniform origins by 0.5 - 3 units, mostly horizontal, with the rules drawn as the batches draw them."""
    rng = np.random.default_rng(21)
    n_boxes, n_spheres, side, n = 2000, 1000, 40.0, 20000
    rec = np.zeros(n_boxes + n_spheres, dtype=H.REC)
    rec["p"] = rng.uniform(-side / 2, side / 2, size=(len(rec), 3))
    rec["q"] = _unit_quats(rng, len(rec))
    rec["h"][:n_boxes] = rng.uniform(0.1, 1.0, size=(n_boxes, 3))
    rec["h"][n_boxes:] = rng.uniform(0.1, 1.0, size=(n_spheres, 1))
    rec["tag"] = rng.integers(0, 1 << 30, size=len(rec))
    o = rng.uniform(-side / 2, side / 2, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)) * (1.0, 0.15, 1.0)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 3.0, size=(n, 1))).astype(np.float32)
    w = WB._draw_rules(rng, HW.walks(o, d, R, HH, skin=SKIN))
    out = HW.walk(rec, n_boxes, w)
    q = np.zeros(n, dtype=E.OVERLAP_QUERY)
    q["center"], q["shape"], q["rotation"], q["ignore_body"] = w["origin"], E.NH_SHAPE_CAPSULE, w["rotation"], NONE
    q["size"][:, 0], q["size"][:, 1] = R, HH
    free = np.diff(HC.overlap(rec, n_boxes, q)[0].astype(np.int64)) == 0
    return rec, n_boxes, w, out, free


def test_invariant_conditions(random_run):
    """What keeps the invariant honest: enough walks start free, and enough of those slide, step, snap and meet steep faces."""
    _, _, w, out, free = random_run
    s = MV.shares(w[free], out[free])
    print("free %.3f, of them: %s" % (free.mean(), {k: round(v, 4) for k, v in s.items()}))
    assert free.mean() >= 0.5
    assert s["slid"] >= 0.25 and s["stepped"] >= 0.01 and s["snapped"] >= 0.02 and s["steep"] >= 0.02
    assert (out["flags"] & E.NH_WALK_INVALID == 0).all() and (out["casts"] <= E.NH_WALK_MAX_CASTS).all()


def test_invariant(random_run):
    """A walk that starts free ends at most skin + 2^-16 C deep in anything (C: the largest coordinate plus extent of the scene): test_cpu_move's bound, and
    its derivation holds -- every position a walk keeps is the end of a move loop (the push skin * n can enter a neighbour by at most skin; the reach rule
    delays a hit by at most the leaf pad plus the cast pad, 2 * 2^-18 of the coordinates; four times that is the 2^-16), and the snap is one more such
    advance along the probe's cast."""
    rec, nbox, w, out, free = random_run
    C = float(max(np.abs(rec["p"]).max() + np.sqrt(3.0) * rec["h"].max(), np.abs(w["origin"]).max() + np.abs(w["displacement"]).max() + R + HH + 2.2 + 0.3))
    tol = 2.0 ** -16 * C
    q = np.zeros(len(w), dtype=E.OVERLAP_QUERY)
    q["center"], q["shape"], q["rotation"], q["ignore_body"] = out["position"], E.NH_SHAPE_CAPSULE, w["rotation"], NONE
    q["size"][:, 0], q["size"][:, 1] = R, HH
    off, hits, total = HP.penetration(rec, nbox, q)
    depth = np.zeros(len(w))
    if total:
        np.maximum.at(depth, np.repeat(np.arange(len(w)), np.diff(off.astype(np.int64))), hits["depth"][:total].astype(np.float64))
    print("deepest end of a free walk: %.6f (bound %.6f); ends touching something: %d of %d" % (depth[free].max(), SKIN + tol, (depth[free] > 0).sum(), free.sum()))
    assert (depth[free] <= SKIN + tol).all()
