"""nh_boxwalk's phase machine on the CPU (include/nudge_hip.h, "nh_boxmove, nh_boxwalk"; nudge_amd/csrc/nh_query.h, "walk"): the host oracle of
tests/hostoracle/hostmover.cpp -- the NH_HD functions the kernel runs, around a brute-force box cast -- against the replay phase by phase through
test_cpu_boxmove's replay round by round, on the hand-built terrain of tests/walk_batches.py for the upright box (0.25, 0.75, 0.25), on every
invalid-record rule, on the identities, on the shares that keep the GPU tests' batches honest, and on THE INVARIANT of a random world."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boxwalk_batches as BWB               # noqa: E402
import hostcast_util as CAST                 # noqa: E402
import hostmover_util as MV                 # noqa: E402
import hostlib as H                         # noqa: E402
import hostoverlap_util as HO               # noqa: E402
import hostquery_util as Q                  # noqa: E402
import walk_batches as WB                   # noqa: E402
from hostmover_util import BOX as HBW       # noqa: E402
from mover_util import NONE                 # noqa: E402
from query_util import SMALL, unit_quats as _unit_quats      # noqa: E402
from test_cpu_boxmove import deepest        # noqa: E402
from test_cpu_walk import BALL_PIT_SHARES, RESTING, TERRAIN_SHARES, TOL, WORLD_SHARES, check_shares, has, is_miss      # noqa: E402
from nudge_amd import engine as E          # noqa: E402

BOX, SKIN = BWB.BOX, BWB.SKIN               # the upright box of the hand-built answers
HX, HY, HZ = BOX
STAND = SKIN + HY                           # the height of its centre above what it stands on
TERRAIN_SEED, WORLD_SEED = 820, 830


@pytest.fixture(scope="module")
def terrain():
    scene = WB.terrain()
    return Q.records(scene["body_transforms"], scene), len(scene["box_tags"])


def one(terrain, lane, x=1.0, top=0.0, d=(2.0, 0.0, 0.0), **kw):
    """The result of one walk of the box BOX standing at x on a top of height `top` in `lane`."""
    rec, nbox = terrain
    w = HBW.walks(BWB.stand(x, top, WB.LANE[lane], HY), d, BOX, skin=SKIN, **kw)
    return HBW.walk(rec, nbox, w)[0]


def test_records_are_the_headers():
    assert E.BOX_WALK.itemsize == 96
    assert [E.BOX_WALK.fields[k][1] for k in E.BOX_MOVE.names] == [E.BOX_MOVE.fields[k][1] for k in E.BOX_MOVE.names]
    tail = ("up", "step_height", "snap_distance", "min_ground_up", "options", "reserved2")
    assert [E.BOX_WALK.fields[k][1] for k in tail] == [64, 76, 80, 84, 88, 92] == [E.WALK.fields[k][1] for k in tail]
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "nudge_hip.h")).read()
    assert ("typedef struct nh_BoxWalk { float origin[3]; float skin; float displacement[3]; uint32_t ignore_body;\n"
            "                            float rotation[4]; float size[3]; uint32_t max_slides;") in text
    assert "uint32_t options; uint32_t reserved2; } nh_BoxWalk;" in text
    assert "int nh_boxwalk(nh_context* ctx, const nh_BoxWalk* walks, uint32_t count, nh_WalkResult* results, uint32_t flags /* 0 */);" in text
    assert "nh_boxwalk" in E.EXPORTS and callable(E.World.boxwalk) and callable(E.World.boxwalk_records)


# ---- hand-built answers on the terrain ------------------------------------------------------------------------------------------------------------------
def test_stairs_are_climbed_with_a_step_height_and_not_without(terrain):
    p = BWB.stand(1.0, 0.0, WB.LANE["stairs"], HY)[0]
    rec, nbox = terrain
    for k in range(1, 4):
        r = HBW.walk(rec, nbox, HBW.walks(p, (1.2, 0.0, 0.0), BOX, skin=SKIN, step_height=0.4, snap_distance=0.3))[0]
        assert has(r, E.NH_WALK_GROUNDED) and not has(r, E.NH_MOVE_START_OVERLAP)
        p = r["position"]
    assert abs(p[1] - (0.9 + STAND)) <= TOL and p[0] > 4.0                     # on the third tread, 0.9 up, one skin above it
    flat = one(terrain, "stairs", d=(3.0, 0.0, 0.0), step_height=0.0, snap_distance=0.3)
    assert not has(flat, E.NH_WALK_STEPPED) and has(flat, E.NH_MOVE_HIT) and has(flat, E.NH_WALK_GROUNDED)
    assert abs(flat["position"][0] - (2.0 - HX - SKIN)) <= TOL and abs(flat["position"][1] - STAND) <= TOL      # stopped by the first riser, on the floor


def test_the_high_riser_blocks_a_low_step_and_is_climbed_by_a_high_one(terrain):
    low = one(terrain, "riser", step_height=0.4, snap_distance=0.3)
    assert not has(low, E.NH_WALK_STEPPED) and has(low, E.NH_MOVE_HIT) and low["step_up"] == 0
    assert abs(low["position"][0] - (2.0 - HX - SKIN)) <= TOL and abs(low["position"][1] - STAND) <= TOL
    assert low["casts"] == 5                                                # A, U, F, D and the probe: the step was tried
    high = one(terrain, "riser", step_height=1.0, snap_distance=0.3)
    assert has(high, E.NH_WALK_STEPPED) and has(high, E.NH_WALK_GROUNDED) and not has(high, E.NH_WALK_SNAPPED)
    assert abs(high["position"][0] - 3.0) <= TOL and abs(high["position"][1] - (0.8 + STAND)) <= TOL and abs(high["step_up"] - 0.8) <= TOL
    assert high["ground"]["collider"] == 6 and abs(high["ground"]["normal"][1] - 1.0) <= TOL
    assert high["casts"] == 4 and high["drop"] == 0                         # A, U, F (free), D: no probe behind a step


def test_the_low_ceiling_vetoes_the_step(terrain):
    r = one(terrain, "ceiling", step_height=0.4, snap_distance=0.3)
    assert not has(r, E.NH_WALK_STEPPED) and r["step_up"] == 0 and r["casts"] == 5
    assert abs(r["position"][0] - (2.0 - HX - SKIN)) <= TOL and abs(r["position"][1] - STAND) <= TOL


def test_ledge_drop_and_probe_only(terrain):
    snap = one(terrain, "ledge", x=1.5, top=0.2, d=(1.5, 0.0, 0.0), snap_distance=0.3)
    assert int(snap["flags"]) == E.NH_WALK_GROUNDED | E.NH_WALK_SNAPPED and snap["casts"] == 2
    assert abs(snap["drop"] - (0.2 + SKIN)) <= TOL and abs(snap["position"][0] - 3.0) <= TOL and abs(snap["position"][1] - STAND) <= TOL
    probe = one(terrain, "ledge", x=1.5, top=0.2, d=(1.5, 0.0, 0.0), snap_distance=0.3, options=E.NH_WALK_PROBE_ONLY)
    assert int(probe["flags"]) == E.NH_WALK_GROUNDED and probe["drop"] == 0 and abs(probe["position"][1] - (0.2 + STAND)) <= TOL
    assert probe["ground"].tobytes() == snap["ground"].tobytes()
    air = one(terrain, "drop", x=1.5, top=2.0, d=(1.5, 0.0, 0.0), snap_distance=0.3)
    assert int(air["flags"]) == 0 and is_miss(air["ground"]) and air["casts"] == 2 and air["drop"] == 0
    still = one(terrain, "open", d=(0.0, 0.0, 0.0))
    assert int(still["flags"]) == 0 and still["casts"] == 0 and is_miss(still["ground"]) and is_miss(still["last_hit"])


def test_ramps_and_the_slope_limit(terrain):
    lim45 = float(MV.cos_deg(45.0))
    gentle = one(terrain, "ramp20", d=(3.0, 0.0, 0.0), step_height=0.4, snap_distance=0.3, min_ground_up=lim45)
    assert has(gentle, E.NH_WALK_GROUNDED) and not has(gentle, E.NH_WALK_STEEP) and not has(gentle, E.NH_WALK_ON_STEEP)
    n = gentle["ground"]["normal"]
    assert abs(n[0] + np.sin(np.deg2rad(20))) <= TOL and abs(n[1] - np.cos(np.deg2rad(20))) <= TOL
    steep = one(terrain, "ramp60", d=(3.0, 0.0, 0.0), snap_distance=0.3, min_ground_up=lim45)
    assert has(steep, E.NH_WALK_STEEP) and not has(steep, E.NH_WALK_STEPPED)
    assert abs(steep["position"][1] - STAND) <= TOL                         # no height gained
    free = one(terrain, "ramp60", d=(3.0, 0.0, 0.0), snap_distance=0.3, min_ground_up=0.0)
    assert not has(free, E.NH_WALK_STEEP) and has(free, E.NH_WALK_GROUNDED)
    assert abs(free["ground"]["normal"][1] - 0.5) <= TOL                    # with the limit off a 60 degree face is ground


# ---- invalid records ----------------------------------------------------------------------------------------------------------------------------------
def _invalid_cases():
    base = HBW.walks(BWB.stand(1.0, 0.0, WB.LANE["open"], HY), (1.0, 0.0, 0.0), BOX, skin=SKIN, step_height=0.4, snap_distance=0.3, min_ground_up=0.5)[0]
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
        for k in range(3):
            case(f"size[{k}] {bad}", "size", bad, k)
        case(f"skin {bad}", "skin", bad)
    for k in range(4):
        case(f"rotation[{k}] nan", "rotation", np.nan, k)
    for k in range(3):
        case(f"size[{k}] < 0", "size", -0.1, k)
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
    w = np.array([c for _, c in cases], dtype=E.BOX_WALK)
    out = HBW.walk(rec, nbox, w)
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
    for field, value, index in (("reserved2", 0xFFFFFFFF, None), ("up", 1.0 + 2.0 ** -12, 1), ("up", 1.0 - 2.0 ** -12, 1), ("min_ground_up", 0.0, None),
                                ("min_ground_up", 1.0, None), ("step_height", 0.0, None), ("snap_distance", 0.0, None), ("options", 1, None),
                                ("max_slides", 8, None), ("max_slides", 0, None), ("skin", 0.0, None), ("size", 0.0, 0), ("size", 0.0, 1), ("size", 0.0, 2)):
        w = base.copy()
        if index is None:
            w[field] = value
        else:
            w[field][index] = value
        edges.append(w)
    w = base.copy()
    w["size"], w["rotation"] = 0.0, np.nan                                 # a ray does not read its rotation
    edges.append(w)
    out = HBW.walk(rec, nbox, np.array(edges, dtype=E.BOX_WALK))
    assert ((out["flags"] & E.NH_WALK_INVALID) == 0).all()
    ref = HBW.walk(rec, nbox, np.array([base], dtype=E.BOX_WALK))[0]
    assert out[0].tobytes() == ref.tobytes()                                # `reserved2` is not read


# ---- the batches: shares, identities -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def terrain_run(terrain):
    rec, nbox = terrain
    w = BWB.terrain_walks(np.random.default_rng(TERRAIN_SEED), 2048)
    return w, HBW.walk(rec, nbox, w)


def test_batch_conditions(terrain_run):
    """What keeps the bit-for-bit tests honest: the batches of tests/test_gpu_boxwalk.py (the same generators, the same seeds) step, snap, meet steep
    faces, stand on ground and walk off ledges often enough: test_cpu_walk's shares, asserted on the oracle's output."""
    w, out = terrain_run
    check_shares(w, out, TERRAIN_SHARES, "terrain")
    assert ((out["flags"] & E.NH_WALK_INVALID) == 0).all() and (out["slides"] >= 1).mean() >= 0.25
    for name in sorted(SMALL):
        scene = SMALL[name]()
        rec, nbox = Q.records(scene["body_transforms"], scene), len(scene["box_tags"])
        ww = BWB.world_walks(np.random.default_rng(WORLD_SEED + sorted(SMALL).index(name)), rec, nbox, 2048)
        res = HBW.walk(rec, nbox, ww)
        need = BALL_PIT_SHARES if name == "ball_pit" else WORLD_SHARES if name in RESTING else dict(grounded=WORLD_SHARES["grounded"])
        check_shares(ww, res, need, name)


def test_results_keep_their_promises(terrain_run):
    """Identity 7: casts never above 21; a GROUNDED result's ground normal is walkable; and what the flags say about each other."""
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


def test_without_its_rules_a_walk_is_nh_boxmove(terrain, terrain_run):
    """Identity 4: step_height = snap_distance = min_ground_up = 0 writes nh_boxmove's 64 bytes, and the miss record as ground."""
    rec, nbox = terrain
    w = terrain_run[0].copy()
    w["step_height"], w["snap_distance"], w["min_ground_up"] = 0.0, 0.0, 0.0
    out = HBW.walk(rec, nbox, w)
    ref, made = HBW.move(rec, nbox, HBW.head(w), casts=True)
    assert out.view(np.uint8).reshape(-1, 112)[:, :64].tobytes() == ref.tobytes()
    assert all(is_miss(h) for h in out["ground"]) and (out["step_up"] == 0).all() and (out["drop"] == 0).all() and (out["casts"] == made).all()
    assert (ref["slides"] >= 1).mean() >= 0.25


def test_the_oracle_equals_the_replay_through_the_old_oracles(terrain, terrain_run):
    """hw_walk for boxes with min_ground_up = 0 against replay_walk -- hostmover.cpp's phase-by-phase helpers -- whose move records are answered by a
    Python loop around hostcast.cpp's box cast and the capsule mover's begin / advance (test_cpu_boxmove) and whose cast records by that cast itself.
    Identity 5 on the CPU."""
    from test_cpu_boxmove import _replay_old
    rec, nbox = terrain
    w = terrain_run[0].copy()
    w["min_ground_up"] = 0.0
    out = HBW.walk(rec, nbox, w)
    got, calls = HBW.replay_walk(w, lambda m: _replay_old(rec, nbox, m), lambda c: CAST.cast(CAST.BOX, rec, nbox, c))
    bad = (got.view(np.uint8).reshape(-1, 112) != out.view(np.uint8).reshape(-1, 112)).any(axis=1)
    assert not bad.any(), (int(bad.sum()), out[np.argmax(bad)], got[np.argmax(bad)])
    s = MV.shares(w, out)
    assert s["stepped"] >= 0.05 and s["snapped"] >= 0.05 and calls >= 6


# ---- THE INVARIANT --------------------------------------------------------------------------------------------------------------------------------
HALF = (0.3, 0.5, 0.4)


@pytest.fixture(scope="module")
def random_run():
    """test_cpu_move's random world -- boxes and spheres of size 0.2 - 2 under random rotations in a cube of side 40 -- and walks of boxes of half extents
    HALF under random rotations from uniform origins by 0.5 - 3 units, mostly horizontal, with the rules drawn as the batches draw them."""
    rng = np.random.default_rng(22)
    n_boxes, n_spheres, side, n = 2000, 1000, 40.0, 12000
    rec = np.zeros(n_boxes + n_spheres, dtype=H.REC)
    rec["p"] = rng.uniform(-side / 2, side / 2, size=(len(rec), 3))
    rec["q"] = _unit_quats(rng, len(rec))
    rec["h"][:n_boxes] = rng.uniform(0.1, 1.0, size=(n_boxes, 3))
    rec["h"][n_boxes:] = rng.uniform(0.1, 1.0, size=(n_spheres, 1))
    rec["tag"] = rng.integers(0, 1 << 30, size=len(rec))
    o = rng.uniform(-side / 2, side / 2, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)) * (1.0, 0.15, 1.0)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 3.0, size=(n, 1))).astype(np.float32)
    w = WB._draw_rules(rng, HBW.walks(o, d, HALF, rotations=_unit_quats(rng, n), skin=SKIN))
    out = HBW.walk(rec, n_boxes, w)
    free = np.diff(HO.overlap(rec, n_boxes, HBW.overlap_queries(w))[0].astype(np.int64)) == 0
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
    """A box walk that starts free ends at most skin + 2^-16 C deep in anything: test_cpu_walk's bound (C: the largest coordinate plus extent of the
    scene, the largest step height and snap distance added) with the box's half diagonal in place of R + HH.  Every position a walk keeps is the end of a
    move loop, and the snap is one more such advance along the probe's cast, whatever the shape."""
    rec, nbox, w, out, free = random_run
    diag = float(np.linalg.norm(HALF))
    C = float(max(np.abs(rec["p"]).max() + np.sqrt(3.0) * rec["h"].max(), np.abs(w["origin"]).max() + np.abs(w["displacement"]).max() + diag + 2.2 + 0.3))
    tol = 2.0 ** -16 * C
    depth = deepest(rec, nbox, out["position"], w["rotation"], w["size"])
    print("deepest end of a free box walk: %.6f (bound %.6f); ends touching something: %d of %d" % (depth[free].max(), SKIN + tol, (depth[free] > 0).sum(), free.sum()))
    assert (depth[free] <= SKIN + tol).all()
