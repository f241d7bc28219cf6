"""nh_move_touched, nh_boxmove_touched, nh_walk_touched and nh_boxwalk_touched on the CPU (include/nudge_hip.h, "nh_move_touched"): the declarations, and
the host oracle of tests/hostoracle/hosttouch.cpp -- the movers' loops around a brute-force cast, which also list every collider a cast found -- against
the plain movers' oracle (T1), against the cast oracle touch by touch (T2), on the identities T3 - T5, on hand-built worlds whose lists are known, and on
the conditions that keep the GPU tests' batches honest."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostcast_util as CAST                 # noqa: E402
import hostquery_util as Q                  # noqa: E402
import hosttouch_util as HT                 # noqa: E402
import touched_batches as TB                # noqa: E402
import walk_batches as WB                   # noqa: E402
from mover_util import NONE, SENTINEL       # noqa: E402
from query_util import SMALL                # noqa: E402
from test_cpu_move import FLOOR, _random_world_and_moves, world      # noqa: E402
from test_cpu_walk import TERRAIN_SHARES    # noqa: E402
from nudge_amd import engine as E          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, HH, SKIN = 0.5, 0.5, 0.01                # the upright capsule of the hand-built moves
WR, WHH = 0.25, 0.5                         # ... and of the hand-built walks
BOX_HALF = (0.3, 0.5, 0.4)
TOL = 2.0 ** -16 * 64
SHAPES = sorted(TB.SHAPES)
NAMES = ("nh_move_touched", "nh_boxmove_touched", "nh_walk_touched", "nh_boxwalk_touched")


def header():
    return open(os.path.join(ROOT, "include", "nudge_hip.h")).read()


def sentinel(n, k):
    return np.full((n, k, 64), SENTINEL, dtype=np.uint8).view(E.TOUCH).reshape(n, k)


def unwritten_keep_the_sentinel(counts, touches):
    raw = touches.view(np.uint8).reshape(len(touches), touches.shape[1], 64)
    return bool((raw[~HT.written(counts, touches.shape[1])] == SENTINEL).all())


# ---- declarations ---------------------------------------------------------------------------------------------------------------------------------
def test_records_are_the_headers():
    assert E.TOUCH.itemsize == 64 and E.TOUCH.names[0] == "hit" and E.TOUCH.fields["hit"][0] == E.RAY_HIT
    assert [E.TOUCH.fields[k][1] for k in ("hit", "origin", "phase", "direction", "cast")] == [0, 32, 44, 48, 60]
    assert (E.NH_TOUCH_SLIDE, E.NH_TOUCH_UP, E.NH_TOUCH_FORWARD, E.NH_TOUCH_DOWN, E.NH_TOUCH_PROBE) == (0, 1, 2, 3, 4)
    text = header()
    assert "enum { NH_TOUCH_SLIDE = 0u, NH_TOUCH_UP = 1u, NH_TOUCH_FORWARD = 2u, NH_TOUCH_DOWN = 3u, NH_TOUCH_PROBE = 4u };" in text
    assert "typedef struct nh_Touch { nh_RayHit hit; float origin[3]; uint32_t phase; float direction[3]; uint32_t cast; } nh_Touch;   /* 64 B */" in text
    for line in (
            "int nh_move_touched   (nh_context* ctx, const nh_Move* moves,    uint32_t count, nh_MoveResult* results, uint32_t k, uint32_t* counts, nh_Touch* touches, uint32_t flags /* 0 */);",
            "int nh_boxmove_touched(nh_context* ctx, const nh_BoxMove* moves, uint32_t count, nh_MoveResult* results, uint32_t k, uint32_t* counts, nh_Touch* touches, uint32_t flags /* 0 */);",
            "int nh_walk_touched   (nh_context* ctx, const nh_Walk* walks,    uint32_t count, nh_WalkResult* results, uint32_t k, uint32_t* counts, nh_Touch* touches, uint32_t flags /* 0 */);",
            "int nh_boxwalk_touched(nh_context* ctx, const nh_BoxWalk* walks, uint32_t count, nh_WalkResult* results, uint32_t k, uint32_t* counts, nh_Touch* touches, uint32_t flags /* 0 */);"):
        assert line in text, line
    for name in NAMES:
        assert name in E.EXPORTS
        assert callable(getattr(E.World, name[3:] + "_records"))
    assert HT.MOVE_K == 9 and HT.WALK_K == 21


def test_the_library_exports_the_four_symbols():
    so = os.path.join(ROOT, "nudge_amd", "libnudge_hip.so")
    names = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.split()
    for name in NAMES:
        assert name in names, name


def test_the_header_lists_the_new_observers_and_no_touch_list_as_not_built():
    text = header()
    note = next(line for line in text.splitlines() if "The scene queries (nh_query_build" in line)
    for name in NAMES:
        assert re.search(r"\b%s\b" % name, note), name
    blocks = re.findall(r"(?is)not built:.*?(?:\*/|\n\s*\n|Cost:)", text)
    assert len(blocks) >= 4
    for block in blocks:
        assert "everything touched" not in re.sub(r"\s+", " ", block.lower()), block[:200]
    assert "twenty-five query calls" in text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "10.20" in design


# ---- the runs the tests below share ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def terrain():
    scene = WB.terrain()
    return Q.records(scene["body_transforms"], scene), len(scene["box_tags"])


@functools.lru_cache(maxsize=None)
def random_moves(shape):
    """test_cpu_move's random world and its moves (for the box: the same origins, displacements, rotations and slide counts), by both oracles."""
    rec, nbox, m = _random_world_and_moves(seed=41, n_moves=2048)
    T = TB.SHAPES[shape]
    if shape == "box":
        m = T.mover.moves(m["origin"], m["displacement"], BOX_HALF, rotations=m["rotation"], skin=SKIN, max_slides=m["max_slides"])
        m["size"][::7] = 0.0                                               # rays among them
    else:
        m["half_height"][::7] = 0.0                                        # balls
    m["origin"][5::97, 1] = np.nan                                         # and invalid records
    return (rec, nbox, m) + T.move(rec, nbox, m, touches=sentinel(len(m), HT.MOVE_K))


@functools.lru_cache(maxsize=None)
def terrain_run(shape):
    rec, nbox = terrain()
    w = TB.terrain_walks(shape)
    return (rec, nbox, w) + TB.SHAPES[shape].walk(rec, nbox, w, touches=sentinel(len(w), HT.WALK_K))


# ---- T1, T2: against the oracles that were there ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_results_are_the_plain_oracles_and_unwritten_slots_stay(shape):
    T = TB.SHAPES[shape]
    rec, nbox, m, out, counts, touches = random_moves(shape)
    assert out.tobytes() == T.mover.move(rec, nbox, m).tobytes()
    assert unwritten_keep_the_sentinel(counts, touches) and (counts >= 1).mean() >= 0.25
    rec, nbox, w, out, counts, touches = terrain_run(shape)
    assert out.tobytes() == T.mover.walk(rec, nbox, w).tobytes()
    assert unwritten_keep_the_sentinel(counts, touches) and (counts >= 1).mean() >= 0.25


@pytest.mark.parametrize("shape", SHAPES)
def test_every_touch_replays_as_a_cast(shape):
    """T2: each touch's hit is the closest-hit cast's record for { origin, 1, direction, ignore_body, rotation, the shape }."""
    T = TB.SHAPES[shape]
    for run in (random_moves, terrain_run):
        rec, nbox, records, _, counts, touches = run(shape)
        casts, _, hits = T.touch_casts(records, counts, touches)
        assert len(casts) == int(np.minimum(counts, touches.shape[1]).sum()) and len(casts) > 500
        assert CAST.cast(T.cast, rec, nbox, casts).tobytes() == hits.tobytes()
        assert (hits["shape"] != NONE).all()


# ---- T3, T4, T5 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_move_identities(shape):
    _, _, m, out, counts, touches = random_moves(shape)
    assert HT.check_move_identities(out, counts, touches, shape) > 500
    assert (counts[out["flags"] == E.NH_MOVE_INVALID] == 0).all() and (out["flags"] == E.NH_MOVE_INVALID).sum() >= 10
    # origin and direction of the first touch are the record's own bits
    first = counts >= 1
    assert touches["origin"][first, 0].tobytes() == m["origin"][first].tobytes() and touches["direction"][first, 0].tobytes() == m["displacement"][first].tobytes()


@pytest.mark.parametrize("shape", SHAPES)
def test_walk_identities(shape):
    _, _, w, out, counts, touches = terrain_run(shape)
    assert HT.check_walk_identities(out, counts, touches, shape) > 500
    stepped = (out["flags"] & E.NH_WALK_STEPPED) != 0
    assert stepped.sum() >= 50 and (~stepped & (out["ground"]["shape"] != NONE)).sum() >= 50


@pytest.mark.parametrize("shape", SHAPES)
def test_a_smaller_k_writes_the_same_counts_and_the_same_first_touches(shape):
    T = TB.SHAPES[shape]
    for run, call in ((random_moves, T.move), (terrain_run, T.walk)):
        rec, nbox, records, out, counts, touches = run(shape)
        # (k = 1 cuts lists short on both batches; k = 3 does on the walks, whose lists are longer)
        assert (counts > 1).mean() >= 0.02 and (run is random_moves or (counts > 3).sum() >= 10), np.bincount(counts).tolist()
        for k in (1, 3):
            o, c, t = call(rec, nbox, records, k=k, touches=sentinel(len(records), k))
            assert o.tobytes() == out.tobytes()
            HT.same_touches(t, c, touches, counts, f"{shape} k = {k}")
            assert unwritten_keep_the_sentinel(c, t)


# ---- hand-built worlds -------------------------------------------------------------------------------------------------------------------------------
WALL = ((3.0, 2.0, 0.0), (1.0, 5.0, 8.0))            # its face at x = 2


def test_floor_then_wall():
    rec, nbox = world(boxes=[FLOOR, WALL])
    T = HT.CAPSULE
    m = T.mover.moves([(0.0, 1.2, 0.0)], [(3.0, -1.0, 0.0)], R, HH, skin=SKIN)
    out, counts, touches = T.move(rec, nbox, m, touches=sentinel(1, HT.MOVE_K))
    assert counts[0] == 2 and out["slides"][0] == 2 and out["last_hit"][0]["tag"] == 101
    t = touches[0]
    assert t["hit"]["tag"][:2].tolist() == [100, 101] and t["cast"][:2].tolist() == [0, 1] and t["phase"][:2].tolist() == [0, 0]
    assert t["hit"]["normal"][0].tolist() == [0.0, 1.0, 0.0] and t["hit"]["normal"][1].tolist() == [-1.0, 0.0, 0.0]
    assert t["origin"][0].tolist() == [0.0, np.float32(1.2), 0.0] and t["direction"][0].tolist() == [3.0, -1.0, 0.0]
    assert abs(t["origin"][1][1] - (1.0 + SKIN)) <= TOL and abs(t["direction"][1][0] - 2.4) <= TOL and t["direction"][1][1] == 0
    assert unwritten_keep_the_sentinel(counts, touches)
    # the box mover: the same list
    B = HT.BOX
    bm = B.mover.moves([(0.0, 1.2, 0.0)], [(3.0, -1.0, 0.0)], (0.5, 1.0, 0.5), skin=SKIN)
    _, bc, bt = B.move(rec, nbox, bm)
    assert bc[0] == 2 and bt[0]["hit"]["tag"][:2].tolist() == [100, 101] and bt[0]["cast"][:2].tolist() == [0, 1]
    # ignore_body: every collider here belongs to body 0
    m["ignore_body"] = 0
    out, counts, touches = T.move(rec, nbox, m, touches=sentinel(1, HT.MOVE_K))
    assert counts[0] == 0 and out["flags"][0] == 0 and unwritten_keep_the_sentinel(counts, touches)
    # a mask that hides the floor's layer: the wall alone is touched, on the way down through where the floor was
    m["ignore_body"] = NONE
    words = np.array([1, 2], dtype=np.uint32)
    out, counts, touches = T.move(rec, nbox, m, words=words, mask=2)
    assert counts[0] >= 1 and (touches[0]["hit"]["tag"][:counts[0]] == 101).all() and out["position"][0][1] < 0.5
    out, counts, touches = T.move(rec, nbox, m, words=words, mask=0)
    assert counts[0] == 0 and out["flags"][0] == 0


def test_a_free_move_lists_nothing_and_a_start_overlap_lists_one():
    rec, nbox = world(boxes=[FLOOR])
    T = HT.CAPSULE
    m = T.mover.moves([(0.0, 5.0, 0.0), (0.0, 0.5, 0.0)], [(1.0, 1.0, 0.0), (1.0, 0.0, 0.0)], R, HH, skin=SKIN)
    out, counts, touches = T.move(rec, nbox, m, touches=sentinel(2, HT.MOVE_K))
    assert counts.tolist() == [0, 1] and out["flags"].tolist() == [0, E.NH_MOVE_START_OVERLAP]
    assert touches[1]["hit"]["t"][0] == 0 and touches[1]["hit"]["tag"][0] == 100 and touches[1]["cast"][0] == 0
    assert touches[1]["hit"][0].tobytes() == out["last_hit"][1].tobytes()
    assert unwritten_keep_the_sentinel(counts, touches)


def test_a_walk_up_a_riser_and_a_walk_on_flat_ground():
    rec, nbox = terrain()
    T = HT.CAPSULE
    w = T.mover.walks(WB.stand([1.0, 1.0], 0.0, [WB.LANE["riser"], WB.LANE["open"]], WR, WHH), (2.0, 0.0, 0.0), WR, WHH, skin=WB.SKIN, step_height=1.0, snap_distance=0.3)
    out, counts, touches = T.walk(rec, nbox, w, touches=sentinel(2, HT.WALK_K))
    # the riser (collider 6): A is blocked by its face, U and F are free, D lands on its top
    assert (int(out["flags"][0]) & E.NH_WALK_STEPPED) != 0 and out["casts"][0] == 4 and counts[0] == 2
    t = touches[0]
    assert t["phase"][:2].tolist() == [E.NH_TOUCH_SLIDE, E.NH_TOUCH_DOWN] and t["cast"][:2].tolist() == [0, 3] and t["hit"]["collider"][:2].tolist() == [6, 6]
    assert t["hit"]["normal"][0].tolist() == [-1.0, 0.0, 0.0] and abs(t["hit"]["normal"][1][1] - 1.0) <= TOL
    assert t["hit"][1].tobytes() == out["ground"][0].tobytes()
    # flat ground: A is free, the probe finds the floor (collider 0)
    assert (int(out["flags"][1]) & (E.NH_WALK_STEPPED | E.NH_WALK_GROUNDED)) == E.NH_WALK_GROUNDED and counts[1] == 1 and out["casts"][1] == 2
    t = touches[1]
    assert t["phase"][0] == E.NH_TOUCH_PROBE and t["cast"][0] == 1 and t["hit"]["collider"][0] == 0 and t["hit"][0].tobytes() == out["ground"][1].tobytes()
    assert t["direction"][0].tolist() == [0.0, np.float32(-0.3), 0.0]
    assert unwritten_keep_the_sentinel(counts, touches)
    HT.check_walk_identities(out, counts, touches, "hand-built walks")
    # a mask that hides the floor (layer 1; everything else layer 2): the probe finds nothing; ignore_body 0 hides the whole static terrain
    words = np.full(len(rec), 2, dtype=np.uint32)
    words[0] = 1
    out, counts, touches = T.walk(rec, nbox, w, words=words, mask=2)
    assert counts[1] == 0 and out["ground"][1]["shape"] == NONE and counts[0] >= 1 and (touches[0]["hit"]["collider"][:counts[0]] != 0).all()
    w["ignore_body"] = 0
    assert (T.walk(rec, nbox, w)[1] == 0).all()


# ---- the batches of the GPU tests --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_batch_conditions(shape):
    """What keeps the GPU's bit-for-bit tests from passing vacuously, on the same generators and seeds.  Moves: counts >= slides, so the bars of
    move_batches.shares hold for the touches.  Walks: a stepped walk touched under SLIDE (what blocked it), under DOWN (what it landed on) and under a
    third phase or not -- so the share asked for is that of records with three phases, at TERRAIN_SHARES' stepped bar; and a GROUNDED walk that did not
    step was grounded by a probe that hit, so PROBE touches occur in at least the grounded bar minus the batch's stepped share."""
    T = TB.SHAPES[shape]
    for name in sorted(SMALL):
        scene = SMALL[name]()
        rec, nbox = Q.records(scene["body_transforms"], scene), len(scene["box_tags"])
        _, counts, _ = T.move(rec, nbox, TB.world_moves(shape, name, rec, nbox))
        once, twice = float((counts >= 1).mean()), float((counts >= 2).mean())
        print("%s %s: touches >= 1 %.3f, >= 2 %.3f, mean %.3f" % (shape, name, once, twice, counts.mean()))
        assert once >= 0.25 and twice >= 0.02, (shape, name, once, twice)
    _, _, _, out, counts, touches = terrain_run(shape)
    three = float((TB.phases(counts, touches) >= 3).mean())
    stepped = float(((out["flags"] & E.NH_WALK_STEPPED) != 0).mean())
    probe = float(((touches["phase"] == E.NH_TOUCH_PROBE) & HT.written(counts, HT.WALK_K)).any(axis=1).mean())
    print("%s terrain: three phases %.3f, stepped %.3f, a PROBE touch %.3f, touches per walk %.3f" % (shape, three, stepped, probe, counts.mean()))
    assert three >= TERRAIN_SHARES["stepped"], (shape, three)
    assert probe >= TERRAIN_SHARES["grounded"] - stepped, (shape, probe, stepped)
