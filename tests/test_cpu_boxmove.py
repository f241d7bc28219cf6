"""nh_boxmove's state machine on the CPU (include/nudge_hip.h, "nh_boxmove"; nudge_amd/csrc/nh_query.h, "move"): the host oracle of
tests/hostoracle/hostmover.cpp -- the NH_HD functions the kernel runs, around a brute-force box cast -- against the replay round by round
(hostcast.cpp's box cast, the capsule mover's begin / advance), on hand-built worlds, on every invalid-record rule, on the identities,
on the conditions that keep the GPU tests' batches honest, and on THE INVARIANT of test_cpu_move's random world: a box move that starts free ends no
deeper than its skin in anything."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boxmove_batches as BMB               # noqa: E402
import hostcast_util as CAST                 # noqa: E402
import hostlib as H                         # noqa: E402
import hostoverlap_util as HO               # noqa: E402
import hostpen_util as HP                   # noqa: E402
import hostquery_util as Q                  # noqa: E402
from hostmover_util import BOX as HBM, CAPSULE as HM      # noqa: E402
from mover_util import NONE, miss           # noqa: E402
from query_util import SMALL                # noqa: E402
from test_cpu_move import FLOOR, QNAN, TOL, _random_world_and_moves, world      # noqa: E402
from nudge_amd import engine as E          # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HALF, SKIN = (0.3, 0.5, 0.4), 0.01          # the box of the invariant and of the hand-built worlds
# candidates drawn per move kept (boxmove_batches.moves): the ball pit is packed, 6 % of its candidates start free
DRAW = dict(ball_pit=16)
BATCH_SEED = 900


def header():
    return open(os.path.join(ROOT, "include", "nudge_hip.h")).read()


def overlapping(rec, nbox, m):
    """Per move: how many colliders the box at its origin overlaps (nh_overlap's NH_SHAPE_BOX predicates)."""
    return np.diff(HO.overlap(rec, nbox, HBM.overlap_queries(m))[0].astype(np.int64))


def deepest(rec, nbox, centres, rotations, sizes):
    """Per box: the depth of its deepest penetration (nh_penetration's NH_SHAPE_BOX queries by brute force), 0 where it touches nothing."""
    q = np.zeros(len(centres), dtype=E.OVERLAP_QUERY)
    q["center"], q["shape"], q["rotation"], q["size"], q["ignore_body"] = centres, E.NH_SHAPE_BOX, rotations, sizes, NONE
    off, hits, total = HP.penetration(rec, nbox, q)
    depth = np.zeros(len(q))
    if total:
        np.maximum.at(depth, np.repeat(np.arange(len(q)), np.diff(off.astype(np.int64))), hits["depth"][:total].astype(np.float64))
    return depth


# ---- declarations ---------------------------------------------------------------------------------------------------------------------------------
def test_records_are_the_headers():
    assert E.BOX_MOVE.itemsize == 64 and E.BOX_WALK.itemsize == 96
    assert [E.BOX_MOVE.fields[k][1] for k in ("origin", "skin", "displacement", "ignore_body", "rotation", "size", "max_slides")] == [0, 12, 16, 28, 32, 48, 60]
    assert [E.BOX_MOVE.fields[k][1] for k in ("origin", "skin", "displacement", "ignore_body", "rotation", "size", "max_slides")] == \
           [E.BOX_CAST.fields[k][1] for k in ("origin", "max_t", "direction", "ignore_body", "rotation", "size", "reserved")]
    text = header()
    assert ("typedef struct nh_BoxMove { float origin[3]; float skin; float displacement[3]; uint32_t ignore_body;\n"
            "                            float rotation[4]; float size[3]; uint32_t max_slides; } nh_BoxMove;") in text
    assert "int nh_boxmove(nh_context* ctx, const nh_BoxMove* moves, uint32_t count, nh_MoveResult* results, uint32_t flags /* 0 */);" in text
    assert "int nh_boxwalk(nh_context* ctx, const nh_BoxWalk* walks, uint32_t count, nh_WalkResult* results, uint32_t flags /* 0 */);" in text
    assert "nh_boxmove" in E.EXPORTS and "nh_boxwalk" in E.EXPORTS
    for name in ("boxmove", "boxmove_records", "boxwalk", "boxwalk_records"):
        assert callable(getattr(E.World, name))


def test_the_library_exports_both_symbols():
    so = os.path.join(ROOT, "nudge_amd", "libnudge_hip.so")
    names = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.split()
    assert "nh_boxmove" in names and "nh_boxwalk" in names


def test_the_header_lists_the_new_observers_and_no_box_movers_as_not_built():
    text = header()
    note = next(line for line in text.splitlines() if "The scene queries (nh_query_build" in line)
    for name in ("nh_walk", "nh_boxmove", "nh_boxwalk"):
        assert re.search(r"\b%s\b" % name, note), name
    for block in re.findall(r"(?is)not built:.*?(?:\*/|\n\s*\n|Cost:)", text):
        assert "box mover" not in block.lower(), block[:200]
    assert "twenty-five query calls" in text and "twenty-three" not in text


# ---- the new oracle against the replay through the old ones -----------------------------------------------------------------------------------------
def _replay_old(rec, nbox, m):
    """hostcast.cpp's box cast per round, the capsule mover's nh_q_move_advance between rounds, on the capsule records of the same moves."""
    cm = np.zeros(len(m), dtype=E.MOVE)
    for name in ("origin", "skin", "displacement", "ignore_body", "rotation", "max_slides"):
        cm[name] = m[name]
    st = HM.begin(cm)
    last = np.tile(miss(), len(m))
    rounds = 0
    while (st["stopped"] == 0).any():
        assert rounds <= E.NH_MOVE_MAX_SLIDES
        live = st["stopped"] == 0
        hits = CAST.cast(CAST.BOX, rec, nbox, HBM.state_casts(m, st))
        last[live] = hits[live]
        HM.advance(cm, st, hits)
        rounds += 1
    out = np.zeros(len(m), dtype=E.MOVE_RESULT)
    out["position"], out["remaining"], out["flags"], out["slides"], out["last_hit"] = st["p"], st["v"], st["flags"], st["slides"], last
    return out


def _random_box_moves(seed, n):
    rec, nbox, cm = _random_world_and_moves(seed=seed, n_moves=n)
    m = HBM.moves(cm["origin"], cm["displacement"], HALF, rotations=cm["rotation"], skin=SKIN, max_slides=cm["max_slides"])
    return rec, nbox, m


def test_the_oracle_equals_the_replay_through_the_old_oracles():
    rec, nbox, m = _random_box_moves(31, 2048)
    m["size"][::7] = 0.0                                                   # rays among them
    m["size"][3::11, 1] = 0.0                                              # and plates
    ref = _replay_old(rec, nbox, m)
    out = HBM.move(rec, nbox, m)
    bad = (out.view(np.uint8).reshape(-1, 64) != ref.view(np.uint8).reshape(-1, 64)).any(axis=1)
    assert not bad.any(), (int(bad.sum()), out[np.argmax(bad)], ref[np.argmax(bad)])
    assert (out["slides"] >= 1).mean() >= 0.15 and (out["slides"] >= 2).mean() >= 0.02
    # ... and the box mover's begin / advance are the capsule mover's
    got, rounds = HBM.replay_move(m, lambda c: CAST.cast(CAST.BOX, rec, nbox, c))
    assert got.tobytes() == out.tobytes() and rounds >= 3


# ---- hand-built worlds ------------------------------------------------------------------------------------------------------------------------------
def test_free_space_floor_and_wall():
    rec, nbox = world(boxes=[FLOOR, ((3.0, 6.0, 0.0), (1.0, 5.0, 5.0))])   # the floor's top at y = 0; a wall whose face is x = 2, from y = 1 up
    hx, hy, hz = HALF
    # free: the whole displacement, one cast, a miss
    out, made = HBM.move(rec, nbox, HBM.moves([(0.0, 20.0, 0.0)], [(1.0, -1.0, 0.5)], HALF, skin=SKIN), casts=True)
    assert out[0]["flags"] == 0 and made[0] == 1 and (out[0]["remaining"] == 0).all() and out[0]["last_hit"].tobytes() == miss().tobytes()
    assert out[0]["position"].tobytes() == np.float32([1.0, 19.0, 0.5]).tobytes()
    assert HBM.move(rec[:0], 0, HBM.moves([(0.0, 20.0, 0.0)], [(1.0, -1.0, 0.5)], HALF, skin=SKIN)).tobytes() == out.tobytes()
    # onto the floor and along it: the bottom face lands at t = 0.2, one skin above the floor
    m = HBM.moves([(-5.0, hy + 0.2, 0.0)], [(1.0, -1.0, 0.0)], HALF, skin=SKIN)
    o, made = HBM.move(rec, nbox, m, casts=True)
    o = o[0]
    assert abs(o["position"][1] - (hy + SKIN)) <= TOL and abs(o["position"][0] + 4.0) <= TOL and o["slides"] == 1 and o["flags"] == E.NH_MOVE_HIT and made[0] == 2
    m["max_slides"] = 0
    first = HBM.move(rec, nbox, m)[0]
    assert first["last_hit"]["normal"].tolist() == [0.0, 1.0, 0.0] and abs(first["last_hit"]["t"] - 0.2) <= TOL and first["last_hit"]["tag"] == 100
    assert first["flags"] == E.NH_MOVE_HIT | E.NH_MOVE_SLIDES_OUT and np.abs(first["remaining"] - np.float32([0.8, 0.0, 0.0])).max() <= TOL
    # identity 1 on the oracle: with max_slides = 0, last_hit is the box cast's record
    assert first["last_hit"].tobytes() == CAST.cast(CAST.BOX, rec, nbox, HBM.first_casts(m))[0].tobytes()
    # head-on into the wall: stops one skin in front of it, WEDGED through the d0 rule
    for max_slides in (0, 4):
        o, made = HBM.move(rec, nbox, HBM.moves([(0.0, 3.0, 0.0)], [(3.0, 0.0, 0.0)], HALF, skin=SKIN, max_slides=max_slides), casts=True)
        o = o[0]
        assert abs(o["position"][0] - (2.0 - hx - SKIN)) <= TOL and o["position"][1] == 3.0 and o["flags"] == E.NH_MOVE_HIT | E.NH_MOVE_WEDGED and made[0] == 1
        assert o["last_hit"]["normal"].tolist() == [-1.0, 0.0, 0.0]
    # a box turned 45 degrees about y meets the wall with its edge: half diagonal of the (hx, hz) rectangle along x
    a = np.pi / 4
    o = HBM.move(rec, nbox, HBM.moves([(0.0, 3.0, 0.0)], [(3.0, 0.0, 0.0)], (0.3, 0.5, 0.3), rotations=[(0.0, np.sin(a / 2), 0.0, np.cos(a / 2))], skin=SKIN))[0]
    assert abs(o["position"][0] - (2.0 - 0.3 * np.sqrt(2.0) - SKIN)) <= TOL
    # start in overlap: nothing but the flag
    m = HBM.moves([(0.0, hy - 0.1, 0.0)], [(1.0, -1.0, 0.0)], HALF, skin=SKIN)
    o, made = HBM.move(rec, nbox, m, casts=True)
    assert o[0]["flags"] == E.NH_MOVE_START_OVERLAP and made[0] == 1 and o[0]["last_hit"]["t"] == 0
    assert o[0]["position"].tobytes() == m["origin"][0].tobytes() and o[0]["remaining"].tobytes() == m["displacement"][0].tobytes()


def test_concave_corner():
    walls = [FLOOR, ((3.0, 2.0, 0.0), (1.0, 5.0, 8.0)), ((0.0, 2.0, 3.0), (8.0, 5.0, 1.0))]      # faces at x = 2 and z = 2
    rec, nbox = world(boxes=walls)
    hx, hy, hz = HALF
    for d in ((3.0, -0.5, 3.2), (3.0, 0.0, 3.25), (2.5, 0.0, 4.0), (3.5, -1.0, 3.0)):
        m = HBM.moves([(0.0, hy + 0.2, 0.0)], [d], HALF, skin=SKIN, max_slides=8)
        o = HBM.move(rec, nbox, m)[0]
        assert abs(o["position"][0] - (2.0 - hx - SKIN)) <= TOL and abs(o["position"][2] - (2.0 - hz - SKIN)) <= TOL, (d, o)
        m["origin"] = o["position"]
        assert overlapping(rec, nbox, m)[0] == 0
        assert 2 <= o["slides"] <= 3 and o["flags"] & E.NH_MOVE_HIT and not o["flags"] & E.NH_MOVE_SLIDES_OUT, (d, o)


# ---- invalid records, valid edges -------------------------------------------------------------------------------------------------------------------
def _invalid_cases():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    cases = []
    for field, k in (("origin", 0), ("origin", 2), ("displacement", 1)):
        for bad in (nan, inf, -inf):
            cases.append((field, k, bad))
    for k in range(3):
        for bad in (nan, inf, np.float32(-0.25)):
            cases.append(("size", k, bad))
    for bad in (nan, inf, np.float32(-0.25)):
        cases.append(("skin", None, bad))
    for k in range(4):
        cases.append(("rotation", k, nan))
    cases.append(("rotation", 3, inf))
    cases.append(("max_slides", None, 9))
    cases.append(("max_slides", None, 0xFFFFFFFF))
    return cases


def test_invalid_records():
    rec, nbox = world(boxes=[FLOOR])
    cases = _invalid_cases()
    m = HBM.moves(np.tile(np.float32([0.0, 1.2, 0.0]), (len(cases), 1)), np.tile(np.float32([1.0, -1.0, 0.0]), (len(cases), 1)), HALF, skin=SKIN)
    for i, (field, k, bad) in enumerate(cases):
        if k is None:
            m[field][i] = bad
        else:
            m[field][i, k] = bad
    out, made = HBM.move(rec, nbox, m, casts=True)
    assert (out["flags"] == E.NH_MOVE_INVALID).all() and (out["slides"] == 0).all() and (made == 0).all()
    assert out["position"].tobytes() == m["origin"].tobytes() and out["remaining"].tobytes() == m["displacement"].tobytes()
    nan_miss = miss()
    nan_miss["t"] = np.uint32(QNAN).view(np.float32)
    assert all(h.tobytes() == nan_miss.tobytes() for h in out["last_hit"])


def test_valid_edges():
    rec, nbox = world(boxes=[FLOOR])
    o, d = [(0.0, 1.2, 0.0)], [(1.0, -1.0, 0.0)]
    for max_slides in (0, 8):
        good = HBM.move(rec, nbox, HBM.moves(o, d, HALF, skin=SKIN, max_slides=max_slides))[0]
        assert good["flags"] & E.NH_MOVE_INVALID == 0 and good["flags"] & E.NH_MOVE_HIT and good["slides"] == 1
    # one half extent 0 is a plate, still a box: it reads its rotation
    for k in range(3):
        size = list(HALF)
        size[k] = 0.0
        m = HBM.moves(o, [(1.0, -2.0, 0.0)], size, skin=SKIN)
        assert HBM.move(rec, nbox, m)[0]["flags"] == E.NH_MOVE_HIT
        m["rotation"][0, 1] = np.nan
        assert HBM.move(rec, nbox, m)[0]["flags"] == E.NH_MOVE_INVALID
    # size (0, 0, 0) is a ray and does not read the rotation
    m = HBM.moves(o, [(1.0, -2.0, 0.0)], (0.0, 0.0, 0.0), skin=SKIN)
    ray = HBM.move(rec, nbox, m)
    m["rotation"] = np.nan
    assert HBM.move(rec, nbox, m).tobytes() == ray.tobytes() and ray["flags"][0] == E.NH_MOVE_HIT
    # displacement = 0 (either sign) is a valid no-op that makes no cast, in overlap or not
    m = HBM.moves([(0.0, 1.2, 0.0), (0.0, 0.2, 0.0)], [(0.0, 0.0, 0.0), (-0.0, 0.0, -0.0)], HALF, skin=SKIN)
    out, made = HBM.move(rec, nbox, m, casts=True)
    assert (made == 0).all() and (out["flags"] == 0).all() and out["position"].tobytes() == m["origin"].tobytes()
    assert all(h.tobytes() == miss().tobytes() for h in out["last_hit"])
    # skin = 0 leaves the box touching: the next cast is a START OVERLAP, with max_slides = 0 there is none
    out = HBM.move(rec, nbox, HBM.moves(o * 2, d * 2, HALF, skin=0.0, max_slides=[0, 4]))
    assert out["flags"][0] == E.NH_MOVE_HIT | E.NH_MOVE_SLIDES_OUT and out["flags"][1] == E.NH_MOVE_HIT | E.NH_MOVE_START_OVERLAP
    # ignore_body: the floor's body ignored, the move goes through
    assert HBM.move(rec, nbox, HBM.moves(o, d, HALF, skin=SKIN, ignore_body=0))[0]["flags"] == 0


def test_size_zero_is_nh_move_with_radius_and_half_height_zero():
    """Identity 2: both are ray casts; the 64 result bytes are equal, whatever the rotation holds."""
    rec, nbox, cm = _random_world_and_moves(seed=33, n_moves=4096)
    cm["radius"], cm["half_height"] = 0.0, 0.0
    m = HBM.moves(cm["origin"], cm["displacement"], (0.0, 0.0, 0.0), rotations=np.full((len(cm), 4), np.nan), skin=SKIN, max_slides=cm["max_slides"])
    out, ref = HBM.move(rec, nbox, m), HM.move(rec, nbox, cm)
    assert out.tobytes() == ref.tobytes()
    assert (out["flags"] & E.NH_MOVE_INVALID == 0).all() and (out["slides"] >= 1).mean() >= 0.1


# ---- the batches of the GPU tests ------------------------------------------------------------------------------------------------------------------
def test_batch_conditions():
    """What keeps the bit-for-bit tests honest: on every world of SMALL the batch of tests/test_gpu_boxmove.py (the same generator, the same seed)
    slides once in a quarter of its moves and twice in 2 %."""
    for name in sorted(SMALL):
        scene = SMALL[name]()
        rec, nbox = Q.records(scene["body_transforms"], scene), len(scene["box_tags"])
        m = BMB.moves(np.random.default_rng(BATCH_SEED + sorted(SMALL).index(name)), rec, nbox, 4096, draw=DRAW.get(name, 4))
        out = HBM.move(rec, nbox, m)
        once, twice = BMB.shares(out)
        print("%s: slides >= 1 %.3f, >= 2 %.3f, start free %.3f" % (name, once, twice, (overlapping(rec, nbox, m) == 0).mean()))
        assert once >= 0.25 and twice >= 0.02, (name, once, twice)
        assert (out["flags"] & E.NH_MOVE_INVALID == 0).all()


# ---- THE INVARIANT --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_run():
    rec, nbox, m = _random_box_moves(20, 20000)
    out = HBM.move(rec, nbox, m)
    free = overlapping(rec, nbox, m) == 0
    return rec, nbox, m, out, free


def test_invariant_conditions(random_run):
    """What keeps the invariant honest: enough moves start free, and enough of those slide once and twice."""
    _, _, m, out, free = random_run
    s = out["slides"][free]
    print("free %.3f, of them slides >= 1 %.3f, >= 2 %.3f, >= 3 %.3f" % (free.mean(), (s >= 1).mean(), (s >= 2).mean(), (s >= 3).mean()))
    assert free.mean() >= 0.5
    assert (s >= 1).mean() >= 0.25
    assert (s >= 2).mean() >= 0.03
    assert (out["flags"] & E.NH_MOVE_INVALID == 0).all()


def test_invariant(random_run):
    """A box move that starts free ends at most skin + 2^-16 C deep in anything: test_cpu_move's bound with the box's half diagonal in place of R + HH
    (C: the largest coordinate plus extent of the scene).  Its derivation does not look at the shape: the push skin * n can enter a neighbour by at most
    skin; the reach rule delays a hit by at most the leaf pad plus the cast pad, 2 * 2^-18 of the coordinates; four times that is the 2^-16.  And it
    ends neither behind its origin (but for the skin pushes) nor farther than it was asked to go."""
    rec, nbox, m, out, free = random_run
    diag = float(np.linalg.norm(HALF))
    C = float(max(np.abs(rec["p"]).max() + np.sqrt(3.0) * rec["h"].max(), np.abs(m["origin"]).max() + np.abs(m["displacement"]).max() + diag))
    tol = 2.0 ** -16 * C
    depth = deepest(rec, nbox, out["position"], m["rotation"], m["size"])
    print("deepest end of a free box move: %.6f (bound %.6f); ends touching something: %d of %d" % (depth[free].max(), SKIN + tol, (depth[free] > 0).sum(), free.sum()))
    assert (depth[free] <= SKIN + tol).all()
    d0 = m["displacement"].astype(np.float64)
    L = np.linalg.norm(d0, axis=1)
    gone = out["position"].astype(np.float64) - m["origin"].astype(np.float64)
    slack = out["slides"] * SKIN + tol
    assert ((gone * d0).sum(axis=1)[free] / L[free] >= -slack[free]).all()
    assert (np.linalg.norm(gone, axis=1)[free] <= (L + slack)[free]).all()
