"""nh_move's state machine on the CPU (include/nudge_hip.h, "nh_move"; nudge_amd/csrc/nh_query.h, "move"): the host oracle of tests/hostoracle/hostmover.cpp --
the same NH_HD functions the kernel runs, around a brute-force capsule cast -- on hand-built worlds whose answers are known, on every invalid-record rule,
and on THE INVARIANT of a random world: a move that starts free ends no deeper than its skin in anything, never behind where it started and never
farther than it was asked to go."""
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
from hostmover_util import CAPSULE as HM    # noqa: E402
from mover_util import NONE, miss           # noqa: E402
from query_util import unit_quats as _unit_quats      # noqa: E402
from nudge_amd import engine as E          # noqa: E402

R, HH, SKIN = 0.5, 0.5, 0.01                # the upright capsule of the hand-built worlds
TOL = 2.0 ** -16 * 64                       # every coordinate of those worlds stays below 64
QNAN = 0x7FC00000


def world(boxes=(), spheres=()):
    """(rec, nbox) of a static world: boxes as (centre, half extents[, rotation]), spheres as (centre, radius); every collider belongs to body 0."""
    rec = np.zeros(len(boxes) + len(spheres), dtype=H.REC)
    rec["q"] = MV.IDENTITY
    for i, b in enumerate(boxes):
        rec["p"][i], rec["h"][i] = b[0], b[1]
        if len(b) > 2:
            rec["q"][i] = b[2]
    for j, (c, rad) in enumerate(spheres):
        rec["p"][len(boxes) + j], rec["h"][len(boxes) + j] = c, (rad, rad, rad)
    rec["tag"] = np.arange(len(rec)) + 100
    return rec, len(boxes)


def overlapping(rec, nbox, centres, rot=MV.IDENTITY, r=R, hh=HH):
    """Per capsule at `centres`: how many colliders it overlaps (hc_overlap, the capsule predicates of nh_overlap)."""
    q = np.zeros(len(centres), dtype=E.OVERLAP_QUERY)
    q["center"], q["shape"], q["rotation"], q["ignore_body"] = centres, E.NH_SHAPE_CAPSULE, rot, NONE
    q["size"][:, 0], q["size"][:, 1] = r, hh
    off, _, _ = HC.overlap(rec, nbox, q)
    return np.diff(off.astype(np.int64))


FLOOR = ((0.0, -1.0, 0.0), (30.0, 1.0, 30.0))                # top face at y = 0


def test_records_are_the_headers():
    assert E.MOVE.itemsize == 64 and E.MOVE_RESULT.itemsize == 64 and E.MOVE_RESULT.fields["last_hit"][1] == 32
    assert [E.MOVE.fields[k][1] for k in ("origin", "skin", "displacement", "ignore_body", "rotation", "radius", "half_height", "max_slides")] == \
           [E.CAPSULE_CAST.fields[k][1] for k in ("origin", "max_t", "direction", "ignore_body", "rotation", "radius", "half_height", "reserved")]
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "nudge_hip.h")).read()
    assert "#define NH_MOVE_MAX_SLIDES 8u" in text
    assert "NH_MOVE_HIT = 1u, NH_MOVE_START_OVERLAP = 2u, NH_MOVE_SLIDES_OUT = 4u, NH_MOVE_WEDGED = 8u, NH_MOVE_INVALID = 0x80000000u" in text
    assert (E.NH_MOVE_HIT, E.NH_MOVE_START_OVERLAP, E.NH_MOVE_SLIDES_OUT, E.NH_MOVE_WEDGED, E.NH_MOVE_INVALID, E.NH_MOVE_MAX_SLIDES) == (1, 2, 4, 8, 0x80000000, 8)
    assert "nh_move" in E.EXPORTS


def test_free_space():
    rec, nbox = world(boxes=[FLOOR])
    rng = np.random.default_rng(1)
    o = rng.uniform(-20, 20, size=(64, 3)).astype(np.float32)
    o[:, 1] = rng.uniform(5, 20, size=64)
    d = rng.uniform(-2, 2, size=(64, 3)).astype(np.float32)
    m = HM.moves(o, d, R, HH, skin=SKIN)
    out, made = HM.move(rec, nbox, m, casts=True)
    assert out["position"].tobytes() == (o + d).tobytes()
    assert (out["flags"] == 0).all() and (out["slides"] == 0).all() and (made == 1).all()
    assert out["remaining"].tobytes() == np.zeros((64, 3), dtype=np.float32).tobytes()
    assert all(h.tobytes() == miss().tobytes() for h in out["last_hit"])
    # an empty world: the same
    assert HM.move(rec[:0], 0, m).tobytes() == out.tobytes()


def test_floor():
    rec, nbox = world(boxes=[FLOOR])
    m = HM.moves([(0.0, 1.2, 0.0)], [(1.0, -1.0, 0.0)], R, HH, skin=SKIN)
    out, made = HM.move(rec, nbox, m, casts=True)
    o = out[0]
    assert abs(o["position"][1] - (1.0 + SKIN)) <= TOL and abs(o["position"][0] - 1.0) <= TOL and o["position"][2] == 0.0
    assert o["slides"] == 1 and o["flags"] == E.NH_MOVE_HIT and made[0] == 2
    assert (o["remaining"] == 0).all()
    assert o["last_hit"].tobytes() == miss().tobytes()
    # the normal the first cast took: max_slides = 0 stops behind it
    m["max_slides"] = 0
    first = HM.move(rec, nbox, m)[0]
    assert first["last_hit"]["normal"].tolist() == [0.0, 1.0, 0.0] and abs(first["last_hit"]["t"] - 0.2) <= TOL
    assert first["last_hit"]["shape"] == E.NH_SHAPE_BOX and first["last_hit"]["tag"] == 100
    assert first["flags"] == E.NH_MOVE_HIT | E.NH_MOVE_SLIDES_OUT and first["slides"] == 1
    assert np.abs(first["remaining"] - np.float32([0.8, 0.0, 0.0])).max() <= TOL and abs(first["position"][1] - (1.0 + SKIN)) <= TOL
    assert first["last_hit"].tobytes() == CAST.cast(CAST.CAPSULE, rec, nbox, HM.first_casts(m))[0].tobytes()


def test_wall_head_on():
    rec, nbox = world(boxes=[((3.0, 0.0, 0.0), (1.0, 5.0, 5.0))])            # its face at x = 2: touching at x = 1.5
    for max_slides in (0, 4):
        out, made = HM.move(rec, nbox, HM.moves([(0.0, 0.0, 0.0)], [(3.0, 0.0, 0.0)], R, HH, skin=SKIN, max_slides=max_slides), casts=True)
        o = out[0]
        assert abs(o["position"][0] - (1.5 - SKIN)) <= TOL and o["position"][1] == 0.0 and o["position"][2] == 0.0
        assert (o["remaining"] == 0).all() and o["slides"] == 1 and made[0] == 1
        # a head-on hit leaves nothing of the displacement: the rule "never against d0" zeroes it, and that sets WEDGED (nh_query.h)
        assert o["flags"] == E.NH_MOVE_HIT | E.NH_MOVE_WEDGED
        assert o["last_hit"]["normal"].tolist() == [-1.0, 0.0, 0.0]


def test_concave_corner():
    walls = [FLOOR, ((3.0, 2.0, 0.0), (1.0, 5.0, 8.0)), ((0.0, 2.0, 3.0), (8.0, 5.0, 1.0))]      # faces at x = 2 and z = 2
    rec, nbox = world(boxes=walls)
    for d in ((3.0, -0.5, 3.2), (3.0, 0.0, 3.25), (2.5, 0.0, 4.0), (3.5, -1.0, 3.0)):
        o = HM.move(rec, nbox, HM.moves([(0.0, 1.2, 0.0)], [d], R, HH, skin=SKIN, max_slides=8))[0]
        assert abs(o["position"][0] - (1.5 - SKIN)) <= TOL and abs(o["position"][2] - (1.5 - SKIN)) <= TOL, (d, o)
        assert overlapping(rec, nbox, o["position"][None])[0] == 0
        assert 2 <= o["slides"] <= 3 and o["flags"] & E.NH_MOVE_HIT and not o["flags"] & E.NH_MOVE_SLIDES_OUT, (d, o)
    # the exact diagonal meets both walls at the same t: the tie goes to the lower index, the skin push is along that wall's normal alone, and the capsule
    # is left TOUCHING the other wall -- the next cast starts in contact and rule 4 ends the move there, inside the corner all the same
    o = HM.move(rec, nbox, HM.moves([(0.0, 1.2, 0.0)], [(3.0, 0.0, 3.0)], R, HH, skin=SKIN, max_slides=8))[0]
    assert o["flags"] == E.NH_MOVE_HIT | E.NH_MOVE_START_OVERLAP and o["slides"] == 1
    assert abs(o["position"][0] - (1.5 - SKIN)) <= TOL and 1.5 - SKIN - TOL <= o["position"][2] <= 1.5 + TOL


def test_acute_corner():
    # the wedge 0 < z < x: wall A fills z < 0, wall B fills z > x (its face through the origin, 45 degrees from A's); the capsule fits down to where the
    # wedge is 2r wide
    th = np.deg2rad(225.0)
    qb = (0.0, np.sin(th / 2), 0.0, np.cos(th / 2))
    s = np.sqrt(0.5)
    rec, nbox = world(boxes=[((0.0, 0.0, -1.0), (40.0, 5.0, 1.0)), ((-s, 0.0, s), (1.0, 5.0, 40.0), qb)])
    rng = np.random.default_rng(5)
    n = 64
    o = np.zeros((n, 3), dtype=np.float32)
    o[:, 0] = rng.uniform(6, 10, size=n)
    o[:, 2] = rng.uniform(1.0, 2.5, size=n)
    aim = np.float32([1.3 * np.cos(np.pi / 8), 0.0, 1.3 * np.sin(np.pi / 8)]) * rng.uniform(-1.0, 0.9, size=(n, 1)).astype(np.float32)      # at or behind the apex
    d = (aim - o) * rng.uniform(1.0, 1.5, size=(n, 1)).astype(np.float32)
    assert (overlapping(rec, nbox, o) == 0).all()
    out = HM.move(rec, nbox, HM.moves(o, d, R, HH, skin=SKIN, max_slides=8))
    assert ((out["flags"] & (E.NH_MOVE_WEDGED | E.NH_MOVE_START_OVERLAP)) != 0).all(), out["flags"]
    p = out["position"].astype(np.float64)
    assert (p[:, 2] >= R - TOL).all() and ((p[:, 0] - p[:, 2]) * s >= R - TOL).all()


def test_ball_over_a_sphere():
    RS = 2.0
    rec, nbox = world(spheres=[((0.0, 0.0, 0.0), RS)])
    rng = np.random.default_rng(7)
    n = 256
    o = np.float32([-6.0, 0.0, 0.0]) + np.concatenate([np.zeros((n, 1)), rng.uniform(-2.4, 2.4, size=(n, 2))], axis=1).astype(np.float32)
    o[:8, 1:] = 0.0                                                          # head-on
    d = np.tile(np.float32([12.0, 0.0, 0.0]), (n, 1))
    slides = rng.integers(0, 9, size=n)
    out = HM.move(rec, nbox, HM.moves(o, d, R, 0.0, skin=SKIN, max_slides=slides))
    dist = np.linalg.norm(out["position"].astype(np.float64), axis=1)
    on_it = (out["last_hit"]["shape"] == E.NH_SHAPE_SPHERE) & ((out["flags"] & E.NH_MOVE_HIT) != 0)
    assert on_it.sum() >= 16 and (out["flags"][:8] == E.NH_MOVE_HIT | E.NH_MOVE_WEDGED).all()
    assert np.abs(dist[on_it] - (RS + R + SKIN)).max() <= TOL
    assert (dist >= RS + R + SKIN - TOL).all()                                # rolled over or past: never nearer than the skin
    went_on = (out["slides"] >= 1) & ~on_it
    assert went_on.sum() >= 16 and (out["position"][went_on, 0] > o[went_on, 0]).all()


def test_start_in_overlap():
    rec, nbox = world(boxes=[FLOOR])
    m = HM.moves([(0.0, 0.7, 0.0), (1.0, -0.5, 2.0)], [(1.0, -1.0, 0.0), (0.0, 3.0, 0.0)], R, HH, skin=SKIN)
    out, made = HM.move(rec, nbox, m, casts=True)
    assert (out["flags"] == E.NH_MOVE_START_OVERLAP).all() and (out["slides"] == 0).all() and (made == 1).all()
    assert out["position"].tobytes() == m["origin"].tobytes() and out["remaining"].tobytes() == m["displacement"].tobytes()
    assert (out["last_hit"]["t"] == 0).all() and (out["last_hit"]["shape"] == E.NH_SHAPE_BOX).all()


def _invalid_cases():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    cases = []
    for field, k in (("origin", 0), ("origin", 2), ("displacement", 1)):
        for bad in (nan, inf, -inf):
            cases.append((field, k, bad))
    for field in ("radius", "half_height", "skin"):
        for bad in (nan, inf, np.float32(-0.25)):
            cases.append((field, None, bad))
    for k in range(4):
        cases.append(("rotation", k, nan))
    cases.append(("rotation", 3, inf))
    cases.append(("max_slides", None, 9))
    cases.append(("max_slides", None, 0xFFFFFFFF))
    return cases


def test_invalid_records():
    rec, nbox = world(boxes=[FLOOR])
    cases = _invalid_cases()
    m = HM.moves(np.tile(np.float32([0.0, 1.2, 0.0]), (len(cases), 1)), np.tile(np.float32([1.0, -1.0, 0.0]), (len(cases), 1)), R, HH, skin=SKIN)
    for i, (field, k, bad) in enumerate(cases):
        if k is None:
            m[field][i] = bad
        else:
            m[field][i, k] = bad
    out, made = HM.move(rec, nbox, m, casts=True)
    assert (out["flags"] == E.NH_MOVE_INVALID).all() and (out["slides"] == 0).all() and (made == 0).all()
    assert out["position"].tobytes() == m["origin"].tobytes() and out["remaining"].tobytes() == m["displacement"].tobytes()
    nan_miss = miss()
    nan_miss["t"] = np.uint32(QNAN).view(np.float32)
    assert all(h.tobytes() == nan_miss.tobytes() for h in out["last_hit"])


def test_valid_edges():
    rec, nbox = world(boxes=[FLOOR])
    good = HM.move(rec, nbox, HM.moves([(0.0, 1.2, 0.0)], [(1.0, -1.0, 0.0)], R, HH, skin=SKIN, max_slides=8))[0]
    assert good["flags"] == E.NH_MOVE_HIT and good["slides"] == 1
    # `reserved` is not read, and neither is the rotation of a ball
    m = HM.moves([(0.0, 1.2, 0.0)], [(1.0, -1.0, 0.0)], R, 0.0, skin=SKIN)
    ball = HM.move(rec, nbox, m)
    m["reserved"], m["rotation"] = 0xDEADBEEF, np.nan
    assert HM.move(rec, nbox, m).tobytes() == ball.tobytes() and ball["flags"][0] == E.NH_MOVE_HIT
    # displacement = 0 (either sign) is a valid no-op that makes no cast, in overlap or not
    m = HM.moves([(0.0, 1.2, 0.0), (0.0, 0.2, 0.0)], [(0.0, 0.0, 0.0), (-0.0, 0.0, -0.0)], R, HH, skin=SKIN)
    out, made = HM.move(rec, nbox, m, casts=True)
    assert (made == 0).all() and (out["flags"] == 0).all() and (out["slides"] == 0).all()
    assert out["position"].tobytes() == m["origin"].tobytes() and out["remaining"].tobytes() == m["displacement"].tobytes()
    assert all(h.tobytes() == miss().tobytes() for h in out["last_hit"])
    # skin = 0 leaves the capsule touching: the next cast is a START OVERLAP, with max_slides = 0 there is none
    m = HM.moves([(0.0, 1.2, 0.0)] * 2, [(1.0, -1.0, 0.0)] * 2, R, HH, skin=0.0, max_slides=[0, 4])
    out = HM.move(rec, nbox, m)
    assert out["flags"][0] == E.NH_MOVE_HIT | E.NH_MOVE_SLIDES_OUT
    assert out["flags"][1] == E.NH_MOVE_HIT | E.NH_MOVE_START_OVERLAP and out["slides"][1] == 1
    # ignore_body: the floor's body ignored, the move goes through
    m = HM.moves([(0.0, 1.2, 0.0)], [(1.0, -1.0, 0.0)], R, HH, skin=SKIN, ignore_body=0)
    assert HM.move(rec, nbox, m)[0]["flags"] == 0


def test_advance_replays_the_oracle():
    """hm_begin / hm_advance (hostmover.cpp) around the brute-force capsule cast give hm_move's bytes: the loop of the REPLAY identity, on the CPU."""
    rec, nbox, m = _random_world_and_moves(seed=21, n_moves=512)
    ref = HM.move(rec, nbox, m)
    st = HM.begin(m)
    last = np.tile(miss(), len(m))
    for _ in range(E.NH_MOVE_MAX_SLIDES + 1):
        live = st["stopped"] == 0
        if not live.any():
            break
        hits = CAST.cast(CAST.CAPSULE, rec, nbox, HM.state_casts(m, st))
        last[live] = hits[live]
        HM.advance(m, st, hits)
    assert (st["stopped"] == 1).all()
    got = np.zeros(len(m), dtype=E.MOVE_RESULT)
    got["position"], got["remaining"], got["flags"], got["slides"], got["last_hit"] = st["p"], st["v"], st["flags"], st["slides"], last
    assert got.tobytes() == ref.tobytes()


# ---- THE INVARIANT --------------------------------------------------------------------------------------------------------------------------------
def _random_world_and_moves(seed, n_moves, n_boxes=2000, n_spheres=1000, side=40.0):
    """A static world of boxes and spheres of size 0.2 - 2 (half extents / radii 0.1 - 1) with random rotations inside a cube, and moves of the capsule
    (r, hh) = (0.5, 0.5) under random rotations from uniform origins by 0.5 - 4 units, max_slides drawn from 0 .. 8."""
    rng = np.random.default_rng(seed)
    rec = np.zeros(n_boxes + n_spheres, dtype=H.REC)
    rec["p"] = rng.uniform(-side / 2, side / 2, size=(len(rec), 3))
    rec["q"] = _unit_quats(rng, len(rec))
    rec["h"][:n_boxes] = rng.uniform(0.1, 1.0, size=(n_boxes, 3))
    rec["h"][n_boxes:] = rng.uniform(0.1, 1.0, size=(n_spheres, 1))
    rec["tag"] = rng.integers(0, 1 << 30, size=len(rec))
    o = rng.uniform(-side / 2, side / 2, size=(n_moves, 3)).astype(np.float32)
    d = rng.normal(size=(n_moves, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 4.0, size=(n_moves, 1))).astype(np.float32)
    m = HM.moves(o, d, R, HH, rotations=_unit_quats(rng, n_moves), skin=SKIN, max_slides=rng.integers(0, 9, size=n_moves))
    return rec, n_boxes, m


@pytest.fixture(scope="module")
def random_run():
    rec, nbox, m = _random_world_and_moves(seed=20, n_moves=20000)
    out = HM.move(rec, nbox, m)
    free = overlapping(rec, nbox, m["origin"], m["rotation"]) == 0
    return rec, nbox, m, out, free


def test_invariant_conditions(random_run):
    """What keeps the invariant honest: enough moves start free, and enough of those slide once and twice."""
    _, _, m, out, free = random_run
    s = out["slides"][free]
    print("free %.3f, of them slides >= 1 %.3f, >= 2 %.3f, >= 3 %.3f; flags: %s" % (
        free.mean(), (s >= 1).mean(), (s >= 2).mean(), (s >= 3).mean(),
        {name: int(((out["flags"][free] & bit) != 0).sum()) for name, bit in (("hit", 1), ("start", 2), ("out", 4), ("wedged", 8))}))
    assert free.mean() >= 0.5
    assert (s >= 1).mean() >= 0.25
    assert (s >= 2).mean() >= 0.03
    assert (out["flags"] & E.NH_MOVE_INVALID == 0).all()


def test_invariant(random_run):
    """A move that starts free ends at most skin + 2^-16 C deep in anything (C: the largest coordinate plus extent of the scene).  Derived, not measured:
    the push skin * n can enter a neighbour by at most skin; the reach rule delays a hit by at most the leaf pad plus the cast pad, 2 * 2^-18 of the
    coordinates; four times that is the 2^-16.  And it ends neither behind its origin (but for the skin pushes) nor farther than it was asked to go."""
    rec, nbox, m, out, free = random_run
    C = float(max(np.abs(rec["p"]).max() + np.sqrt(3.0) * rec["h"].max(), np.abs(m["origin"]).max() + np.abs(m["displacement"]).max() + R + HH))
    tol = 2.0 ** -16 * C
    q = np.zeros(len(m), dtype=E.OVERLAP_QUERY)
    q["center"], q["shape"], q["rotation"], q["ignore_body"] = out["position"], E.NH_SHAPE_CAPSULE, m["rotation"], NONE
    q["size"][:, 0], q["size"][:, 1] = R, HH
    off, hits, total = HP.penetration(rec, nbox, q)
    depth = np.zeros(len(m))
    if total:
        np.maximum.at(depth, np.repeat(np.arange(len(m)), np.diff(off.astype(np.int64))), hits["depth"][:total].astype(np.float64))
    print("deepest end of a free move: %.6f (bound %.6f); ends touching something: %d of %d" % (depth[free].max(), SKIN + tol, (depth[free] > 0).sum(), free.sum()))
    assert (depth[free] <= SKIN + tol).all()
    d0 = m["displacement"].astype(np.float64)
    L = np.linalg.norm(d0, axis=1)
    gone = out["position"].astype(np.float64) - m["origin"].astype(np.float64)
    slack = out["slides"] * SKIN + tol
    assert ((gone * d0).sum(axis=1)[free] / L[free] >= -slack[free]).all()
    assert (np.linalg.norm(gone, axis=1)[free] <= (L + slack)[free]).all()
