"""nh_recover's state machine on the CPU (include/nudge_hip.h, "nh_recover"; nudge_amd/csrc/nh_query.h, "recover"): the records against the header, the
host oracle of tests/hostoracle/hostrecover.cpp -- the same NH_HD functions the kernel runs, around a brute force over all colliders -- on hand-built worlds
whose answers are known and on every invalid-record rule, the header's identities against the penetration oracle, and the share conditions of the GPU
test's batches, which must hold for the reference alone before that test ever runs."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import hostlib as H                         # noqa: E402
import hostpen_util as HP                   # noqa: E402
import hostquery_util as Q                  # noqa: E402
import hostrecover_util as HR               # noqa: E402
import make_golden as G                     # noqa: E402
import recover_batches as RB                # noqa: E402
from query_util import SMALL                # noqa: E402
from nudge_amd import engine as E          # noqa: E402

NONE = 0xFFFFFFFF
SKIN = 0.01
ULP = 2.0 ** -23                            # of a coordinate of about 1: the hand-built sphere answers hold to a few of these
PEN_TOL = 7.5e-6                            # tests/test_cpu_penetration.py's TOL for the box and capsule pair functions, on pairs of scale 1
PUSHED, OVERLAPPING, TOUCHING, INVALID = E.NH_RECOVER_PUSHED, E.NH_RECOVER_OVERLAPPING, E.NH_RECOVER_TOUCHING, E.NH_RECOVER_INVALID
STOPPED = OVERLAPPING | TOUCHING | INVALID


def world(boxes=(), spheres=()):
    """(rec, nbox) of a static world: boxes as (centre, half extents[, rotation]), spheres as (centre, radius); every collider belongs to body 0."""
    rec = np.zeros(len(boxes) + len(spheres), dtype=H.REC)
    rec["q"] = HR.IDENTITY
    for i, b in enumerate(boxes):
        rec["p"][i], rec["h"][i] = b[0], b[1]
        if len(b) > 2:
            rec["q"][i] = b[2]
    for j, (c, rad) in enumerate(spheres):
        rec["p"][len(boxes) + j], rec["h"][len(boxes) + j] = c, (rad, rad, rad)
    rec["tag"] = np.arange(len(rec)) + 100
    return rec, len(boxes)


FLOOR = ((0.0, -1.0, 0.0), (30.0, 1.0, 30.0))                # top face at y = 0
WALL = ((3.0, 2.0, 0.0), (1.0, 5.0, 8.0))                    # face at x = 2


def counts(rec, nbox, m, centres=None):
    """How many colliders each shape of `m` overlaps (at `centres` where given): nh_overlap's count through the penetration oracle's offsets."""
    return np.diff(HP.penetration(rec, nbox, HR.queries(m, centres))[0].astype(np.int64))


def test_records_are_the_headers(tmp_path):
    """nh_Recover and nh_RecoverResult: size and every member offset as gcc lays them out, against the ctypes mirrors and the numpy records; nh_Recover's
    first 48 bytes are nh_OverlapQuery's members, nh_RecoverResult.last is nh_PenetrationHit."""
    members = {"nh_Recover": ("center", "shape", "rotation", "size", "ignore_body", "skin", "max_iterations", "reserved"),
               "nh_RecoverResult": ("position", "flags", "push", "iterations", "last")}
    body = "".join(f'  printf("%zu %zu\\n", sizeof({s}), offsetof({s}, {m}));\n' for s, ms in members.items() for m in ms)
    body += '  printf("%zu %zu\\n", sizeof(nh_OverlapQuery), sizeof(((nh_RecoverResult*)0)->last));\n'
    body += "".join(f'  printf("%zu %zu\\n", offsetof(nh_OverlapQuery, {m}), sizeof(((nh_OverlapQuery*)0)->{m}));\n' for m in members["nh_Recover"][:5])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nudge_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = iter(subprocess.check_output([str(exe)], text=True).split("\n"))
    for s, ct, dt in (("nh_Recover", E.Recover, E.RECOVER), ("nh_RecoverResult", E.RecoverResult, E.RECOVER_RESULT)):
        for m in members[s]:
            size, off = (int(v) for v in next(lines).split())
            assert ctypes.sizeof(ct) == size == dt.itemsize == 64, s
            assert getattr(ct, m).offset == off == dt.fields[m][1], (s, m, off)
    assert [int(v) for v in next(lines).split()] == [48, 32] == [E.OVERLAP_QUERY.itemsize, E.PENETRATION_HIT.itemsize]
    for m in members["nh_Recover"][:5]:
        off, size = (int(v) for v in next(lines).split())
        assert off == E.RECOVER.fields[m][1] == E.OVERLAP_QUERY.fields[m][1] and size == E.RECOVER.fields[m][0].itemsize, m
    assert E.RECOVER_RESULT.fields["last"][0] == E.PENETRATION_HIT and E.RECOVER_RESULT.fields["last"][1] == 32
    assert HR.STATE.itemsize == 32


def test_the_entry_point_is_declared_exported_and_built():
    header = open(os.path.join(ROOT, "include", "nudge_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S)).replace(" ,", ",").replace(" )", ")")
    assert "int nh_recover(nh_context* ctx, const nh_Recover* queries, uint32_t count, nh_RecoverResult* results, uint32_t flags);" in flat
    assert "#define NH_RECOVER_MAX_ITERATIONS 8u" in header
    assert "enum { NH_RECOVER_PUSHED = 1u, NH_RECOVER_OVERLAPPING = 2u, NH_RECOVER_TOUCHING = 4u, NH_RECOVER_INVALID = 0x80000000u };" in flat
    assert (PUSHED, OVERLAPPING, TOUCHING, INVALID, E.NH_RECOVER_MAX_ITERATIONS) == (1, 2, 4, 0x80000000, 8)
    assert "nh_recover" in E.EXPORTS and callable(E.World.recover) and callable(E.World.recover_records)
    note9 = next(line for line in header.splitlines() if "The scene queries (nh_query_build" in line)
    assert "nh_recover" in note9
    so = os.path.join(ROOT, "nudge_amd", "libnudge_hip.so")
    if not os.path.exists(so):
        pytest.fail("nudge_amd/libnudge_hip.so is not built")
    assert " T nh_recover\n" in subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)


# ---- hand-built worlds ------------------------------------------------------------------------------------------------------------------------
def test_a_ball_sunk_into_a_slab_is_pushed_up_once():
    rec, nbox = world(boxes=[FLOOR])
    m = HR.recovers([(1.0, 0.3, -2.0)], radii=0.5, skin=SKIN)
    out, walks = HR.recover(rec, nbox, m, walks=True)
    o = out[0]
    assert o["flags"] == PUSHED and o["iterations"] == 1 and walks[0] == 2
    assert abs(o["position"][1] - 0.51) <= 4 * ULP and o["position"][0] == 1.0 and o["position"][2] == -2.0
    assert o["push"][0] == 0.0 and o["push"][2] == 0.0 and o["push"][1] == np.float32(o["position"][1] - np.float32(0.3))
    last = o["last"]
    assert last["normal"].tolist() == [0.0, 1.0, 0.0] and abs(last["depth"] - 0.2) <= 4 * ULP
    assert (last["body"], last["collider"], last["shape"], last["tag"]) == (0, 0, E.NH_SHAPE_BOX, 100)
    assert counts(rec, nbox, m, out["position"])[0] == 0
    # the same for a box and an upright capsule whose lowest point is 0.2 below the face
    for kw in (dict(half_extents=(0.4, 0.5, 0.3)), dict(radii=0.2, half_heights=0.3)):
        o = HR.recover(rec, nbox, HR.recovers([(1.0, 0.3, -2.0)], skin=SKIN, **kw))[0]
        assert o["flags"] == PUSHED and o["iterations"] == 1 and abs(o["position"][1] - 0.51) <= PEN_TOL, (kw, o)


def test_a_floor_and_a_wall_take_two_pushes():
    rec, nbox = world(boxes=[FLOOR, WALL])
    m = HR.recovers([(1.8, 0.3, 0.0)], radii=0.5, skin=SKIN)              # 0.3 into the wall, 0.2 into the floor: the wall first
    out, walks = HR.recover(rec, nbox, m, walks=True)
    o = out[0]
    assert o["flags"] == PUSHED and o["iterations"] == 2 and walks[0] == 3
    assert abs(o["position"][0] - 1.49) <= 4 * ULP and abs(o["position"][1] - 0.51) <= 4 * ULP and o["position"][2] == 0.0
    assert o["last"]["collider"] == 0 and o["last"]["normal"].tolist() == [0.0, 1.0, 0.0]      # the last pair kept is the floor's, of the second walk
    assert counts(rec, nbox, m, out["position"])[0] == 0
    # one push allowed: the wall's, and the floor is still there
    m["max_iterations"] = 1
    o = HR.recover(rec, nbox, m)[0]
    assert o["flags"] == PUSHED | OVERLAPPING and o["iterations"] == 1 and abs(o["position"][0] - 1.49) <= 4 * ULP and o["position"][1] == np.float32(0.3)
    assert o["last"]["collider"] == 0
    # equal depths: the tie goes to the lower index, the floor (box 0)
    m = HR.recovers([(1.75, 0.25, 0.0)], radii=0.5, skin=SKIN, max_iterations=0)
    o = HR.recover(rec, nbox, m)[0]
    assert o["last"]["collider"] == 0 and o["last"]["depth"] == 0.25 and o["flags"] == OVERLAPPING


def test_a_ball_in_a_slot_narrower_than_itself_never_frees():
    rec, nbox = world(boxes=[((-1.4, 5.0, 0.0), (1.0, 5.0, 5.0)), ((1.4, 5.0, 0.0), (1.0, 5.0, 5.0))])      # faces at x = -0.4 and x = 0.4
    for max_iterations in (1, 4, 8):
        m = HR.recovers([(0.05, 5.0, 0.0)], radii=0.5, skin=SKIN, max_iterations=max_iterations)
        out, walks = HR.recover(rec, nbox, m, walks=True)
        o = out[0]
        assert o["flags"] == PUSHED | OVERLAPPING and o["iterations"] == max_iterations and walks[0] == max_iterations + 1
        assert counts(rec, nbox, m, out["position"])[0] >= 1 and abs(o["position"][0]) < 0.5 and o["position"][1] == 5.0


def test_a_touching_pair_with_no_skin_is_left_alone():
    rec, nbox = world(boxes=[FLOOR], spheres=[((10.0, 3.0, 0.0), 1.0)])
    m = HR.recovers([(0.0, 0.5, 0.0), (11.5, 3.0, 0.0)], radii=0.5, skin=0.0)
    out, walks = HR.recover(rec, nbox, m, walks=True)
    assert (out["flags"] == TOUCHING).all() and (out["iterations"] == 0).all() and (walks == 1).all()
    assert out["position"].tobytes() == m["center"].tobytes() and not out["push"].any()
    assert (out["last"]["depth"] == 0).all() and out["last"]["shape"].tolist() == [E.NH_SHAPE_BOX, E.NH_SHAPE_SPHERE]
    # with a skin the same pairs are pushed apart by it, once
    m["skin"] = SKIN
    out = HR.recover(rec, nbox, m)
    assert (out["flags"] == PUSHED).all() and (out["iterations"] == 1).all()
    assert abs(out["position"][0][1] - 0.51) <= 4 * ULP and abs(out["position"][1][0] - 11.51) <= 16 * ULP


def _invalid_cases():
    ok = HR.recovers([(0.0, 0.3, 0.0)] * 3, skin=SKIN, radii=0.5)
    ok["shape"][1], ok["size"][1] = E.NH_SHAPE_BOX, (0.5, 0.5, 0.5)
    ok["shape"][2], ok["size"][2] = E.NH_SHAPE_CAPSULE, (0.3, 0.2, 0.0)
    sphere, box, capsule = ok[0], ok[1], ok[2]
    cases = []

    def case(base, what, **fields):
        r = base.copy()
        for k, v in fields.items():
            if isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], int):
                r[k][v[0]] = v[1]
            else:
                r[k] = v
        cases.append((what, r))
    case(sphere, "an unknown shape", shape=7)
    case(sphere, "NH_SHAPE_NONE", shape=NONE)
    for v in (np.nan, np.inf, -np.inf):
        case(sphere, f"centre {v}", center=(1, v))
        case(sphere, f"skin {v}", skin=v)
        case(sphere, f"radius {v}", size=(0, v))
        case(box, f"a box's half extent {v}", size=(2, v))
        case(box, f"a box's rotation {v}", rotation=(3, v))
        case(capsule, f"a capsule's half height {v}", size=(1, v))
        case(capsule, f"a capsule's rotation {v}", rotation=(0, v))
    case(sphere, "a negative radius", size=(0, -0.5))
    case(box, "a negative half extent", size=(1, -0.5))
    case(capsule, "a negative half height", size=(1, -0.2))
    case(sphere, "a negative skin", skin=-0.01)
    case(box, "9 iterations", max_iterations=9)
    case(capsule, "2^32 - 1 iterations", max_iterations=NONE)
    return ok, cases


def test_every_kind_of_invalid_record():
    rec, nbox = world(boxes=[FLOOR])
    ok, cases = _invalid_cases()
    assert (HR.recover(rec, nbox, ok)["flags"] == PUSHED).all()
    m = np.array([r for _, r in cases], dtype=E.RECOVER)
    out, walks = HR.recover(rec, nbox, m, walks=True)
    none = HR.none_record().tobytes()
    for (what, r), o, w in zip(cases, out, walks):
        assert o["flags"] == INVALID and o["iterations"] == 0 and w == 0, what
        assert o["position"].tobytes() == r["center"].tobytes() and o["push"].tobytes() == bytes(12) and o["last"].tobytes() == none, what
    assert (HR.begin(m)["stopped"] == 1).all() and (HR.begin(ok)["stopped"] == 0).all()


def test_what_a_shape_does_not_read_is_not_read():
    rec, nbox = world(boxes=[FLOOR, WALL], spheres=[((0.0, 0.6, 0.5), 0.4)])
    c = [(1.8, 0.3, 0.0), (0.0, 0.4, 0.0)]
    base = HR.recover(rec, nbox, HR.recovers(c, radii=0.5, skin=SKIN))
    assert (base["iterations"] >= 1).all()
    # a sphere reads neither its rotation nor size[1], size[2]; nobody reads `reserved`
    m = HR.recovers(c, radii=0.5, skin=SKIN)
    m["rotation"], m["size"][:, 1:], m["reserved"] = np.nan, np.nan, 0xDEADBEEF
    assert HR.recover(rec, nbox, m).tobytes() == base.tobytes()
    # a capsule of half height 0 is that sphere, whatever its rotation; max_iterations = 8 and skin = 0 are valid
    m = HR.recovers(c, radii=0.5, half_heights=0.0, skin=SKIN)
    m["rotation"], m["size"][:, 2] = np.nan, -1.0
    assert HR.recover(rec, nbox, m).tobytes() == base.tobytes()
    m["max_iterations"], m["skin"] = 8, 0.0
    assert (HR.recover(rec, nbox, m)["flags"] & INVALID == 0).all()


def test_the_deepest_first_order_is_total():
    rng = np.random.default_rng(830)
    d = rng.choice(np.float32([0.0, 0.25, 0.5, 1.0, np.inf]), size=(512, 2))
    c = rng.integers(0, 4, size=(512, 2))
    for (da, db), (ca, cb) in zip(d, c):
        ab, ba = HR.better(da, ca, db, cb), HR.better(db, cb, da, ca)
        assert ab != ba if (da, ca) != (db, cb) else not (ab or ba)
        assert ab == (da > db or (da == db and ca < cb))
    assert HR.better(0.0, 5, 0.0, NONE) and HR.better(0.0, 0xFFFFFFFE, 0.0, NONE) and not HR.better(0.0, NONE, 0.0, NONE)


# ---- the identities, against the penetration oracle -----------------------------------------------------------------------------------------------
def _golden(name):
    scene, _ = G.build(name)
    fx = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    return Q.records(fx["transforms"], scene), len(scene["box_tags"])


@pytest.fixture(scope="module")
def settled():
    """The settled mixed pile of the golden fixtures, one batch on it and the oracle's results: shared, and left unchanged."""
    rec, nbox = _golden("pile_mixed")
    m = RB.recovers(np.random.default_rng(831), rec, nbox, 2048)
    out, walks = HR.recover(rec, nbox, m, walks=True)
    return rec, nbox, m, out, walks


def test_walks_and_flags_agree(settled):
    rec, nbox, m, out, walks = settled
    valid = out["flags"] != INVALID
    assert (walks[~valid] == 0).all() and (walks[valid] >= 1).all() and (walks <= E.NH_RECOVER_MAX_ITERATIONS + 1).all()
    assert (out["iterations"] <= m["max_iterations"])[valid].all()
    assert (((out["flags"] & PUSHED) != 0) == (out["iterations"] >= 1)).all()
    over = (out["flags"] & OVERLAPPING) != 0
    assert (out["iterations"][over] == m["max_iterations"][over]).all() and not (over & ((out["flags"] & TOUCHING) != 0)).any()
    assert (walks[valid] == out["iterations"][valid] + 1).all()
    assert out["push"][valid].tobytes() == (out["position"][valid] - m["center"][valid]).tobytes()


def test_no_overlap_is_no_change_and_max_iterations_zero_only_looks(settled):
    rec, nbox, m, out, _ = settled
    look = m.copy()
    look["max_iterations"] = 0
    got = HR.recover(rec, nbox, look)
    valid = got["flags"] != INVALID
    off, hits, _ = HP.penetration(rec, nbox, HR.queries(look))
    found, kept = HR.deepest(off, hits, len(look))
    assert got["position"].tobytes() == look["center"].tobytes() and (got["iterations"] == 0).all() and not got["push"].any()
    # (a record that is invalid by its skin or max_iterations alone is a valid overlap query: nh_penetration answers it, nh_recover does not)
    assert got["last"][valid].tobytes() == kept[valid].tobytes() and all(r.tobytes() == HR.none_record().tobytes() for r in got["last"][~valid])
    assert np.isin(got["flags"][valid], (0, OVERLAPPING, TOUCHING)).all()
    assert ((got["flags"] == 0) == (found == 0))[valid].all() and (found[valid] != 0).mean() > 0.5
    touching = got["flags"] == TOUCHING
    assert ((kept["depth"][touching] == 0) & (look["skin"][touching] == 0)).all()
    # ... and the batch's own records that overlap nothing: flags 0, the centre's bits, the NONE record
    free = (found == 0) & (out["flags"] != INVALID)
    assert free.sum() >= 16 and (out["flags"][free] == 0).all() and out["position"][free].tobytes() == m["center"][free].tobytes()
    assert all(r.tobytes() == HR.none_record().tobytes() for r in out["last"][free])


def test_a_result_that_did_not_stop_short_is_free(settled):
    rec, nbox, m, out, _ = settled
    freed = (out["flags"] & STOPPED) == 0
    n = counts(rec, nbox, m, out["position"])
    assert freed.mean() > 0.3 and (n[freed] == 0).all()
    # and one that ended OVERLAPPING or TOUCHING overlaps something where it stands
    stuck = (out["flags"] & (OVERLAPPING | TOUCHING)) != 0
    assert stuck.sum() >= 16 and (n[stuck] >= 1).all()


def test_replay_with_one_penetration_call_per_round_gives_the_same_bytes(settled):
    rec, nbox, m, out, _ = settled
    st = HR.begin(m)
    last = np.full(len(m), HR.none_record(), dtype=E.PENETRATION_HIT)
    rounds = 0
    while (st["stopped"] == 0).any():
        assert rounds <= E.NH_RECOVER_MAX_ITERATIONS
        live = st["stopped"] == 0
        off, hits, _ = HP.penetration(rec, nbox, HR.queries(m, st["p"]))
        found, kept = HR.deepest(off, hits, len(m))
        take = live & (found != 0)
        last[take] = kept[take]
        HR.advance(m, st, found, kept)
        rounds += 1
    ref = np.zeros(len(m), dtype=E.RECOVER_RESULT)
    ref["position"], ref["flags"], ref["iterations"], ref["last"] = st["p"], st["flags"], st["iterations"], last
    ref["push"] = st["p"] - m["center"]
    bad = out["flags"] == INVALID
    ref["flags"][bad], ref["push"][bad] = INVALID, 0.0
    assert ref.tobytes() == out.tobytes() and rounds >= 3


def test_layer_masks_are_the_masked_world(settled):
    rec, nbox, m, out, _ = settled
    words = (np.random.default_rng(832).integers(0, 4, size=len(rec)) + 1).astype(np.uint32)        # 1, 2, 3 or 4 (bit 2 alone)
    for mask in (1, 2, 3):
        hidden = rec.copy()
        hidden["p"][(words & mask) == 0] = np.nan
        assert HR.recover(rec, nbox, m, words=words, mask=mask).tobytes() == HR.recover(hidden, nbox, m).tobytes()
    assert HR.recover(rec, nbox, m, words=words, mask=7).tobytes() == out.tobytes()
    none = HR.recover(rec, nbox, m, words=words, mask=0)
    valid = none["flags"] != INVALID
    assert (none["flags"][valid] == 0).all() and none["position"].tobytes() == m["center"].tobytes()
    masks = np.where(np.arange(len(m)) % 2 == 0, 1, 7).astype(np.uint32)
    per = HR.recover(rec, nbox, m, words=words, masks=masks)
    one = HR.recover(rec, nbox, m, words=words, mask=1)
    assert per[0::2].tobytes() == one[0::2].tobytes() and per[1::2].tobytes() == out[1::2].tobytes()


# ---- the GPU test's conditions, by the reference alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SMALL))
def test_the_gpu_batches_meet_their_share_conditions(name):
    """tests/test_gpu_recover.py compares 4096 records per small world with this oracle, and asks of each batch that it cannot pass on idle lanes.  With
    the same generator and seeds on the world before stepping, the reference's own results meet those conditions -- with room, since the stepped world's
    batch is another one."""
    scene = SMALL[name]()
    rec, nbox = Q.records(scene["body_transforms"], scene), len(scene["box_tags"])
    for seed in RB.SEEDS[name]:
        out = HR.recover(rec, nbox, RB.recovers(np.random.default_rng(seed), rec, nbox, 4096))
        once, twice, overlapping, free = RB.shares(out)
        assert RB.shares_hold(out), (name, seed, once, twice, overlapping, free)
        assert once >= 2 * RB.PUSHED_ONCE and twice >= 2 * RB.PUSHED_TWICE and overlapping >= 16 and free >= 16, (name, seed, once, twice, overlapping, free)


@pytest.mark.parametrize("name", ["pile_mixed", "pit6", "stacks", "compound", "mixed20"])
def test_settled_worlds_meet_the_share_conditions_too(name):
    rec, nbox = _golden(name)
    out = HR.recover(rec, nbox, RB.recovers(np.random.default_rng(833), rec, nbox, 4096))
    assert RB.shares_hold(out), (name, RB.shares(out))
