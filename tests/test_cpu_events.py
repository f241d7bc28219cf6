"""Trigger events without a GPU: nh_overlap_bodies / nh_overlap_events (include/nudge_hip.h, "trigger events").

The declarations; the two oracles of tests/hostevents_util.py against each other -- a per-volume set computation in numpy, and
tests/hostoracle/hostevents.cpp, which runs the per-record searches of nudge_amd/csrc/nh_query.h that the device's lanes run -- and against hand-built
lists with known answers; and the conditions of the batches the GPU tests compare byte for byte (tests/events_batches.py), on the host overlap oracle
with the GPU tests' generators and seeds, so that those tests cannot pass on empty event lists."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import events_batches as B                   # noqa: E402
import hostevents_util as HE                 # noqa: E402
import hostoverlap_util as O                 # noqa: E402
from query_util import SMALL                 # noqa: E402
from nudge_amd import engine as E           # noqa: E402

NONE = 0xFFFFFFFF
SENTINEL = 0xA5
BOX, SPHERE = E.NH_SHAPE_BOX, E.NH_SHAPE_SPHERE


# ---- the declarations -------------------------------------------------------------------------------------------------------------------------
def test_the_calls_are_declared_exported_and_wrapped(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "nudge_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "typedef struct nh_HitList { uint32_t* offsets ; nh_OverlapHit* hits; uint32_t capacity; uint32_t reserved; } nh_HitList;" in flat
    assert "enum { NH_EVENTS_BY_BODY = 1u };" in flat and E.NH_EVENTS_BY_BODY == 1
    assert "int nh_overlap_bodies(nh_context* ctx, uint32_t count, const nh_HitList* in, const nh_HitList* out, uint32_t flags );" in flat
    assert ("int nh_overlap_events(nh_context* ctx, uint32_t count, const nh_HitList* prev , const nh_HitList* cur, const nh_HitList* entered, "
            "const nh_HitList* left, uint32_t flags );") in flat
    syms = subprocess.check_output(["nm", "-D", "--defined-only", E._LIB_PATH], text=True)
    for name in ("nh_overlap_bodies", "nh_overlap_events"):
        assert name in E.EXPORTS
        assert re.search(r"\bT %s$" % name, syms, flags=re.M)
    assert list(inspect.signature(E.World.overlap_bodies_records).parameters) == ["self", "n", "src", "offsets", "hits", "capacity"]
    assert list(inspect.signature(E.World.overlap_events_records).parameters) == ["self", "n", "prev", "cur", "entered", "left", "by_body"]
    assert list(inspect.signature(E.World.overlap_events).parameters) == ["self", "prev", "cur", "by_body", "capacity", "synchronize"]
    # nh_HitList as gcc lays it out and as the ctypes structure has it
    ms = ("offsets", "hits", "capacity", "reserved")
    body = "".join(f'  printf("%zu %zu\\n", sizeof(nh_HitList), offsetof(nh_HitList, {m}));\n' for m in ms)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nudge_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    for k, m in enumerate(ms):
        size, off = (int(v) for v in lines[k].split())
        assert size == ctypes.sizeof(E.HitList) == 24
        assert off == getattr(E.HitList, m).offset, (m, off)


# ---- the searches -----------------------------------------------------------------------------------------------------------------------------
def test_a_record_finds_its_segment_over_empty_ones():
    off = np.array([0, 0, 0, 3, 3, 4, 4, 4], dtype=np.uint32)          # segments 2 (3 records) and 4 (1 record); empty ones before, between, behind
    assert [HE.seg_of(off, r) for r in range(4)] == [2, 2, 2, 4]
    assert HE.seg_of(off, 4) == 7 and HE.seg_of(off, 1000) == 7        # at or behind the total: `count` itself
    rng = np.random.default_rng(1)
    counts = rng.integers(0, 4, size=500) * (rng.random(500) < 0.5)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    want = np.repeat(np.arange(500), counts)
    assert [HE.seg_of(off, r) for r in range(int(off[-1]))] == want.tolist()


def test_present_segments_are_the_written_prefix():
    off = np.array([0, 2, 2, 5, 9], dtype=np.uint32)
    L = HE.lib()
    for cap, want in ((9, [1, 1, 1, 1]), (8, [1, 1, 1, 0]), (5, [1, 1, 1, 0]), (4, [1, 1, 0, 0]), (1, [0, 0, 0, 0]), (0, [0, 0, 0, 0])):
        got = [L.he_seg_present(HE.H.p(off), 4, cap, i) for i in range(4)]
        assert got == want and HE.present((off, None, cap)).astype(int).tolist() == want, cap
    marked = off.copy()
    marked[-1] = NONE
    assert [L.he_seg_present(HE.H.p(marked), 4, 100, i) for i in range(4)] == [0, 0, 0, 0] and not HE.present((marked, None, 100)).any()
    bent = np.array([0, 5, 3, 6], dtype=np.uint32)                     # a non-monotone pair is absent
    assert [L.he_seg_present(HE.H.p(bent), 3, 100, i) for i in range(3)] == [1, 0, 1]


# ---- hand-built lists with known answers --------------------------------------------------------------------------------------------------------
def _both(prev, cur, by_body=False):
    """(entered segments, left segments) where both oracles agree byte for byte."""
    a, b = HE.events(prev, cur, by_body), HE.events_np(prev, cur, by_body)
    for (o, h), (o2, h2) in zip(a, b):
        assert o.tobytes() == o2.tobytes() and h.tobytes() == h2.tobytes()
    return tuple(HE.segments(HE.as_list(o, h)) for o, h in a)


def _bodies(lst):
    a, b = HE.bodies(lst), HE.bodies_np(lst)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    return HE.as_list(*a)


def test_empty_segments_at_the_start_the_end_and_in_a_row():
    r = lambda c, body=1: (body, c, BOX, 100 + c)          # noqa: E731
    prev = HE.make_list([[], [], [r(1), r(2)], [], [], [r(3)], []])
    cur = HE.make_list([[], [r(9)], [r(2), r(4)], [], [], [], []])
    entered, left = _both(prev, cur)
    assert entered == [[], [r(9)], [r(4)], [], [], [], []]
    assert left == [[], [], [r(1)], [], [], [r(3)], []]
    empty = HE.make_list([[], [], []])
    assert _both(empty, empty) == ([[], [], []], [[], [], []])
    assert HE.segments(_bodies(empty)) == [[], [], []]


def test_the_identity_includes_the_shape():
    boxes = HE.make_list([[(1, 0, BOX, 7), (1, 1, BOX, 7), (2, 2, BOX, 7)]])
    spheres = HE.make_list([[(1, 0, SPHERE, 7), (1, 1, SPHERE, 7), (2, 2, SPHERE, 7)]])
    entered, left = _both(boxes, spheres)
    assert entered == HE.segments(spheres) and left == HE.segments(boxes)
    # by body they are the same two bodies: no event
    assert _both(_bodies(boxes), _bodies(spheres), True) == ([[]], [[]])
    # a box and a sphere of one collider number side by side: the box stays, the sphere leaves
    mixed = HE.make_list([[(1, 3, BOX, 0), (1, 3, SPHERE, 0)]])
    entered, left = _both(mixed, HE.make_list([[(1, 3, BOX, 0)]]))
    assert entered == [[]] and left == [[(1, 3, SPHERE, 0)]]


def test_the_first_frame_and_identical_lists():
    cur = HE.make_list([[(1, 0, BOX, 5)], [], [(2, 1, BOX, 6), (3, 0, SPHERE, 7)]])
    entered, left = _both(None, cur)
    assert entered == HE.segments(cur) and left == [[], [], []]
    assert _both(cur, cur) == ([[], [], []], [[], [], []])
    assert _both(_bodies(cur), _bodies(cur), True) == ([[], [], []], [[], [], []])


def test_a_body_with_three_colliders_fires_once():
    three = [(4, 10, BOX, 1), (4, 11, BOX, 2), (4, 2, SPHERE, 3)]
    other = (9, 20, BOX, 0)
    full = HE.make_list([[three[0], three[1], other, three[2]]])          # (nh_overlap's order: the boxes by collider, then the spheres)
    assert HE.segments(_bodies(full)) == [[three[0], other]]               # ascending body, the lowest combined collider index
    # one of the three leaves: a collider event, no body event
    two = HE.make_list([[three[0], other, three[2]]])
    assert _both(full, two) == ([[]], [[three[1]]])
    assert _both(_bodies(full), _bodies(two), True) == ([[]], [[]])
    # the run's lowest collider leaves while the body stays: the by-body record changes, but there is no event
    late = HE.make_list([[three[1], other, three[2]]])
    assert HE.segments(_bodies(late)) == [[three[1], other]] and HE.segments(_bodies(full)) == [[three[0], other]]
    assert _both(_bodies(full), _bodies(late), True) == ([[]], [[]])
    # all three leave: three collider events, ONE body event, carrying the record the body had in prev
    gone = HE.make_list([[other]])
    assert _both(late, gone) == ([[]], [[three[1], three[2]]])
    assert _both(_bodies(late), _bodies(gone), True) == ([[]], [[three[1]]])
    # and back in: one body event with cur's record
    assert _both(_bodies(gone), _bodies(full), True) == ([[three[0]]], [[]])


def test_absent_segments_give_no_event_and_output_capacity_cuts_whole_segments():
    r = lambda c: (c, c, BOX, c)          # noqa: E731
    prev = HE.make_list([[r(1)], [r(2), r(3)], [r(4)], [r(5)]])
    cur = HE.make_list([[r(6)], [r(3)], [r(7), r(8)], []])
    cut = (cur[0], cur[1], 3)                                    # cur's segments 2 and 3 were not written (offsets[3] = 4 > 3)
    (eo, eh), (lo, lh) = HE.events(prev, cut)
    (eo2, eh2), (lo2, lh2) = HE.events_np(prev, cut)
    assert eo.tolist() == eo2.tolist() == [0, 1, 1, 1, 1] and lo.tolist() == lo2.tolist() == [0, 1, 2, 2, 2]
    assert eh.tobytes() == eh2.tobytes() and lh.tobytes() == lh2.tobytes()
    marked = (np.array([0, 1, 2, 4, NONE], dtype=np.uint32), cur[1], 4)
    for f in (HE.events, HE.events_np):
        (eo, _), (lo, _) = f(prev, marked)
        assert not eo.any() and not lo.any()
    # output capacity: inside a segment, and exactly a boundary
    # (what left `cur` on the way to `prev`: r(6) of volume 0, r(7) and r(8) of volume 2)
    for cap, written in ((0, 0), (1, 1), (2, 1), (3, 3), (4, 3)):
        got = []
        for f in (HE.events, HE.events_np):
            hits = np.frombuffer(bytes([SENTINEL]) * 16 * 4, dtype=E.OVERLAP_HIT).copy()
            (_, _), (lo, lh) = f(cur, prev, left_capacity=cap, left_hits=hits)
            assert lo.tolist() == [0, 1, 1, 3, 3] and set(lh[written:].tobytes()) == {SENTINEL}
            assert [tuple(int(v) for v in x) for x in lh[:written]] == [r(6), r(7), r(8)][:written]
            got.append(lh.tobytes())
        assert got[0] == got[1]


# ---- the batches of the GPU tests -------------------------------------------------------------------------------------------------------------
def _host_lists(name):
    scene = SMALL[name]()
    rec = B.initial_records(scene)
    nbox = len(scene["box_tags"])
    a, b = B.batch(name, rec)
    return tuple(HE.as_list(*O.overlap(rec, nbox, q)[:2]) for q in (a, b))


@pytest.mark.parametrize("name", sorted(SMALL))
def test_the_gpu_batches_hold_entries_exits_and_both(name):
    prev, cur = _host_lists(name)
    assert len(prev[0]) == B.COUNT + 1 == 2049
    a, b = HE.events(prev, cur), HE.events_np(prev, cur)
    for (o, h), (o2, h2) in zip(a, b):
        assert o.tobytes() == o2.tobytes() and h.tobytes() == h2.tobytes(), "the C++ oracle differs from the numpy one"
    e, l, both = B.shares(a[0][0], a[1][0])
    print(name, "entered", e, "left", l, "both", both)
    assert e >= B.ENTERED and l >= B.LEFT and both >= B.BOTH, (e, l, both)
    pb, cb = HE.bodies(prev), HE.bodies(cur)
    for got, lst in ((pb, prev), (cb, cur)):
        want = HE.bodies_np(lst)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), "the C++ bodies oracle differs from the numpy one"
    c, d = HE.events(HE.as_list(*pb), HE.as_list(*cb), True), HE.events_np(HE.as_list(*pb), HE.as_list(*cb), True)
    for (o, h), (o2, h2) in zip(c, d):
        assert o.tobytes() == o2.tobytes() and h.tobytes() == h2.tobytes(), "by body: the C++ oracle differs from the numpy one"
    if name == "compound":
        segs = [s for s in HE.segments(prev) if s]
        twice = np.mean([len({x[0] for x in s}) < len(s) for s in segs])
        print("compound: segments holding a body twice", twice, "events by collider", int(a[0][0][-1]), int(a[1][0][-1]), "by body", int(c[0][0][-1]), int(c[1][0][-1]))
        assert twice >= B.COMPOUND
        assert int(c[0][0][-1]) < int(a[0][0][-1]) and int(c[1][0][-1]) < int(a[1][0][-1])
