"""Trigger events on the GPU (pytest -m gpu): nh_overlap_bodies / nh_overlap_events (include/nudge_hip.h, "trigger events").

The lists come from the GPU's own nh_overlap / nh_region list calls; the oracle is tests/hostevents_util.py's C++ one (the per-record searches of
nudge_amd/csrc/nh_query.h on the host; tests/test_cpu_events.py holds it against a numpy set computation and asserts that the batches used here hold
entries, exits and both).  Offsets and records must equal the oracle's byte for byte, and so must every byte behind an output's written prefix (a
sentinel there stays the sentinel)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import events_batches as B                   # noqa: E402
import hostevents_util as HE                 # noqa: E402
import hostregion_util as R                  # noqa: E402
import query_util as Q                       # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
SENTINEL = 0xA5
SMALL = Q.SMALL


# ---- lists on the device ------------------------------------------------------------------------------------------------------------------------
def _np_list(dl):
    """The numpy list (hostevents_util) of a device list (offsets int32, hits uint8 (capacity, 16) or None, capacity)."""
    ot, ht, cap = dl
    hits = np.zeros(0, dtype=E.OVERLAP_HIT) if ht is None else np.frombuffer(ht.cpu().numpy().tobytes(), dtype=E.OVERLAP_HIT)[:cap].copy()
    return ot.cpu().numpy().view(np.uint32).copy(), hits, cap


def _listed(w, records, q, capacity=None):
    """A device list of one list call through `records` (overlap_records / region_records) on the records `q`; capacity None: exactly the total."""
    import torch
    qt = Q.upload(w, q)
    ot, _ = records(qt)
    if capacity is None:
        capacity = int(ot[-1].item()) & NONE
    ht = torch.full((max(capacity, 1), 16), SENTINEL, dtype=torch.uint8, device=w.dev)
    if capacity:
        records(qt, offsets=ot, hits=ht, capacity=capacity)
    return ot, (ht if capacity else None), capacity


def _upload_list(w, lst):
    import torch
    off, hits, cap = lst
    ot = torch.from_numpy(off.view(np.int32).copy()).to(w.dev)
    return ot, (Q.upload(w, hits[:cap]).reshape(-1, 16) if cap else None), cap


def _output(w, n, capacity):
    """An output list: offsets of -1, `capacity` records of the sentinel (None: count only)."""
    import torch
    ot = torch.full((n + 1,), -1, dtype=torch.int32, device=w.dev)
    if capacity is None:
        return ot, None, 0
    return ot, torch.full((max(capacity, 1), 16), SENTINEL, dtype=torch.uint8, device=w.dev), capacity


def _sentinels(capacity):
    return np.frombuffer(bytes([SENTINEL]) * 16 * max(capacity or 0, 1), dtype=E.OVERLAP_HIT).copy()


def _read(out):
    ot, ht, _ = out
    return ot.cpu().numpy().view(np.uint32).copy(), (None if ht is None else np.frombuffer(ht.cpu().numpy().tobytes(), dtype=E.OVERLAP_HIT).copy())


def _same(got, want, what):
    assert got[0].tobytes() == want[0].tobytes(), f"{what}: offsets differ in {int((got[0] != want[0]).sum())} of {len(got[0])}"
    if got[1] is not None:
        a, b = got[1].view(np.uint8).reshape(-1, 16), want[1].view(np.uint8).reshape(-1, 16)
        assert a.tobytes() == b.tobytes(), f"{what}: {int((a != b).any(axis=1).sum())} of {len(a)} record slots differ"


def _bodies(w, n, dl, what, capacity=-1):
    """nh_overlap_bodies of the device list `dl` against the oracle (capacity -1: the input's; None: count only); the output as a device list."""
    cap = dl[2] if capacity == -1 else capacity
    out = _output(w, n, cap)
    w.overlap_bodies_records(n, dl, offsets=out[0], hits=out[1], capacity=out[2])
    want = HE.bodies(_np_list(dl), capacity=cap or 0, hits=_sentinels(cap))
    _same(_read(out), want, what)
    return out


def _events(w, n, dprev, dcur, by_body, what, capacities=(-1, -1)):
    """nh_overlap_events of two device lists against the oracle (a capacity of -1: the input's; None: count only); ((entered), (left)) as numpy."""
    ecap = dcur[2] if capacities[0] == -1 else capacities[0]
    lcap = (dprev[2] if dprev is not None else 0) if capacities[1] == -1 else capacities[1]
    eo, lo = _output(w, n, ecap), _output(w, n, lcap)
    w.overlap_events_records(n, dprev, dcur, entered=eo, left=lo, by_body=by_body)
    want = HE.events(None if dprev is None else _np_list(dprev), _np_list(dcur), by_body, entered_capacity=ecap or 0, left_capacity=lcap or 0,
                     entered_hits=_sentinels(ecap), left_hits=_sentinels(lcap))
    got = _read(eo), _read(lo)
    _same(got[0], want[0], what + " / entered")
    _same(got[1], want[1], what + " / left")
    return got


def _both_modes(w, n, dprev, dcur, what):
    """Both calls in both modes; (events by collider, events by body)."""
    by_collider = _events(w, n, dprev, dcur, False, what)
    bp, bc = _bodies(w, n, dprev, what + " / bodies of prev"), _bodies(w, n, dcur, what + " / bodies of cur")
    return by_collider, _events(w, n, bp, bc, True, what + " / by body")


def _total(ev):
    return int(ev[0][0][-1]), int(ev[1][0][-1])


# ---- 1: both calls, both modes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SMALL))
def test_bodies_and_events_equal_the_oracle_in_both_modes(name):
    scene = SMALL[name]()
    w = E.World(scene, flags=Q.FUSED)
    w.query_build()
    a, b = B.batch(name, Q.records(w, scene))
    n = len(a)
    at_a, at_b = _listed(w, w.overlap_records, a), _listed(w, w.overlap_records, b)
    moved, moved_bodies = _both_modes(w, n, at_a, at_b, f"{name}: the volumes move")
    e, l, both = B.shares(moved[0][0], moved[1][0])
    assert e >= B.ENTERED and l >= B.LEFT and both >= B.BOTH, (e, l, both)
    if name == "compound":
        assert _total(moved_bodies)[0] < _total(moved)[0] and _total(moved_bodies)[1] < _total(moved)[1]
    # the world moves instead: a few steps and a refit, the volumes at rest
    w.step(8)
    w.query_refit()
    later = _listed(w, w.overlap_records, a)
    stepped, _ = _both_modes(w, n, at_a, later, f"{name}: the world moves")
    assert sum(_total(stepped)) > 0
    w.close()


# ---- 2: one huge segment ----------------------------------------------------------------------------------------------------------------------------
def _box_region(lo, hi):
    pl = np.zeros((6, 4), dtype=np.float32)
    for k in range(3):
        pl[2 * k, k], pl[2 * k, 3] = 1.0, -lo[k]
        pl[2 * k + 1, k], pl[2 * k + 1, 3] = -1.0, hi[k]
    return pl


def test_two_regions_of_thousands_of_records_among_empty_ones():
    scene = S.pile(4096, 2048, seed=3)
    w = E.World(scene, flags=Q.FUSED)
    w.query_build()
    rec = Q.records(w, scene)
    lo, hi = Q.bounds(rec)
    lo, hi = lo - 0.5, hi + 0.5
    shift = np.array([0.25 * (hi[0] - lo[0]), 0.0, 0.0])
    world, shifted, empty = _box_region(lo, hi), _box_region(lo + shift, hi + shift), _box_region(hi + 1e4, hi + 1e4 + 1.0)
    prev = _listed(w, w.region_records, R.regions(np.stack([empty, empty, world, empty, empty, shifted, empty])))
    cur = _listed(w, w.region_records, R.regions(np.stack([empty, empty, shifted, empty, empty, world, empty])))
    sizes = np.diff(_np_list(prev)[0].astype(np.int64))
    assert sizes[2] == len(rec) > 6000 and sizes[5] > 2000 and not sizes[[0, 1, 3, 4, 6]].any()
    by_collider, by_body = _both_modes(w, 7, prev, cur, "two big regions")
    for ev in (by_collider, by_body):
        counts = np.diff(ev[0][0].astype(np.int64)), np.diff(ev[1][0].astype(np.int64))
        assert counts[0][2] == 0 and counts[1][2] > 100 and counts[0][5] > 100 and counts[1][5] == 0          # (what the shift cut off / brought back)
    w.close()


# ---- 3, 4, 5: capacities, truncated inputs, the first frame ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def compound():
    """One compound world with two lists of the shared batch, for the tests that only differ in capacities."""
    scene = SMALL["compound"]()
    w = E.World(scene, flags=Q.FUSED)
    w.query_build()
    a, b = B.batch("compound", Q.records(w, scene))
    lists = _listed(w, w.overlap_records, a), _listed(w, w.overlap_records, b)
    yield w, a, b, lists
    w.close()


def _cuts(offsets):
    """Capacities that cut inside a segment of at least two records, and exactly at that segment's start and end."""
    off = offsets.astype(np.int64)
    big = np.nonzero(np.diff(off) > 1)[0]
    i = big[len(big) // 2]
    return int(off[i]) + 1, int(off[i]), int(off[i + 1])


def test_output_capacity_writes_whole_segments_and_nothing_behind_them(compound):
    w, a, b, (prev, cur) = compound
    n = len(a)
    full = _events(w, n, prev, cur, False, "full")
    for k, side in enumerate(("entered", "left")):
        for cap in _cuts(full[k][0]) + (0, None):
            caps = (cap, -1) if k == 0 else (-1, cap)
            got = _events(w, n, prev, cur, False, f"{side} capacity {cap}", capacities=caps)
            assert got[k][0].tobytes() == full[k][0].tobytes(), "offsets are complete whatever the capacity"
    whole = _read(_bodies(w, n, cur, "bodies, full"))
    for cap in _cuts(whole[0]) + (0, None):
        got = _read(_bodies(w, n, cur, f"bodies capacity {cap}", capacity=cap))
        assert got[0].tobytes() == whole[0].tobytes()


def test_truncated_inputs_give_no_event_at_or_behind_the_cut(compound):
    w, a, b, (prev, cur) = compound
    n = len(a)
    full = _events(w, n, prev, cur, False, "full")
    for which in ("cur", "prev"):
        whole = cur if which == "cur" else prev
        cap = _cuts(_np_list(whole)[0])[0]
        short = _listed(w, w.overlap_records, b if which == "cur" else a, capacity=cap)
        off = _np_list(short)[0].astype(np.int64)
        cut = int(np.nonzero(off[1:] > cap)[0][0])                      # the first volume whose segment was not written
        assert 0 < cut < n
        got = _events(w, n, short if which == "prev" else prev, short if which == "cur" else cur, False, f"{which} cut at volume {cut}")
        for k in range(2):
            counts, want = np.diff(got[k][0].astype(np.int64)), np.diff(full[k][0].astype(np.int64))
            assert np.array_equal(counts[:cut], want[:cut]) and not counts[cut:].any()
        _bodies(w, n, short, f"bodies of the short {which}")
    # the overflow marker, written by hand: nothing is present
    off, hits, cap = _np_list(cur)
    off[-1] = NONE
    marked = _upload_list(w, (off, hits, cap))
    for dp, dc in ((prev, marked), (marked, cur)):
        got = _events(w, n, dp, dc, False, "the marker")
        assert not got[0][0].any() and not got[1][0].any()
    assert not _read(_bodies(w, n, marked, "bodies of the marker"))[0].any()


def test_the_first_frame_and_no_change(compound):
    w, a, b, (prev, cur) = compound
    n = len(a)
    for by_body, lst in ((False, cur), (True, _bodies(w, n, cur, "bodies"))):
        (eo, eh), (lo, lh) = _events(w, n, None, lst, by_body, "the first frame")
        want = _np_list(lst)
        assert eo.tobytes() == want[0].tobytes() and eh[:want[2]].tobytes() == want[1].tobytes() and not lo.any()
        (eo, _), (lo, _) = _events(w, n, lst, lst, by_body, "no change")
        assert not eo.any() and not lo.any()


# ---- 6: arguments -----------------------------------------------------------------------------------------------------------------------------------
def test_arguments_and_observers():
    import torch
    scene = Q.OBSERVED["pile"]()
    a, b = E.World(scene, flags=Q.FUSED), E.World(scene, flags=Q.FUSED)
    L = a.L
    n = 64
    off = torch.zeros(4 * (n + 4), dtype=torch.int32, device=a.dev)
    hits = torch.zeros((256, 16), dtype=torch.uint8, device=a.dev)

    def lst(o=off.data_ptr(), h=hits.data_ptr(), cap=256):
        return E.HitList(o, h, cap, 0)

    ok = [lst(off.data_ptr() + 4 * (n + 1) * k) for k in range(4)]
    r = [C.byref(x) for x in ok]
    assert L.nh_overlap_bodies(a.ctx, n, r[0], r[1], 0) == 1                                  # before any build: NH_ERR_INVALID
    assert L.nh_overlap_events(a.ctx, n, r[0], r[1], r[2], r[3], 0) == 1
    assert L.nh_overlap_events(None, n, r[0], r[1], r[2], r[3], 0) == 1
    a.query_build()
    assert L.nh_overlap_bodies(a.ctx, n, r[0], r[1], 1) == 1                                  # unknown flags
    assert L.nh_overlap_events(a.ctx, n, r[0], r[1], r[2], r[3], 2) == 1
    assert L.nh_overlap_events(a.ctx, n, r[0], r[1], r[2], r[3], 3) == 1
    for count in (1 << 30, NONE):                                                             # count >= 2^30
        assert L.nh_overlap_bodies(a.ctx, count, r[0], r[1], 0) == 1
        assert L.nh_overlap_events(a.ctx, count, r[0], r[1], r[2], r[3], 0) == 1
    assert L.nh_overlap_bodies(a.ctx, n, None, r[1], 0) == 1                                  # a NULL list
    assert L.nh_overlap_bodies(a.ctx, n, r[0], None, 0) == 1
    for k in (1, 2, 3):
        args = list(r)
        args[k] = None
        assert L.nh_overlap_events(a.ctx, n, *args, 0) == 1
    bad = [lst(o=0), lst(o=off.data_ptr() + 2), lst(h=0), lst(h=hits.data_ptr() + 8, cap=200)]   # offsets null / misaligned, hits null with a capacity / misaligned
    for x in bad:
        rb = C.byref(x)
        assert L.nh_overlap_bodies(a.ctx, n, rb, r[1], 0) == 1 and L.nh_overlap_bodies(a.ctx, n, r[0], rb, 0) == 1
        for k in range(4):
            args = list(r)
            args[k] = rb
            assert L.nh_overlap_events(a.ctx, n, *args, 0) == 1
    assert L.nh_overlap_bodies(a.ctx, 0, r[0], r[1], 0) == 0                                  # count 0: a no-op
    assert L.nh_overlap_events(a.ctx, 0, None, None, None, None, 0) == 0
    torch.cuda.synchronize()
    assert int(off.abs().sum()) == 0 and int(hits.sum()) == 0                                 # nothing was written
    # observers: a world that lists, reduces and diffs between its steps steps exactly like one that does not
    rec = Q.records(a, scene)
    qa = B.volumes(np.random.default_rng(7), rec, 1024)
    qb = B.shifted(np.random.default_rng(8), qa, 1.0)
    prev = None
    for k in (1, 2, 3, 5, 7, 4, 8) * 2:
        a.query_build()
        cur = _listed(a, a.overlap_records, qa if prev is None or k % 2 else qb)
        _events(a, 1024, prev, cur, False, "between steps")
        _events(a, 1024, None if prev is None else _bodies(a, 1024, prev, "prev"), _bodies(a, 1024, cur, "cur"), True, "between steps, by body")
        prev = cur
        a.step(k)
        b.step(k)
    Q.same_stepped_world(a, b, "events between steps")
    a.close(); b.close()


# ---- 7: Python ----------------------------------------------------------------------------------------------------------------------------------------
def _dict_list(d):
    off = d["offsets"].cpu().numpy().astype(np.uint32)
    return off, np.frombuffer(d["raw"].cpu().numpy().tobytes(), dtype=E.OVERLAP_HIT).copy(), d["raw"].shape[0]


def test_world_overlap_events_on_the_dicts_of_overlap_and_region(compound):
    w, a, b, (prev, cur) = compound
    sph = np.arange(len(a)) % 2 == 0                                       # (overlap() takes one shape a call: the batch's spheres)
    pd = w.overlap(a["center"][sph], radii=a["size"][sph, 0])
    cd = w.overlap(b["center"][sph], radii=b["size"][sph, 0])
    for by_body in (False, True):
        r = w.overlap_events(pd, cd, by_body=by_body, synchronize=True)
        lp, lc = _dict_list(pd), _dict_list(cd)
        if by_body:
            lp, lc = HE.as_list(*HE.bodies(lp)), HE.as_list(*HE.bodies(lc))
        want = HE.events(lp, lc, by_body)
        for key, (wo, wh) in zip(("entered", "left"), want):
            got = r[key]
            total = int(wo[-1])
            assert got["offsets"].cpu().numpy().astype(np.uint32).tobytes() == wo.tobytes() and int(got["written"]) == total > 0
            assert got["raw"].cpu().numpy().tobytes()[:16 * total] == wh[:total].tobytes()
            assert np.array_equal(got["body"].cpu().numpy()[:total], wh["body"][:total])
            assert np.array_equal(got["query"].cpu().numpy()[:total], np.repeat(np.arange(len(wo) - 1), np.diff(wo.astype(np.int64))))
    first = w.overlap_events(None, cd, synchronize=True)
    assert int(first["entered"]["written"]) == int(cd["written"]) and int(first["left"]["written"]) == 0
    assert first["entered"]["raw"].cpu().numpy().tobytes() == cd["raw"].cpu().numpy().tobytes()
    # region() dicts: one box region, and it moved
    rec = Q.records(w, SMALL["compound"]())
    lo, hi = Q.bounds(rec)
    mid = 0.5 * (lo + hi)
    boxes = [_box_region(lo - 1.0 + d, np.array([mid[0], hi[1] + 1.0, hi[2] + 1.0]) + d) for d in (np.zeros(3), np.array([5.0, 0.0, 0.0]))]
    pd, cd = w.region(boxes[0]), w.region(boxes[1])
    r = w.overlap_events(pd, cd, by_body=True, capacity=4096, synchronize=True)
    want = HE.events(HE.as_list(*HE.bodies(_dict_list(pd))), HE.as_list(*HE.bodies(_dict_list(cd))), True)
    for key, (wo, wh) in zip(("entered", "left"), want):
        total = int(wo[-1])
        assert 0 < total <= 4096 and int(r[key]["written"]) == total
        assert r[key]["raw"].cpu().numpy().tobytes()[:16 * total] == wh[:total].tobytes()
