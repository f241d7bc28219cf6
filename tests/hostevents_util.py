"""The oracles of nh_overlap_bodies / nh_overlap_events (include/nudge_hip.h, "trigger events"), twice: a plain per-volume set computation in numpy,
and tests/hostoracle/hostevents.cpp, which runs the per-record functions of nudge_amd/csrc/nh_query.h ("events") that the device's lanes run.

A LIST is (offsets, hits, capacity): uint32 offsets (count + 1), E.OVERLAP_HIT records (at least `capacity`, or None) and the capacity the list call
was given.  An output is (offsets, hits): `hits` holds `capacity` records (capacity=None: exactly the total), written in place into `hits` when that
is given -- bytes behind the written prefix are left as they are."""
import ctypes as C

import numpy as np

import hostlib as H
from nudge_amd import engine as E

NONE = 0xFFFFFFFF
_U, _P = C.c_uint32, C.c_void_p
_SIG = {
    "he_events": ([_U, _P, _P, _U, _P, _P, _U, _U, _P, _P, _U, _P, _P, _U], None),
    "he_bodies": ([_U, _P, _P, _U, _P, _P, _U], None),
    "he_seg_of": ([_P, _U, _U], _U),
    "he_seg_present": ([_P, _U, _U, _U], C.c_int),
    "he_ident_find": ([_P, _U, _U, _P, _U], C.c_int),
}
lib = H.oracle(_SIG)


def as_list(offsets, hits, capacity=None):
    """A list from what a list call returned: capacity defaults to len(hits)."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
    hits = None if hits is None else np.ascontiguousarray(hits, dtype=E.OVERLAP_HIT)
    return offsets, hits, (0 if hits is None else len(hits)) if capacity is None else capacity


def make_list(segments):
    """A list of exactly its total from per-volume lists of (body, collider, shape, tag)."""
    flat = [r for s in segments for r in s]
    off = np.concatenate([[0], np.cumsum([len(s) for s in segments])]).astype(np.uint32)
    return off, np.array(flat, dtype=E.OVERLAP_HIT).reshape(-1), len(flat)


def segments(lst):
    """Per volume the list of (body, collider, shape, tag) tuples of a list whose every segment is present."""
    off, hits, _ = lst
    return [[tuple(int(v) for v in hits[r]) for r in range(off[i], off[i + 1])] for i in range(len(off) - 1)]


def present(lst):
    """Per volume: is its segment present (nh_overlap's written-prefix rule; a non-monotone pair is absent)?"""
    off, _, cap = lst
    o = off.astype(np.int64)
    return (o[1:] <= cap) & (o[:-1] <= o[1:]) & (o[-1] != NONE)


def ident(hits, by_body):
    """The identity of each record as one ordered integer: the body, or (shape, collider)."""
    return hits["body"].astype(np.int64) if by_body else (hits["shape"].astype(np.int64) << 32) | hits["collider"].astype(np.int64)


def _emit(per_volume, capacity, hits):
    """nh_overlap's output rules over per-volume record arrays: complete offsets (32-bit), a volume's records iff its segment ends at or below capacity."""
    counts = np.array([len(s) for s in per_volume], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    if capacity is None:
        capacity = int(off[-1])
    if hits is None:
        hits = np.zeros(capacity, dtype=E.OVERLAP_HIT)
    assert len(hits) >= capacity
    for i, s in enumerate(per_volume):
        if len(s) and off[i + 1] <= capacity:
            hits[off[i]:off[i + 1]] = s
    return off.astype(np.uint32), hits


def bodies_np(lst, capacity=None, hits=None):
    off, h, _ = lst
    ok = present(lst)
    out = []
    for i in range(len(off) - 1):
        if not ok[i]:
            out.append(h[:0] if h is not None else [])
            continue
        seg = h[off[i]:off[i + 1]]
        first = {}
        for k, b in enumerate(seg["body"]):          # (the input is in ascending combined collider index: the first seen is the lowest)
            first.setdefault(int(b), k)
        out.append(seg[[first[b] for b in sorted(first)]] if first else seg[:0])
    return _emit(out, capacity, hits)


def _difference(mine, other, by_body):
    off, h, _ = mine
    ok = present(mine)
    if other is not None:
        ok = ok & present(other)
    out = []
    for i in range(len(off) - 1):
        if not ok[i]:
            out.append([])
            continue
        seg = h[off[i]:off[i + 1]]
        if other is not None:
            gone = set(ident(other[1][other[0][i]:other[0][i + 1]], by_body).tolist())
            seg = seg[[k for k, v in enumerate(ident(seg, by_body).tolist()) if v not in gone]]
        out.append(seg)
    return out


def events_np(prev, cur, by_body=False, entered_capacity=None, left_capacity=None, entered_hits=None, left_hits=None):
    """((entered offsets, hits), (left offsets, hits)); prev None: the first frame."""
    n = len(cur[0]) - 1
    entered = _emit(_difference(cur, prev, by_body), entered_capacity, entered_hits)
    left = _emit(_difference(prev, cur, by_body) if prev is not None else [[]] * n, left_capacity, left_hits)
    return entered, left


def _out(n, capacity, hits):
    if hits is None:
        hits = np.zeros(capacity, dtype=E.OVERLAP_HIT)
    assert len(hits) >= capacity and hits.flags.c_contiguous
    return np.zeros(n + 1, dtype=np.uint32), hits


def _args(lst):
    off, hits, cap = lst
    return H.p(off), (H.p(hits) if hits is not None and len(hits) else None), cap


def bodies(lst, capacity=None, hits=None):
    """nh_overlap_bodies through hostevents.cpp."""
    n = len(lst[0]) - 1
    if capacity is None:
        cnt = np.zeros(n + 1, dtype=np.uint32)
        lib().he_bodies(n, *_args(lst), H.p(cnt), None, 0)
        capacity = int(cnt[-1])
    off, hits = _out(n, capacity, hits)
    lib().he_bodies(n, *_args(lst), H.p(off), H.p(hits) if capacity else None, capacity)
    return off, hits


def events(prev, cur, by_body=False, entered_capacity=None, left_capacity=None, entered_hits=None, left_hits=None):
    """nh_overlap_events through hostevents.cpp: events_np's arguments and result."""
    n = len(cur[0]) - 1
    pa = (None, None, 0) if prev is None else _args(prev)
    if entered_capacity is None or left_capacity is None:
        ce, cl = np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
        lib().he_events(n, *pa, *_args(cur), int(by_body), H.p(ce), None, 0, H.p(cl), None, 0)
        entered_capacity = int(ce[-1]) if entered_capacity is None else entered_capacity
        left_capacity = int(cl[-1]) if left_capacity is None else left_capacity
    eo, eh = _out(n, entered_capacity, entered_hits)
    lo, lh = _out(n, left_capacity, left_hits)
    lib().he_events(n, *pa, *_args(cur), int(by_body), H.p(eo), H.p(eh) if entered_capacity else None, entered_capacity,
                    H.p(lo), H.p(lh) if left_capacity else None, left_capacity)
    return (eo, eh), (lo, lh)


def seg_of(offsets, r):
    offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
    return int(lib().he_seg_of(H.p(offsets), len(offsets) - 1, r))
