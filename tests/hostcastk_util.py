"""The oracle of the first-k casts (nh_raycast_k / nh_spherecast_k / nh_boxcast_k / nh_capsulecast_k of include/nudge_hip.h), in plain Python over
oracles that exist and share no code with the feature: the all-hits brute force of tests/hostcast_util.py gives each cast's segment, which is cut at
k and padded with the miss record; for a cast whose segment is empty the miss is the record of the closest-hit brute force beside it (a loop of its
own over other predicates), which must be a miss.  Nothing here keeps a bounded list.  premise() is tests/hostoracle/hostcastk.cpp: the pruning
premise of the k walk, counted at the leaves."""
import ctypes as C

import numpy as np

import hostlib as H
from hostcast_util import cast, cast_all, shape_of
from hostlib import records      # noqa: F401
from nudge_amd import engine as E

NONE = 0xFFFFFFFF

_lib = H.oracle({"hk_premise": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_uint32],
                                C.c_uint64)})


def segments(rec, nbox, casts):
    """(offsets, hits) of the all-hits brute force for `casts`, whatever their shape: every segment complete."""
    off, hits, total = cast_all(shape_of(casts), rec, nbox, casts)
    assert total < NONE
    return off, hits[:total]


def misses(rec, nbox, casts, empty):
    """The miss record of every cast (E.RAY_HIT): shape NONE, normal 0, nobody, t = max_t -- NaN where the closest-hit brute force writes NaN.  For
    the casts of an `empty` segment it is that brute force's own record, which must be a miss."""
    best = cast(shape_of(casts), rec, nbox, casts)
    assert (best["shape"][empty] == NONE).all(), "the closest-hit brute force hits where the all-hits segment is empty"
    # a record the closest-hit call writes as t = NaN: exactly the invalid ones, which list nothing (so `best` is their miss), and a NaN max_t
    miss = np.zeros(len(casts), dtype=E.RAY_HIT)
    miss["t"] = casts["max_t"]
    miss["body"] = miss["collider"] = miss["tag"] = NONE
    miss["shape"] = E.NH_SHAPE_NONE
    miss[empty] = best[empty]
    return miss


def cast_k(rec, nbox, casts, k, seg=None):
    """(counts, hits) of the first-k call: counts uint32 (n), hits E.RAY_HIT (n, k).  `seg`: segments() of the same casts, where the caller has it."""
    off, all_hits = seg if seg is not None else segments(rec, nbox, casts)
    n = len(casts)
    size = np.diff(off.astype(np.int64))
    miss = misses(rec, nbox, casts, size == 0)
    counts = np.minimum(size, k).astype(np.uint32)
    hits = np.repeat(miss, k).reshape(n, k)
    for j in range(k):
        has = size > j
        hits[has, j] = all_hits[off[:-1][has].astype(np.int64) + j]
    return counts, hits


def premise(rec, nbox, casts, seg=None, extra=0.0, threads=None):
    """The number of listed (cast, collider) pairs whose leaf box the k walk's node test does not enter at or before the listed t."""
    off, hits = seg if seg is not None else segments(rec, nbox, casts)
    rec = np.ascontiguousarray(rec, dtype=H.REC)
    casts = np.ascontiguousarray(casts)
    hits = np.ascontiguousarray(hits) if len(hits) else np.zeros(1, dtype=E.RAY_HIT)
    off = np.ascontiguousarray(off, dtype=np.uint32)
    return int(_lib().hk_premise(H.p(rec), len(rec), nbox, shape_of(casts).number, H.p(casts), len(casts), H.p(off), H.p(hits), C.c_float(extra),
                                 H.threads(threads)))
