"""ctypes access to tests/hostcapsule/libhostcapsule.so: the capsule arithmetic of nudge_amd/csrc/nh_query.h built for the host with
g++ -ffp-contract=off -- the same bits as the device -- with a brute-force nh_capsulecast and a brute-force nh_overlap that knows capsule queries,
over all colliders with the header's exact rules: the oracles of the GPU's tree traversals.  The per-collider records come from
tests/hostquery_util.records()."""
import ctypes as C
import os
import subprocess

import numpy as np

import hostquery_util as Q
from nudge_amd import engine as E

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcapsule")
_LIB = None
records = Q.records


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_DIR, "libhostcapsule.so")
        src = os.path.join(_DIR, "hostcapsule.cpp")
        hdrs = [os.path.join(_DIR, "..", "..", "nudge_amd", "csrc", h) for h in ("nh_math.h", "nh_query.h")] + [os.path.join(_DIR, "..", "..", "include", "nudge_hip.h")]
        newest = max(os.path.getmtime(p) for p in [src] + hdrs)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++14", "-pthread", src, "-o", so])
        L = C.CDLL(so)
        L.hc_capsulecast.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_uint32]
        L.hc_overlap.restype = C.c_uint64
        L.hc_overlap.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.hc_sweep_capsule_box.argtypes = [C.c_void_p] * 3 + [C.c_float, C.c_float] + [C.c_void_p] * 4
        L.hc_sweep_capsule_sphere.argtypes = [C.c_void_p] * 3 + [C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_void_p]
        L.hc_overlap_capsule_box.argtypes = [C.c_void_p] * 2 + [C.c_float, C.c_float] + [C.c_void_p] * 3
        L.hc_overlap_capsule_sphere.argtypes = [C.c_void_p] * 2 + [C.c_float, C.c_float, C.c_void_p, C.c_float]
        L.hc_capsule_axis.argtypes = [C.c_void_p, C.c_float, C.c_void_p]
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f(a, n):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(n)


def _threads(threads):
    return threads or min(os.cpu_count() or 1, 16)


def capsulecast(rec, nbox, casts, only=-1, threads=None):
    """nh_RayHit records (E.RAY_HIT) of `casts` (E.CAPSULE_CAST) by brute force over `rec`; `only` >= 0: that one collider (combined index) alone."""
    casts = np.ascontiguousarray(casts, dtype=E.CAPSULE_CAST)
    hits = np.zeros(len(casts), dtype=E.RAY_HIT)
    rec = np.ascontiguousarray(rec, dtype=Q.REC)
    lib().hc_capsulecast(_p(rec), len(rec), nbox, _p(casts), len(casts), _p(hits), int(only), _threads(threads))
    return hits


def overlap(rec, nbox, queries, capacity=None, hits=None, threads=None):
    """(offsets, hits, true total) of nh_overlap -- sphere, box and capsule queries -- by brute force over `rec` (hostquery_util.REC).  capacity=None:
    room for every record.  `hits` (E.OVERLAP_HIT, at least `capacity` long) is written in place when given -- bytes behind the written prefix are
    left as they are."""
    queries = np.ascontiguousarray(queries, dtype=E.OVERLAP_QUERY)
    rec = np.ascontiguousarray(rec, dtype=Q.REC)
    n = len(queries)
    offsets = np.zeros(n + 1, dtype=np.uint32)
    if capacity is None:
        total = lib().hc_overlap(_p(rec), len(rec), nbox, _p(queries), n, _p(offsets), None, 0, _threads(threads))
        capacity = 0 if total >= 0xFFFFFFFF else int(total)
    if hits is None:
        hits = np.zeros(max(capacity, 1), dtype=E.OVERLAP_HIT)
    assert len(hits) >= capacity and hits.flags.c_contiguous
    total = lib().hc_overlap(_p(rec), len(rec), nbox, _p(queries), n, _p(offsets), _p(hits) if capacity else None, capacity, _threads(threads))
    return offsets, hits, int(total)


def sweep_capsule_box(o, d, q, r, hh, p, qb, hb):
    """(t, normal, hit) of nh_q_sweep_capsule_box: the capsule (o + t d, q, r, hh) against the box (p, qb, hb)."""
    out = np.zeros(5, dtype=np.float32)
    lib().hc_sweep_capsule_box(_p(_f(o, 3)), _p(_f(d, 3)), _p(_f(q, 4)), C.c_float(r), C.c_float(hh), _p(_f(p, 3)), _p(_f(qb, 4)), _p(_f(hb, 3)), _p(out))
    return float(out[0]), out[1:4].copy(), bool(out[4])


def sweep_capsule_sphere(o, d, q, r, hh, c, R):
    """(t, normal, hit) of nh_q_sweep_capsule_sphere: the capsule (o + t d, q, r, hh) against the sphere (c, R)."""
    out = np.zeros(5, dtype=np.float32)
    lib().hc_sweep_capsule_sphere(_p(_f(o, 3)), _p(_f(d, 3)), _p(_f(q, 4)), C.c_float(r), C.c_float(hh), _p(_f(c, 3)), C.c_float(R), _p(out))
    return float(out[0]), out[1:4].copy(), bool(out[4])


def overlap_capsule_box(c, q, r, hh, p, qb, hb):
    return bool(lib().hc_overlap_capsule_box(_p(_f(c, 3)), _p(_f(q, 4)), C.c_float(r), C.c_float(hh), _p(_f(p, 3)), _p(_f(qb, 4)), _p(_f(hb, 3))))


def overlap_capsule_sphere(c, q, r, hh, p, R):
    return bool(lib().hc_overlap_capsule_sphere(_p(_f(c, 3)), _p(_f(q, 4)), C.c_float(r), C.c_float(hh), _p(_f(p, 3)), C.c_float(R)))


def capsule_axis(q, hh):
    out = np.zeros(3, dtype=np.float32)
    lib().hc_capsule_axis(_p(_f(q, 4)), C.c_float(hh), _p(out))
    return out
