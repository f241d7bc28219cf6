"""ctypes access to tests/hostpen/libhostpen.so: the penetration arithmetic of nudge_amd/csrc/nh_query.h built for the host with
g++ -ffp-contract=off -- the same bits as the device -- with a brute-force nh_penetration over all colliders with the header's exact rules, the
oracle of the GPU's nh_penetration.  The per-collider records come from tests/hostquery_util.records()."""
import ctypes as C
import os
import subprocess

import numpy as np

import hostquery_util as Q
from nudge_amd import engine as E

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostpen")
_LIB = None
records = Q.records
# nh_PenetrationHit (checked against the header in tests/test_cpu_penetration.py)
HIT = E.PENETRATION_HIT


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_DIR, "libhostpen.so")
        src = os.path.join(_DIR, "hostpen.cpp")
        hdrs = [os.path.join(_DIR, "..", "..", "nudge_amd", "csrc", h) for h in ("nh_math.h", "nh_query.h")] + [os.path.join(_DIR, "..", "..", "include", "nudge_hip.h")]
        newest = max(os.path.getmtime(p) for p in [src] + hdrs)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++14", "-pthread", src, "-o", so])
        L = C.CDLL(so)
        L.hp_penetration.restype = C.c_uint64
        L.hp_penetration.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.hp_touches.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.hp_pen.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.hp_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.hp_pen_sphere_sphere.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_void_p]
        L.hp_pen_sphere_box.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.hp_pen_box_sphere.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        L.hp_pen_capsule_sphere.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_void_p]
        L.hp_pen_box_box.argtypes = [C.c_void_p] * 7
        L.hp_pen_capsule_box.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.hp_point_box_distance.restype = C.c_float
        L.hp_point_box_distance.argtypes = [C.c_void_p] * 4
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f(a, n):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(n)


def _threads(threads):
    return threads or min(os.cpu_count() or 1, 16)


def penetration(rec, nbox, queries, capacity=None, hits=None, threads=None):
    """(offsets, hits, true total) of nh_penetration -- sphere, box and capsule queries -- by brute force over `rec` (hostquery_util.REC).
    capacity=None: room for every record.  `hits` (HIT, at least `capacity` long) is written in place when given -- bytes behind the written prefix
    are left as they are."""
    queries = np.ascontiguousarray(queries, dtype=E.OVERLAP_QUERY)
    rec = np.ascontiguousarray(rec, dtype=Q.REC)
    n = len(queries)
    offsets = np.zeros(n + 1, dtype=np.uint32)
    if capacity is None:
        total = lib().hp_penetration(_p(rec), len(rec), nbox, _p(queries), n, _p(offsets), None, 0, _threads(threads))
        capacity = 0 if total >= 0xFFFFFFFF else int(total)
    if hits is None:
        hits = np.zeros(max(capacity, 1), dtype=HIT)
    assert len(hits) >= capacity and hits.flags.c_contiguous
    total = lib().hp_penetration(_p(rec), len(rec), nbox, _p(queries), n, _p(offsets), _p(hits) if capacity else None, capacity, _threads(threads))
    return offsets, hits, int(total)


def pairs(queries, rec, box):
    """Query i against collider record i (box[i]: a box collider): (accepted by nh_overlap's predicate, normals (n, 3), depths (n,))."""
    queries = np.ascontiguousarray(queries, dtype=E.OVERLAP_QUERY)
    rec = np.ascontiguousarray(rec, dtype=Q.REC)
    box = np.ascontiguousarray(box, dtype=np.uint8)
    assert len(queries) == len(rec) == len(box)
    ok = np.zeros(len(queries), dtype=np.uint8)
    out = np.zeros((len(queries), 4), dtype=np.float32)
    lib().hp_pairs(_p(queries), _p(rec), _p(box), len(queries), _p(ok), _p(out))
    return ok.astype(bool), out[:, :3].copy(), out[:, 3].copy()


def _out(call, *args):
    out = np.zeros(4, dtype=np.float32)
    call(*args, _p(out))
    return out[:3].copy(), out[3]


def pen_sphere_sphere(c, r, p, R):
    return _out(lib().hp_pen_sphere_sphere, _p(_f(c, 3)), C.c_float(r), _p(_f(p, 3)), C.c_float(R))


def pen_sphere_box(c, r, p, q, h):
    return _out(lib().hp_pen_sphere_box, _p(_f(c, 3)), C.c_float(r), _p(_f(p, 3)), _p(_f(q, 4)), _p(_f(h, 3)))


def pen_box_sphere(ca, qa, ha, p, R):
    return _out(lib().hp_pen_box_sphere, _p(_f(ca, 3)), _p(_f(qa, 4)), _p(_f(ha, 3)), _p(_f(p, 3)), C.c_float(R))


def pen_capsule_sphere(c, q, r, hh, p, R):
    return _out(lib().hp_pen_capsule_sphere, _p(_f(c, 3)), _p(_f(q, 4)), C.c_float(r), C.c_float(hh), _p(_f(p, 3)), C.c_float(R))


def pen_box_box(ca, qa, ha, cb, qb, hb):
    """Box a is the query box, box b the collider."""
    return _out(lib().hp_pen_box_box, _p(_f(ca, 3)), _p(_f(qa, 4)), _p(_f(ha, 3)), _p(_f(cb, 3)), _p(_f(qb, 4)), _p(_f(hb, 3)))


def pen_capsule_box(c, q, r, hh, p, qb, hb):
    return _out(lib().hp_pen_capsule_box, _p(_f(c, 3)), _p(_f(q, 4)), C.c_float(r), C.c_float(hh), _p(_f(p, 3)), _p(_f(qb, 4)), _p(_f(hb, 3)))


def point_box_distance(x, p, q, h):
    return np.float32(lib().hp_point_box_distance(_p(_f(x, 3)), _p(_f(p, 3)), _p(_f(q, 4)), _p(_f(h, 3))))
