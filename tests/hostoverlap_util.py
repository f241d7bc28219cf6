"""ctypes access to tests/hostoverlap/libhostoverlap.so: the overlap predicates of nudge_amd/csrc/nh_query.h built for the host with
g++ -ffp-contract=off -- the device's answers -- and a brute-force nh_overlap over all colliders with the header's exact semantics, the oracle of
the GPU's tree traversal.  The per-collider records come from tests/hostquery_util.records()."""
import ctypes as C
import os
import subprocess

import numpy as np

import hostquery_util as Q
from nudge_amd import engine as E

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostoverlap")
_LIB = None
records = Q.records


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_DIR, "libhostoverlap.so")
        src = os.path.join(_DIR, "hostoverlap.cpp")
        hdrs = [os.path.join(_DIR, "..", "..", "nudge_amd", "csrc", h) for h in ("nh_math.h", "nh_query.h")] + [os.path.join(_DIR, "..", "..", "include", "nudge_hip.h")]
        newest = max(os.path.getmtime(p) for p in [src] + hdrs)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++14", "-pthread", src, "-o", so])
        L = C.CDLL(so)
        L.ho_overlap.restype = C.c_uint64
        L.ho_overlap.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.ho_sphere_sphere.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_float]
        L.ho_sphere_box.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ho_box_box.argtypes = [C.c_void_p] * 6
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f(a, n):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(n)


def overlap(rec, nbox, queries, capacity=None, hits=None, threads=None):
    """(offsets, hits, true total) of nh_overlap by brute force over `rec` (hostquery_util.REC).  capacity=None: room for every record.  `hits`
    (E.OVERLAP_HIT, at least `capacity` long) is written in place when given -- bytes behind the written prefix are left as they are."""
    queries = np.ascontiguousarray(queries, dtype=E.OVERLAP_QUERY)
    rec = np.ascontiguousarray(rec, dtype=Q.REC)
    n = len(queries)
    offsets = np.zeros(n + 1, dtype=np.uint32)
    threads = threads or min(os.cpu_count() or 1, 16)
    if capacity is None:
        total = lib().ho_overlap(_p(rec), len(rec), nbox, _p(queries), n, _p(offsets), None, 0, threads)
        capacity = 0 if total >= 0xFFFFFFFF else int(total)
    if hits is None:
        hits = np.zeros(max(capacity, 1), dtype=E.OVERLAP_HIT)
    assert len(hits) >= capacity and hits.flags.c_contiguous
    total = lib().ho_overlap(_p(rec), len(rec), nbox, _p(queries), n, _p(offsets), _p(hits) if capacity else None, capacity, threads)
    return offsets, hits, int(total)


def sphere_sphere(c, r, p, R):
    return bool(lib().ho_sphere_sphere(_p(_f(c, 3)), C.c_float(r), _p(_f(p, 3)), C.c_float(R)))


def sphere_box(c, r, p, q, h):
    return bool(lib().ho_sphere_box(_p(_f(c, 3)), C.c_float(r), _p(_f(p, 3)), _p(_f(q, 4)), _p(_f(h, 3))))


def box_box(ca, qa, ha, cb, qb, hb):
    """Box a is the query box, box b the collider (nh_q_overlap_box_box)."""
    return bool(lib().ho_box_box(_p(_f(ca, 3)), _p(_f(qa, 4)), _p(_f(ha, 3)), _p(_f(cb, 3)), _p(_f(qb, 4)), _p(_f(hb, 3))))
