"""ctypes access to tests/hostcastall/libhostcastall.so: nh_raycast_all / nh_spherecast_all by brute force on the host -- the per-collider
arithmetic of nudge_amd/csrc/nh_query.h built with g++ -ffp-contract=off, the same bits as the device, and the header's rules around it
(ignore_body, the reach rule, the order by t with ties in index order, offsets, the capacity prefix, the marker): the oracle of the GPU's chain.
The per-collider records come from tests/hostquery_util.records()."""
import ctypes as C
import os
import subprocess

import numpy as np

import hostquery_util as Q
from nudge_amd import engine as E

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostcastall")
_LIB = None
records = Q.records


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_DIR, "libhostcastall.so")
        src = os.path.join(_DIR, "hostcastall.cpp")
        hdrs = [os.path.join(_DIR, "..", "..", "nudge_amd", "csrc", h) for h in ("nh_math.h", "nh_query.h")] + [os.path.join(_DIR, "..", "..", "include", "nudge_hip.h")]
        newest = max(os.path.getmtime(p) for p in [src] + hdrs)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++14", "-pthread", src, "-o", so])
        L = C.CDLL(so)
        for f in (L.hc_raycast_all, L.hc_spherecast_all):
            f.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
            f.restype = C.c_uint64
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _castall(fn, dtype, rec, nbox, casts, capacity, hits, threads):
    casts = np.ascontiguousarray(casts, dtype=dtype)
    rec = np.ascontiguousarray(rec, dtype=Q.REC)
    n = len(casts)
    offsets = np.zeros(n + 1, dtype=np.uint32)
    threads = threads or min(os.cpu_count() or 1, 16)
    if capacity is None:
        total = fn(_p(rec), len(rec), nbox, _p(casts), n, _p(offsets), None, 0, threads)
        capacity = 0 if total >= 0xFFFFFFFF else int(total)
    if hits is None:
        hits = np.zeros(max(capacity, 1), dtype=E.RAY_HIT)
    assert len(hits) >= capacity and hits.flags.c_contiguous
    total = fn(_p(rec), len(rec), nbox, _p(casts), n, _p(offsets), _p(hits) if capacity else None, capacity, threads)
    return offsets, hits, int(total)


def raycast_all(rec, nbox, rays, capacity=None, hits=None, threads=None):
    """(offsets, hits, true total) of nh_raycast_all by brute force over `rec` (hostquery_util.REC).  capacity=None: room for every record.  `hits`
    (E.RAY_HIT, at least `capacity` long) is written in place when given -- bytes behind the written prefix are left as they are."""
    return _castall(lib().hc_raycast_all, E.RAY, rec, nbox, rays, capacity, hits, threads)


def spherecast_all(rec, nbox, casts, capacity=None, hits=None, threads=None):
    """The same for nh_spherecast_all (`casts`: E.SPHERE_CAST)."""
    return _castall(lib().hc_spherecast_all, E.SPHERE_CAST, rec, nbox, casts, capacity, hits, threads)
