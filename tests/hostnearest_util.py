"""ctypes access to tests/hostnearest/libhostnearest.so: the oracle of the GPU's nh_closest_k, built for the host with g++ -ffp-contract=off -- the
same bits as the device.  closest_k() is a brute force that evaluates every collider as tests/hostpoint does, sorts ALL candidates and takes the first
k; insert() drives the bounded list of nudge_amd/csrc/nh_query.h (nh_q_nearest_insert) that the kernel keeps per lane.  The per-collider records come
from tests/hostquery_util.records()."""
import ctypes as C
import os
import subprocess

import numpy as np

import hostquery_util as Q
from nudge_amd import engine as E

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostnearest")
_LIB = None
records = Q.records


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_DIR, "libhostnearest.so")
        src = os.path.join(_DIR, "hostnearest.cpp")
        hdrs = [os.path.join(_DIR, "..", "..", "nudge_amd", "csrc", h) for h in ("nh_math.h", "nh_query.h")] + [os.path.join(_DIR, "..", "..", "include", "nudge_hip.h")]
        newest = max(os.path.getmtime(p) for p in [src] + hdrs)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++14", "-pthread", src, "-o", so])
        L = C.CDLL(so)
        L.hn_closest_k.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
        L.hn_insert.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
        L.hn_insert.restype = C.c_uint32
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def closest_k(rec, nbox, queries, k, threads=None):
    """(counts, hits) of `queries` (E.POINT_QUERY) by brute force over `rec`: counts uint32 (n), hits E.POINT_HIT (n, k), the nearest first."""
    queries = np.ascontiguousarray(queries, dtype=E.POINT_QUERY)
    rec = np.ascontiguousarray(rec, dtype=Q.REC)
    counts = np.zeros(len(queries), dtype=np.uint32)
    hits = np.zeros((len(queries), k), dtype=E.POINT_HIT)
    lib().hn_closest_k(_p(rec), len(rec), nbox, _p(queries), len(queries), k, _p(counts), _p(hits), threads or min(os.cpu_count() or 1, 16))
    return counts, hits


def insert(keys, idx, k, stride=1, max_d=np.inf):
    """The candidates (keys[i], idx[i]) in their order through nh_q_nearest_insert over storage of `stride`: (list keys, list indices, changed), the
    list's entries in slot order.  The words between the slots must stay as they were (checked here)."""
    keys = np.ascontiguousarray(keys, dtype=np.float32)
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    fill = 0xA5A5A5A5
    store = np.full((k, stride, 2), fill, dtype=np.uint32)
    changed = np.zeros(len(keys), dtype=np.uint8)
    held = lib().hn_insert(_p(keys), _p(idx), len(keys), k, stride, C.c_float(max_d), _p(store), _p(changed))
    assert 0 <= held <= k
    assert (store[:, 1:] == fill).all() and (store[held:, 0] == fill).all(), "nh_q_nearest_insert wrote outside the slots it holds"
    return store[:held, 0, 0].copy().view(np.float32), store[:held, 0, 1].copy(), changed.astype(bool)
