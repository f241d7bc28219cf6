"""ctypes access to tests/hostpoint/libhostpoint.so: the closest-point arithmetic of nudge_amd/csrc/nh_query.h built for the host with
g++ -ffp-contract=off -- the same bits as the device -- with a brute-force nh_closest over all colliders with the header's exact rules: the oracle
of the GPU's tree walk.  The per-collider records come from tests/hostquery_util.records()."""
import ctypes as C
import os
import subprocess

import numpy as np

import hostquery_util as Q
from nudge_amd import engine as E

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostpoint")
_LIB = None
records = Q.records


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_DIR, "libhostpoint.so")
        src = os.path.join(_DIR, "hostpoint.cpp")
        hdrs = [os.path.join(_DIR, "..", "..", "nudge_amd", "csrc", h) for h in ("nh_math.h", "nh_query.h")] + [os.path.join(_DIR, "..", "..", "include", "nudge_hip.h")]
        newest = max(os.path.getmtime(p) for p in [src] + hdrs)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++14", "-pthread", src, "-o", so])
        L = C.CDLL(so)
        L.hp_closest.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_uint32]
        L.hp_point_box.argtypes = [C.c_void_p] * 5
        L.hp_point_sphere.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        L.hp_point_node.argtypes = [C.c_void_p] * 3
        L.hp_point_node.restype = C.c_float
        L.hp_point_key.argtypes = [C.c_float, C.c_float]
        L.hp_point_key.restype = C.c_float
        L.hp_leaf_box.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f(a, n):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(n)


def _threads(threads):
    return threads or min(os.cpu_count() or 1, 16)


def closest(rec, nbox, queries, only=-1, threads=None):
    """nh_PointHit records (E.POINT_HIT) of `queries` (E.POINT_QUERY) by brute force over `rec`; `only` >= 0: that one collider (combined index) alone."""
    queries = np.ascontiguousarray(queries, dtype=E.POINT_QUERY)
    hits = np.zeros(len(queries), dtype=E.POINT_HIT)
    rec = np.ascontiguousarray(rec, dtype=Q.REC)
    lib().hp_closest(_p(rec), len(rec), nbox, _p(queries), len(queries), _p(hits), int(only), _threads(threads))
    return hits


def point_box(p, c, q, h):
    """(distance, normal, point) of nh_q_point_box: p against the box (c, q, h)."""
    out = np.zeros(7, dtype=np.float32)
    lib().hp_point_box(_p(_f(p, 3)), _p(_f(c, 3)), _p(_f(q, 4)), _p(_f(h, 3)), _p(out))
    return out[0], out[1:4].copy(), out[4:7].copy()


def point_sphere(p, c, R):
    """(distance, normal, point) of nh_q_point_sphere: p against the sphere (c, R)."""
    out = np.zeros(7, dtype=np.float32)
    lib().hp_point_sphere(_p(_f(p, 3)), _p(_f(c, 3)), C.c_float(R), _p(out))
    return out[0], out[1:4].copy(), out[4:7].copy()


def point_node(lo, hi, p):
    """nh_q_point_node: the squared distance of p from the box [lo, hi] as the walk computes it."""
    return np.float32(lib().hp_point_node(_p(_f(lo, 3)), _p(_f(hi, 3)), _p(_f(p, 3))))


def point_key(d, d2):
    return np.float32(lib().hp_point_key(C.c_float(d), C.c_float(d2)))


def leaf_box(p, q, h, box):
    """(lo, hi) of a collider's leaf box as the build stores it (nh_q_leaf_box)."""
    out = np.zeros(6, dtype=np.float32)
    lib().hp_leaf_box(_p(_f(p, 3)), _p(_f(q, 4)), _p(_f(h, 3)), 1 if box else 0, _p(out))
    return out[:3].copy(), out[3:].copy()
