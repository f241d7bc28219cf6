"""ctypes access to tests/hostboxcast/libhostboxcast.so: the box-cast arithmetic of nudge_amd/csrc/nh_query.h built for the host with
g++ -ffp-contract=off -- the same bits as the device -- and a brute-force nh_boxcast over all colliders with the header's exact rules, the oracle
of the GPU's tree traversal.  The per-collider records come from tests/hostquery_util.records()."""
import ctypes as C
import os
import subprocess

import numpy as np

import hostquery_util as Q
from nudge_amd import engine as E

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostboxcast")
_LIB = None
records = Q.records


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_DIR, "libhostboxcast.so")
        src = os.path.join(_DIR, "hostboxcast.cpp")
        hdrs = [os.path.join(_DIR, "..", "..", "nudge_amd", "csrc", h) for h in ("nh_math.h", "nh_query.h")] + [os.path.join(_DIR, "..", "..", "include", "nudge_hip.h")]
        newest = max(os.path.getmtime(p) for p in [src] + hdrs)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++14", "-pthread", src, "-o", so])
        L = C.CDLL(so)
        L.hb_boxcast.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_uint32]
        L.hb_sweep_box_box.argtypes = [C.c_void_p] * 8
        L.hb_sweep_box_sphere.argtypes = [C.c_void_p] * 5 + [C.c_float, C.c_void_p]
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f(a, n):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(n)


def boxcast(rec, nbox, casts, only=-1, threads=None):
    """nh_RayHit records (E.RAY_HIT) of `casts` (E.BOX_CAST) by brute force over `rec`; `only` >= 0: that one collider (combined index) alone."""
    casts = np.ascontiguousarray(casts, dtype=E.BOX_CAST)
    hits = np.zeros(len(casts), dtype=E.RAY_HIT)
    rec = np.ascontiguousarray(rec, dtype=Q.REC)
    lib().hb_boxcast(_p(rec), len(rec), nbox, _p(casts), len(casts), _p(hits), int(only), threads or min(os.cpu_count() or 1, 16))
    return hits


def sweep_box_box(o, d, qa, ha, p, qb, hb):
    """(t, normal, hit) of nh_q_sweep_box_box: the cast box (o + t d, qa, ha) against the box (p, qb, hb)."""
    out = np.zeros(5, dtype=np.float32)
    lib().hb_sweep_box_box(_p(_f(o, 3)), _p(_f(d, 3)), _p(_f(qa, 4)), _p(_f(ha, 3)), _p(_f(p, 3)), _p(_f(qb, 4)), _p(_f(hb, 3)), _p(out))
    return float(out[0]), out[1:4].copy(), bool(out[4])


def sweep_box_sphere(o, d, qa, ha, c, R):
    """(t, normal, hit) of nh_q_sweep_box_sphere: the cast box (o + t d, qa, ha) against the sphere (c, R)."""
    out = np.zeros(5, dtype=np.float32)
    lib().hb_sweep_box_sphere(_p(_f(o, 3)), _p(_f(d, 3)), _p(_f(qa, 4)), _p(_f(ha, 3)), _p(_f(c, 3)), C.c_float(R), _p(out))
    return float(out[0]), out[1:4].copy(), bool(out[4])
