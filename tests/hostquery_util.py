"""ctypes access to tests/hostquery/libhostquery.so: the scene query's per-item arithmetic (nudge_amd/csrc/nh_query.h) built for the host with
g++ -ffp-contract=off -- the same bits as the device -- and a brute-force closest hit over all colliders, the oracle of the GPU's tree traversal."""
import ctypes as C
import os
import subprocess

import numpy as np

from nudge_amd import engine as E

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostquery")
_LIB = None
# hq_records: 12 words per collider (nh_query.hip's nh_QRec)
REC = np.dtype([("p", "<f4", 3), ("body", "<u4"), ("q", "<f4", 4), ("h", "<f4", 3), ("tag", "<u4")])


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_DIR, "libhostquery.so")
        src = os.path.join(_DIR, "hostquery.cpp")
        hdrs = [os.path.join(_DIR, "..", "..", "nudge_amd", "csrc", h) for h in ("nh_math.h", "nh_query.h")] + [os.path.join(_DIR, "..", "..", "include", "nudge_hip.h")]
        newest = max(os.path.getmtime(p) for p in [src] + hdrs)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++14", "-pthread", src, "-o", so])
        L = C.CDLL(so)
        L.hq_raycast.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_uint32]
        L.hq_records.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.hq_ray_sphere.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        _LIB = L
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def records(body_transforms, scene, nbox=None, nsph=None):
    """The per-collider records of a world whose bodies stand at `body_transforms` (first nbox boxes / nsph spheres of the scene)."""
    nbox = len(scene["box_tags"]) if nbox is None else nbox
    nsph = len(scene["sphere_tags"]) if nsph is None else nsph
    bt = np.ascontiguousarray(body_transforms)
    arrs = [np.ascontiguousarray(scene[k]) for k in ("box_transforms", "box_data", "sphere_transforms", "sphere_data")]
    bx_t, sp_t = np.ascontiguousarray(scene["box_tags"], dtype=np.uint32), np.ascontiguousarray(scene["sphere_tags"], dtype=np.uint32)
    out = np.zeros(nbox + nsph, dtype=REC)
    lib().hq_records(_p(bt), len(bt), nbox, _p(arrs[0]), _p(arrs[1]), _p(bx_t), nsph, _p(arrs[2]), _p(arrs[3]), _p(sp_t), _p(out))
    return out


def raycast(rec, nbox, rays, only=-1, threads=None):
    """nh_RayHit records (E.RAY_HIT) of `rays` (E.RAY) by brute force over `rec`; `only` >= 0: that one collider (combined index) alone."""
    rays = np.ascontiguousarray(rays, dtype=E.RAY)
    hits = np.zeros(len(rays), dtype=E.RAY_HIT)
    rec = np.ascontiguousarray(rec, dtype=REC)
    lib().hq_raycast(_p(rec), len(rec), nbox, _p(rays), len(rays), _p(hits), int(only), threads or os.cpu_count() or 1)
    return hits


def _f(a, n):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(n)


def ray_box(o, d, p, q, h):
    """(t, normal, hit) of nh_q_ray_box."""
    out = np.zeros(5, dtype=np.float32)
    lib().hq_ray_box(_p(_f(o, 3)), _p(_f(d, 3)), _p(_f(p, 3)), _p(_f(q, 4)), _p(_f(h, 3)), _p(out))
    return float(out[0]), out[1:4].copy(), bool(out[4])


def ray_sphere(o, d, c, r):
    out = np.zeros(5, dtype=np.float32)
    lib().hq_ray_sphere(_p(_f(o, 3)), _p(_f(d, 3)), _p(_f(c, 3)), C.c_float(r), _p(out))
    return float(out[0]), out[1:4].copy(), bool(out[4])


def pose(bpos, brot, lpos, lrot):
    """World position (3) and rotation (4) of a collider: nh_q_pose, k_xform's arithmetic."""
    out = np.zeros(7, dtype=np.float32)
    lib().hq_pose(_p(_f(bpos, 3)), _p(_f(brot, 4)), _p(_f(lpos, 3)), _p(_f(lrot, 4)), _p(out))
    return out[:3].copy(), out[3:].copy()
