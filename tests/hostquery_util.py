"""ctypes access to the ray-cast oracle of tests/hostoracle/hostquery.cpp (built by tests/hostlib.py): the scene query's per-item arithmetic
(nudge_amd/csrc/nh_query.h) with the device's bits, and a brute-force closest hit over all colliders, the oracle of the GPU's tree traversal."""
import ctypes as C
import numpy as np

import hostlib as H
from hostlib import REC, records      # noqa: F401  (the per-collider records every query oracle reads)
from nudge_amd import engine as E

_SIG = {
    "hq_raycast": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_uint32], None),
    "hq_ray_box": ([C.c_void_p] * 6, None),
    "hq_ray_sphere": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p], None),
    "hq_pose": ([C.c_void_p] * 5, None),
}
lib = H.oracle(_SIG)


def _hit5(fn, *args):
    """(t, normal, hit) of a single-shape predicate that writes t, normal[3], hit (1.0 / 0.0)."""
    out = np.zeros(5, dtype=np.float32)
    fn(*args, H.p(out))
    return float(out[0]), out[1:4].copy(), bool(out[4])


def raycast(rec, nbox, rays, only=-1, threads=None):
    """nh_RayHit records (E.RAY_HIT) of `rays` (E.RAY) by brute force over `rec`; `only` >= 0: that one collider (combined index) alone."""
    rays = np.ascontiguousarray(rays, dtype=E.RAY)
    hits = np.zeros(len(rays), dtype=E.RAY_HIT)
    rec = np.ascontiguousarray(rec, dtype=REC)
    lib().hq_raycast(H.p(rec), len(rec), nbox, H.p(rays), len(rays), H.p(hits), int(only), H.threads(threads))
    return hits


def ray_box(o, d, p, q, h):
    """(t, normal, hit) of nh_q_ray_box."""
    return _hit5(lib().hq_ray_box, H.p(H.f(o, 3)), H.p(H.f(d, 3)), H.p(H.f(p, 3)), H.p(H.f(q, 4)), H.p(H.f(h, 3)))


def ray_sphere(o, d, c, r):
    return _hit5(lib().hq_ray_sphere, H.p(H.f(o, 3)), H.p(H.f(d, 3)), H.p(H.f(c, 3)), C.c_float(r))


def pose(bpos, brot, lpos, lrot):
    """World position (3) and rotation (4) of a collider: nh_q_pose, k_xform's arithmetic."""
    out = np.zeros(7, dtype=np.float32)
    lib().hq_pose(H.p(H.f(bpos, 3)), H.p(H.f(brot, 4)), H.p(H.f(lpos, 3)), H.p(H.f(lrot, 4)), H.p(out))
    return out[:3].copy(), out[3:].copy()
