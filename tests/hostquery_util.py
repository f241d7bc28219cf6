"""ctypes access to the ray predicates and the collider pose of tests/hostoracle/hostshapes.cpp (built by tests/hostlib.py): the scene query's
per-item arithmetic (nudge_amd/csrc/nh_query.h) with the device's bits, and the per-collider records every query oracle reads.  The casts themselves
are tests/hostcast_util.py's."""
import ctypes as C
import numpy as np

import hostlib as H
from hostlib import REC, records      # noqa: F401  (the per-collider records every query oracle reads)

_SIG = {
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
