"""ctypes access to the sphere-cast oracle of tests/hostoracle/hostsweep.cpp (built by tests/hostlib.py): the sphere-cast arithmetic of
nudge_amd/csrc/nh_query.h with the device's bits, and a brute-force nh_spherecast over all colliders with the header's exact rules, the oracle of the
GPU's tree traversal."""
import ctypes as C
import numpy as np

import hostlib as H
from hostlib import records      # noqa: F401
from hostquery_util import _hit5
from nudge_amd import engine as E

_SIG = {
    "hs_spherecast": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_uint32], None),
    "hs_sweep_box": ([C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], None),
    "hs_sweep_sphere": ([C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_void_p], None),
}
lib = H.oracle(_SIG)


def spherecast(rec, nbox, casts, only=-1, threads=None):
    """nh_RayHit records (E.RAY_HIT) of `casts` (E.SPHERE_CAST) by brute force over `rec`; `only` >= 0: that one collider (combined index) alone."""
    casts = np.ascontiguousarray(casts, dtype=E.SPHERE_CAST)
    hits = np.zeros(len(casts), dtype=E.RAY_HIT)
    rec = np.ascontiguousarray(rec, dtype=H.REC)
    lib().hs_spherecast(H.p(rec), len(rec), nbox, H.p(casts), len(casts), H.p(hits), int(only), H.threads(threads))
    return hits


def sweep_box(o, d, r, p, q, h):
    """(t, normal, hit) of nh_q_sweep_box."""
    return _hit5(lib().hs_sweep_box, H.p(H.f(o, 3)), H.p(H.f(d, 3)), C.c_float(r), H.p(H.f(p, 3)), H.p(H.f(q, 4)), H.p(H.f(h, 3)))


def sweep_sphere(o, d, r, c, R):
    """(t, normal, hit) of nh_q_sweep_sphere."""
    return _hit5(lib().hs_sweep_sphere, H.p(H.f(o, 3)), H.p(H.f(d, 3)), C.c_float(r), H.p(H.f(c, 3)), C.c_float(R))
