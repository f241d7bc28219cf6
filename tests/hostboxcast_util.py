"""ctypes access to the box-cast oracle of tests/hostoracle/hostboxcast.cpp (built by tests/hostlib.py): the box-cast arithmetic of
nudge_amd/csrc/nh_query.h with the device's bits, and a brute-force nh_boxcast over all colliders with the header's exact rules, the oracle of the
GPU's tree traversal."""
import ctypes as C
import numpy as np

import hostlib as H
from hostlib import records      # noqa: F401
from hostquery_util import _hit5
from nudge_amd import engine as E

_SIG = {
    "hb_boxcast": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_uint32], None),
    "hb_sweep_box_box": ([C.c_void_p] * 8, None),
    "hb_sweep_box_sphere": ([C.c_void_p] * 5 + [C.c_float, C.c_void_p], None),
}
lib = H.oracle(_SIG)


def boxcast(rec, nbox, casts, only=-1, threads=None):
    """nh_RayHit records (E.RAY_HIT) of `casts` (E.BOX_CAST) by brute force over `rec`; `only` >= 0: that one collider (combined index) alone."""
    casts = np.ascontiguousarray(casts, dtype=E.BOX_CAST)
    hits = np.zeros(len(casts), dtype=E.RAY_HIT)
    rec = np.ascontiguousarray(rec, dtype=H.REC)
    lib().hb_boxcast(H.p(rec), len(rec), nbox, H.p(casts), len(casts), H.p(hits), int(only), H.threads(threads))
    return hits


def sweep_box_box(o, d, qa, ha, p, qb, hb):
    """(t, normal, hit) of nh_q_sweep_box_box: the cast box (o + t d, qa, ha) against the box (p, qb, hb)."""
    return _hit5(lib().hb_sweep_box_box, H.p(H.f(o, 3)), H.p(H.f(d, 3)), H.p(H.f(qa, 4)), H.p(H.f(ha, 3)), H.p(H.f(p, 3)), H.p(H.f(qb, 4)), H.p(H.f(hb, 3)))


def sweep_box_sphere(o, d, qa, ha, c, R):
    """(t, normal, hit) of nh_q_sweep_box_sphere: the cast box (o + t d, qa, ha) against the sphere (c, R)."""
    return _hit5(lib().hb_sweep_box_sphere, H.p(H.f(o, 3)), H.p(H.f(d, 3)), H.p(H.f(qa, 4)), H.p(H.f(ha, 3)), H.p(H.f(c, 3)), C.c_float(R))
