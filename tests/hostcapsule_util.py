"""ctypes access to the capsule predicates of tests/hostoracle/hostshapes.cpp (built by tests/hostlib.py): the capsule arithmetic of
nudge_amd/csrc/nh_query.h with the device's bits.  overlap() is hostoverlap_util's with capsule queries valid; the capsule casts are
tests/hostcast_util.py's."""
import ctypes as C
import numpy as np

import hostlib as H
from hostlib import records      # noqa: F401
import hostoverlap_util as O
from hostquery_util import _hit5

_SIG = {
    "hc_sweep_capsule_box": ([C.c_void_p] * 3 + [C.c_float, C.c_float] + [C.c_void_p] * 4, None),
    "hc_sweep_capsule_sphere": ([C.c_void_p] * 3 + [C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_void_p], None),
    "hc_overlap_capsule_box": ([C.c_void_p] * 2 + [C.c_float, C.c_float] + [C.c_void_p] * 3, C.c_int),
    "hc_overlap_capsule_sphere": ([C.c_void_p] * 2 + [C.c_float, C.c_float, C.c_void_p, C.c_float], C.c_int),
    "hc_capsule_axis": ([C.c_void_p, C.c_float, C.c_void_p], None),
}
lib = H.oracle(_SIG)


def overlap(rec, nbox, queries, capacity=None, hits=None, threads=None):
    """hostoverlap_util.overlap() for sphere, box and capsule queries."""
    return O.overlap(rec, nbox, queries, capacity, hits, threads, capsules=True)


def sweep_capsule_box(o, d, q, r, hh, p, qb, hb):
    """(t, normal, hit) of nh_q_sweep_capsule_box: the capsule (o + t d, q, r, hh) against the box (p, qb, hb)."""
    return _hit5(lib().hc_sweep_capsule_box, H.p(H.f(o, 3)), H.p(H.f(d, 3)), H.p(H.f(q, 4)), C.c_float(r), C.c_float(hh), H.p(H.f(p, 3)), H.p(H.f(qb, 4)),
                 H.p(H.f(hb, 3)))


def sweep_capsule_sphere(o, d, q, r, hh, c, R):
    """(t, normal, hit) of nh_q_sweep_capsule_sphere: the capsule (o + t d, q, r, hh) against the sphere (c, R)."""
    return _hit5(lib().hc_sweep_capsule_sphere, H.p(H.f(o, 3)), H.p(H.f(d, 3)), H.p(H.f(q, 4)), C.c_float(r), C.c_float(hh), H.p(H.f(c, 3)), C.c_float(R))


def overlap_capsule_box(c, q, r, hh, p, qb, hb):
    return bool(lib().hc_overlap_capsule_box(H.p(H.f(c, 3)), H.p(H.f(q, 4)), C.c_float(r), C.c_float(hh), H.p(H.f(p, 3)), H.p(H.f(qb, 4)), H.p(H.f(hb, 3))))


def overlap_capsule_sphere(c, q, r, hh, p, R):
    return bool(lib().hc_overlap_capsule_sphere(H.p(H.f(c, 3)), H.p(H.f(q, 4)), C.c_float(r), C.c_float(hh), H.p(H.f(p, 3)), C.c_float(R)))


def capsule_axis(q, hh):
    out = np.zeros(3, dtype=np.float32)
    lib().hc_capsule_axis(H.p(H.f(q, 4)), C.c_float(hh), H.p(out))
    return out
