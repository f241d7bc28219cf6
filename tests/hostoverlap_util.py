"""ctypes access to the overlap oracle of tests/hostoracle/hostoverlap.cpp (built by tests/hostlib.py): the overlap predicates of
nudge_amd/csrc/nh_query.h with the device's answers, and a brute-force nh_overlap over all colliders with the
header's exact semantics, the oracle of the GPU's tree traversal."""
import ctypes as C
import numpy as np

import hostlib as H
from hostlib import records      # noqa: F401
from nudge_amd import engine as E

_SIG = {
    "ho_overlap": H.BATCH,
    "hc_overlap": H.BATCH,
    "ho_sphere_sphere": ([C.c_void_p, C.c_float, C.c_void_p, C.c_float], C.c_int),
    "ho_sphere_box": ([C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int),
    "ho_box_box": ([C.c_void_p] * 6, C.c_int),
}
lib = H.oracle(_SIG)


def overlap(rec, nbox, queries, capacity=None, hits=None, threads=None, capsules=False):
    """(offsets, hits, true total) of nh_overlap by brute force over `rec` (hostlib.REC); a capsule query is valid only with `capsules`.  capacity=None:
    room for every record.  `hits` (E.OVERLAP_HIT, at least `capacity` long) is written in place when given -- bytes behind the written prefix are
    left as they are."""
    fn = lib().hc_overlap if capsules else lib().ho_overlap
    return H.batch(fn, E.OVERLAP_QUERY, E.OVERLAP_HIT, rec, nbox, queries, capacity, hits, threads)


def sphere_sphere(c, r, p, R):
    return bool(lib().ho_sphere_sphere(H.p(H.f(c, 3)), C.c_float(r), H.p(H.f(p, 3)), C.c_float(R)))


def sphere_box(c, r, p, q, h):
    return bool(lib().ho_sphere_box(H.p(H.f(c, 3)), C.c_float(r), H.p(H.f(p, 3)), H.p(H.f(q, 4)), H.p(H.f(h, 3))))


def box_box(ca, qa, ha, cb, qb, hb):
    """Box a is the query box, box b the collider (nh_q_overlap_box_box)."""
    return bool(lib().ho_box_box(H.p(H.f(ca, 3)), H.p(H.f(qa, 4)), H.p(H.f(ha, 3)), H.p(H.f(cb, 3)), H.p(H.f(qb, 4)), H.p(H.f(hb, 3))))
