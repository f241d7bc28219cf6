"""ctypes access to the penetration oracle of tests/hostoracle/hostpen.cpp (built by tests/hostlib.py): the penetration arithmetic of
nudge_amd/csrc/nh_query.h with the device's bits, and a brute-force nh_penetration over all colliders with the header's exact rules, the oracle of the
GPU's nh_penetration."""
import ctypes as C
import numpy as np

import hostlib as H
from hostlib import records      # noqa: F401
from nudge_amd import engine as E

# nh_PenetrationHit (checked against the header in tests/test_cpu_penetration.py)
HIT = E.PENETRATION_HIT
_SIG = {
    "hp_penetration": H.BATCH,
    "hp_touches": ([C.c_void_p, C.c_void_p, C.c_int], C.c_int),
    "hp_pen": ([C.c_void_p, C.c_void_p, C.c_int, C.c_void_p], None),
    "hp_pairs": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p], None),
    "hp_pen_sphere_sphere": ([C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_void_p], None),
    "hp_pen_sphere_box": ([C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], None),
    "hp_pen_box_sphere": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p], None),
    "hp_pen_capsule_sphere": ([C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_float, C.c_void_p], None),
    "hp_pen_box_box": ([C.c_void_p] * 7, None),
    "hp_pen_capsule_box": ([C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], None),
    "hp_point_box_distance": ([C.c_void_p] * 4, C.c_float),
}
lib = H.oracle(_SIG)


def penetration(rec, nbox, queries, capacity=None, hits=None, threads=None):
    """(offsets, hits, true total) of nh_penetration -- sphere, box and capsule queries -- by brute force over `rec` (hostlib.REC).
    capacity=None: room for every record.  `hits` (HIT, at least `capacity` long) is written in place when given -- bytes behind the written prefix
    are left as they are."""
    return H.batch(lib().hp_penetration, E.OVERLAP_QUERY, HIT, rec, nbox, queries, capacity, hits, threads)


def pairs(queries, rec, box):
    """Query i against collider record i (box[i]: a box collider): (accepted by nh_overlap's predicate, normals (n, 3), depths (n,))."""
    queries = np.ascontiguousarray(queries, dtype=E.OVERLAP_QUERY)
    rec = np.ascontiguousarray(rec, dtype=H.REC)
    box = np.ascontiguousarray(box, dtype=np.uint8)
    assert len(queries) == len(rec) == len(box)
    ok = np.zeros(len(queries), dtype=np.uint8)
    out = np.zeros((len(queries), 4), dtype=np.float32)
    lib().hp_pairs(H.p(queries), H.p(rec), H.p(box), len(queries), H.p(ok), H.p(out))
    return ok.astype(bool), out[:, :3].copy(), out[:, 3].copy()


def _out(call, *args):
    out = np.zeros(4, dtype=np.float32)
    call(*args, H.p(out))
    return out[:3].copy(), out[3]


def pen_sphere_sphere(c, r, p, R):
    return _out(lib().hp_pen_sphere_sphere, H.p(H.f(c, 3)), C.c_float(r), H.p(H.f(p, 3)), C.c_float(R))


def pen_sphere_box(c, r, p, q, h):
    return _out(lib().hp_pen_sphere_box, H.p(H.f(c, 3)), C.c_float(r), H.p(H.f(p, 3)), H.p(H.f(q, 4)), H.p(H.f(h, 3)))


def pen_box_sphere(ca, qa, ha, p, R):
    return _out(lib().hp_pen_box_sphere, H.p(H.f(ca, 3)), H.p(H.f(qa, 4)), H.p(H.f(ha, 3)), H.p(H.f(p, 3)), C.c_float(R))


def pen_capsule_sphere(c, q, r, hh, p, R):
    return _out(lib().hp_pen_capsule_sphere, H.p(H.f(c, 3)), H.p(H.f(q, 4)), C.c_float(r), C.c_float(hh), H.p(H.f(p, 3)), C.c_float(R))


def pen_box_box(ca, qa, ha, cb, qb, hb):
    """Box a is the query box, box b the collider."""
    return _out(lib().hp_pen_box_box, H.p(H.f(ca, 3)), H.p(H.f(qa, 4)), H.p(H.f(ha, 3)), H.p(H.f(cb, 3)), H.p(H.f(qb, 4)), H.p(H.f(hb, 3)))


def pen_capsule_box(c, q, r, hh, p, qb, hb):
    return _out(lib().hp_pen_capsule_box, H.p(H.f(c, 3)), H.p(H.f(q, 4)), C.c_float(r), C.c_float(hh), H.p(H.f(p, 3)), H.p(H.f(qb, 4)), H.p(H.f(hb, 3)))


def point_box_distance(x, p, q, h):
    return np.float32(lib().hp_point_box_distance(H.p(H.f(x, 3)), H.p(H.f(p, 3)), H.p(H.f(q, 4)), H.p(H.f(h, 3))))
