"""ctypes access to the cast oracle of tests/hostoracle/hostcast.cpp (built by tests/hostlib.py): the casts of all four shapes by brute force on the
host -- the per-collider arithmetic of nudge_amd/csrc/nh_query.h with the device's bits, and the header's rules around it (invalid casts, ignore_body,
ties, the reach rule; for the all-hits lists the order by t with ties in index order, offsets, the capacity prefix, the marker): the oracle of the
GPU's walks.  The table below says per shape what the tests and tools need to call either side."""
import collections
import ctypes as C
import functools

import numpy as np

import hostlib as H
from hostlib import records      # noqa: F401
from hostquery_util import _hit5
from nudge_amd import engine as E

# per shape: its name, the cast record, World's method prefix (<call>_records, <call>_all_records, <call>_k_records) and the oracle's shape number
Shape = collections.namedtuple("Shape", "name record call number")
RAY, SPHERE = Shape("ray", E.RAY, "raycast", 0), Shape("sphere", E.SPHERE_CAST, "spherecast", 1)
BOX, CAPSULE = Shape("box", E.BOX_CAST, "boxcast", 2), Shape("capsule", E.CAPSULE_CAST, "capsulecast", 3)
SHAPES = {s.name: s for s in (RAY, SPHERE, BOX, CAPSULE)}

lib = H.oracle({
    "hc_cast": ([C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_uint32], None),
    "hc_cast_all": ([C.c_uint32] + H.BATCH[0], H.BATCH[1]),
    "hs_sweep_box": ([C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], None),
    "hs_sweep_sphere": ([C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_void_p], None),
    "hb_sweep_box_box": ([C.c_void_p] * 8, None),
    "hb_sweep_box_sphere": ([C.c_void_p] * 5 + [C.c_float, C.c_void_p], None),
})


def shape_of(casts):
    """The entry of SHAPES whose record type `casts` has."""
    return next(s for s in SHAPES.values() if s.record == casts.dtype)


def cast(shape, rec, nbox, casts, only=-1, threads=None):
    """nh_RayHit records (E.RAY_HIT) of the closest-hit call for `casts` (shape.record) by brute force over `rec` (hostlib.REC); `only` >= 0: that
    one collider (combined index) alone."""
    casts = np.ascontiguousarray(casts, dtype=shape.record)
    hits = np.zeros(len(casts), dtype=E.RAY_HIT)
    rec = np.ascontiguousarray(rec, dtype=H.REC)
    lib().hc_cast(shape.number, H.p(rec), len(rec), nbox, H.p(casts), len(casts), H.p(hits), int(only), H.threads(threads))
    return hits


def cast_all(shape, rec, nbox, casts, capacity=None, hits=None, threads=None):
    """(offsets, hits, true total) of the all-hits call for `casts` (shape.record) by brute force over `rec`.  capacity=None: room for every record.
    `hits` (E.RAY_HIT, at least `capacity` long) is written in place when given -- bytes behind the written prefix are left as they are."""
    return H.batch(functools.partial(lib().hc_cast_all, shape.number), shape.record, E.RAY_HIT, rec, nbox, casts, capacity, hits, threads)


def sweep_box(o, d, r, p, q, h):
    """(t, normal, hit) of nh_q_sweep_box."""
    return _hit5(lib().hs_sweep_box, H.p(H.f(o, 3)), H.p(H.f(d, 3)), C.c_float(r), H.p(H.f(p, 3)), H.p(H.f(q, 4)), H.p(H.f(h, 3)))


def sweep_sphere(o, d, r, c, R):
    """(t, normal, hit) of nh_q_sweep_sphere."""
    return _hit5(lib().hs_sweep_sphere, H.p(H.f(o, 3)), H.p(H.f(d, 3)), C.c_float(r), H.p(H.f(c, 3)), C.c_float(R))


def sweep_box_box(o, d, qa, ha, p, qb, hb):
    """(t, normal, hit) of nh_q_sweep_box_box: the cast box (o + t d, qa, ha) against the box (p, qb, hb)."""
    return _hit5(lib().hb_sweep_box_box, H.p(H.f(o, 3)), H.p(H.f(d, 3)), H.p(H.f(qa, 4)), H.p(H.f(ha, 3)), H.p(H.f(p, 3)), H.p(H.f(qb, 4)), H.p(H.f(hb, 3)))


def sweep_box_sphere(o, d, qa, ha, c, R):
    """(t, normal, hit) of nh_q_sweep_box_sphere: the cast box (o + t d, qa, ha) against the sphere (c, R)."""
    return _hit5(lib().hb_sweep_box_sphere, H.p(H.f(o, 3)), H.p(H.f(d, 3)), H.p(H.f(qa, 4)), H.p(H.f(ha, 3)), H.p(H.f(c, 3)), C.c_float(R))
