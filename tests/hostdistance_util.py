"""ctypes access to the distance oracle of tests/hostoracle/hostdistance.cpp (built by tests/hostlib.py): the distance arithmetic of
nudge_amd/csrc/nh_query.h with the device's bits, and a brute-force nh_distance over all colliders with the header's exact rules: the oracle of the
GPU's tree walk."""
import ctypes as C
import numpy as np

import hostlib as H
from hostlib import records      # noqa: F401
from nudge_amd import engine as E

_SIG = {
    "hd_distance": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_uint32], None),
    "hd_pair": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p], None),
}
lib = H.oracle(_SIG)


def queries(centres, radii=None, half_extents=None, rotations=None, half_heights=None, max_distance=np.inf, ignore_body=0xFFFFFFFF):
    """nh_DistanceQuery records (E.DISTANCE_QUERY) of n spheres (`radii`), boxes (`half_extents`) or capsules (`radii` with `half_heights`)."""
    c = np.asarray(centres, dtype=np.float32).reshape(-1, 3)
    q = np.zeros(len(c), dtype=E.DISTANCE_QUERY)
    q["center"] = c
    q["rotation"] = (0, 0, 0, 1) if rotations is None else np.asarray(rotations, dtype=np.float32).reshape(-1, 4)
    if half_extents is not None:
        q["shape"] = E.NH_SHAPE_BOX
        q["size"] = np.asarray(half_extents, dtype=np.float32).reshape(-1, 3)
    else:
        q["shape"] = E.NH_SHAPE_SPHERE if half_heights is None else E.NH_SHAPE_CAPSULE
        q["size"][:, 0] = radii
        if half_heights is not None:
            q["size"][:, 1] = half_heights
    q["max_distance"] = max_distance
    q["ignore_body"] = ignore_body
    return q


def distance(rec, nbox, queries, only=-1, threads=None):
    """nh_PointHit records (E.POINT_HIT) of `queries` (E.DISTANCE_QUERY) by brute force over `rec`; `only` >= 0: that one collider (combined index) alone."""
    queries = np.ascontiguousarray(queries, dtype=E.DISTANCE_QUERY)
    hits = np.zeros(len(queries), dtype=E.POINT_HIT)
    rec = np.ascontiguousarray(rec, dtype=H.REC)
    lib().hd_distance(H.p(rec), len(rec), nbox, H.p(queries), len(queries), H.p(hits), int(only), H.threads(threads))
    return hits


def pairs(queries, rec, box):
    """Query i against collider record i (box[i]: a box collider), the pair function alone: (separation (n,), normal (n, 3), point (n, 3))."""
    queries = np.ascontiguousarray(queries, dtype=E.DISTANCE_QUERY)
    rec = np.ascontiguousarray(rec, dtype=H.REC)
    box = np.ascontiguousarray(box, dtype=np.uint8)
    assert len(queries) == len(rec) == len(box)
    out = np.zeros((len(queries), 7), dtype=np.float32)
    lib().hd_pair(H.p(queries), H.p(rec), H.p(box), len(queries), H.p(out))
    return out[:, 0].copy(), out[:, 1:4].copy(), out[:, 4:7].copy()
