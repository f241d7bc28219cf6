"""ctypes access to the closest-point oracle of tests/hostoracle/hostpoint.cpp (built by tests/hostlib.py): the closest-point arithmetic of
nudge_amd/csrc/nh_query.h with the device's bits, and a brute-force nh_closest over all colliders with the header's exact rules: the oracle of the
GPU's tree walk."""
import ctypes as C
import numpy as np

import hostlib as H
from hostlib import records      # noqa: F401
from nudge_amd import engine as E

_SIG = {
    "hp_closest": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_uint32], None),
    "hp_point_box": ([C.c_void_p] * 5, None),
    "hp_point_sphere": ([C.c_void_p, C.c_void_p, C.c_float, C.c_void_p], None),
    "hp_point_node": ([C.c_void_p] * 3, C.c_float),
    "hp_point_key": ([C.c_float, C.c_float], C.c_float),
    "hp_leaf_box": ([C.c_void_p] * 3 + [C.c_int, C.c_void_p], None),
}
lib = H.oracle(_SIG)


def closest(rec, nbox, queries, only=-1, threads=None):
    """nh_PointHit records (E.POINT_HIT) of `queries` (E.POINT_QUERY) by brute force over `rec`; `only` >= 0: that one collider (combined index) alone."""
    queries = np.ascontiguousarray(queries, dtype=E.POINT_QUERY)
    hits = np.zeros(len(queries), dtype=E.POINT_HIT)
    rec = np.ascontiguousarray(rec, dtype=H.REC)
    lib().hp_closest(H.p(rec), len(rec), nbox, H.p(queries), len(queries), H.p(hits), int(only), H.threads(threads))
    return hits


def point_box(p, c, q, h):
    """(distance, normal, point) of nh_q_point_box: p against the box (c, q, h)."""
    out = np.zeros(7, dtype=np.float32)
    lib().hp_point_box(H.p(H.f(p, 3)), H.p(H.f(c, 3)), H.p(H.f(q, 4)), H.p(H.f(h, 3)), H.p(out))
    return out[0], out[1:4].copy(), out[4:7].copy()


def point_sphere(p, c, R):
    """(distance, normal, point) of nh_q_point_sphere: p against the sphere (c, R)."""
    out = np.zeros(7, dtype=np.float32)
    lib().hp_point_sphere(H.p(H.f(p, 3)), H.p(H.f(c, 3)), C.c_float(R), H.p(out))
    return out[0], out[1:4].copy(), out[4:7].copy()


def point_node(lo, hi, p):
    """nh_q_point_node: the squared distance of p from the box [lo, hi] as the walk computes it."""
    return np.float32(lib().hp_point_node(H.p(H.f(lo, 3)), H.p(H.f(hi, 3)), H.p(H.f(p, 3))))


def point_key(d, d2):
    return np.float32(lib().hp_point_key(C.c_float(d), C.c_float(d2)))


def leaf_box(p, q, h, box):
    """(lo, hi) of a collider's leaf box as the build stores it (nh_q_leaf_box)."""
    out = np.zeros(6, dtype=np.float32)
    lib().hp_leaf_box(H.p(H.f(p, 3)), H.p(H.f(q, 4)), H.p(H.f(h, 3)), 1 if box else 0, H.p(out))
    return out[:3].copy(), out[3:].copy()
