"""ctypes access to the region oracle of tests/hostoracle/hostregion.cpp (built by tests/hostlib.py): the per-plane predicates of
nudge_amd/csrc/nh_query.h ("region") with the device's answers, and a brute-force nh_region over all colliders with the header's exact semantics,
the oracle of the GPU's entry-node sweep."""
import ctypes as C

import numpy as np

import hostlib as H
from hostlib import records      # noqa: F401
from nudge_amd import engine as E

NONE = 0xFFFFFFFF
_SIG = {
    "hq_region": H.BATCH,
    "hq_region_keeps": ([C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p], None),
    "hq_region_valid": ([C.c_void_p], C.c_int),
    "hq_region_node_outside": ([C.c_void_p] * 3, C.c_int),
    "hq_region_leaf_box": ([C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p], None),
}
lib = H.oracle(_SIG)


def regions(planes, plane_counts=None, ignore_body=NONE):
    """E.REGION records of `planes` ((n, P, 4) or (P, 4), P <= 8): plane_counts default P, planes behind P are zero."""
    planes = np.asarray(planes, dtype=np.float32)
    if planes.ndim == 2:
        planes = planes[None]
    n, P = planes.shape[:2]
    out = np.zeros(n, dtype=E.REGION)
    out["planes"][:, :P] = planes
    out["plane_count"] = P if plane_counts is None else plane_counts
    out["ignore_body"] = ignore_body
    return out


def region(rec, nbox, regs, capacity=None, hits=None, threads=None):
    """(offsets, hits, true total) of nh_region by brute force over `rec` (hostlib.REC).  capacity=None: room for every record.  `hits`
    (E.OVERLAP_HIT, at least `capacity` long) is written in place when given -- bytes behind the written prefix are left as they are."""
    return H.batch(lib().hq_region, E.REGION, E.OVERLAP_HIT, rec, nbox, regs, capacity, hits, threads)


def keeps(planes, p, q, h, box):
    """Per k: does plane k keep collider k?  planes (n, 4), p (n, 3), q (n, 4), h (n, 3; h[:, 0] the radius of a sphere).  A bool array."""
    n = len(planes)
    out = np.zeros(n, dtype=np.uint8)
    lib().hq_region_keeps(n, H.p(H.f(planes, (n, 4))), H.p(H.f(p, (n, 3))), H.p(H.f(q, (n, 4))), H.p(H.f(h, (n, 3))), 1 if box else 0, H.p(out))
    return out.astype(bool)


def valid(reg):
    reg = np.ascontiguousarray(reg, dtype=E.REGION).reshape(1)
    return bool(lib().hq_region_valid(H.p(reg)))


def node_outside(plane, lo, hi):
    return bool(lib().hq_region_node_outside(H.p(H.f(plane, 4)), H.p(H.f(lo, 3)), H.p(H.f(hi, 3))))


def leaf_box(p, q, h, box):
    lo, hi = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    lib().hq_region_leaf_box(H.p(H.f(p, 3)), H.p(H.f(q, 4)), H.p(H.f(h, 3)), 1 if box else 0, H.p(lo), H.p(hi))
    return lo, hi
