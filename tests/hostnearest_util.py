"""ctypes access to the oracle of the GPU's nh_closest_k, tests/hostoracle/hostnearest.cpp (built by tests/hostlib.py, the same bits as the device).
closest_k() is a brute force that evaluates every collider as hostpoint.cpp does, sorts ALL candidates and takes the first k; insert() drives the
bounded list of nudge_amd/csrc/nh_query.h (nh_q_nearest_insert) that the kernel keeps per lane."""
import ctypes as C
import numpy as np

import hostlib as H
from hostlib import records      # noqa: F401
from nudge_amd import engine as E

_SIG = {
    "hn_closest_k": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32], None),
    "hn_insert": ([C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p], C.c_uint32),
}
lib = H.oracle(_SIG)


def closest_k(rec, nbox, queries, k, threads=None):
    """(counts, hits) of `queries` (E.POINT_QUERY) by brute force over `rec`: counts uint32 (n), hits E.POINT_HIT (n, k), the nearest first."""
    queries = np.ascontiguousarray(queries, dtype=E.POINT_QUERY)
    rec = np.ascontiguousarray(rec, dtype=H.REC)
    counts = np.zeros(len(queries), dtype=np.uint32)
    hits = np.zeros((len(queries), k), dtype=E.POINT_HIT)
    lib().hn_closest_k(H.p(rec), len(rec), nbox, H.p(queries), len(queries), k, H.p(counts), H.p(hits), H.threads(threads))
    return counts, hits


def insert(keys, idx, k, stride=1, max_d=np.inf):
    """The candidates (keys[i], idx[i]) in their order through nh_q_nearest_insert over storage of `stride`: (list keys, list indices, changed), the
    list's entries in slot order.  The words between the slots must stay as they were (checked here)."""
    keys = np.ascontiguousarray(keys, dtype=np.float32)
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    fill = 0xA5A5A5A5
    store = np.full((k, stride, 2), fill, dtype=np.uint32)
    changed = np.zeros(len(keys), dtype=np.uint8)
    held = lib().hn_insert(H.p(keys), H.p(idx), len(keys), k, stride, C.c_float(max_d), H.p(store), H.p(changed))
    assert 0 <= held <= k
    assert (store[:, 1:] == fill).all() and (store[held:, 0] == fill).all(), "nh_q_nearest_insert wrote outside the slots it holds"
    return store[:held, 0, 0].copy().view(np.float32), store[:held, 0, 1].copy(), changed.astype(bool)
