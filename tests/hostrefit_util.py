"""ctypes access to tests/hostrefit/libhostrefit.so: the cut of the scene query's box pass (nudge_amd/csrc/nh_query.h) built for the host by tests/hostlib.py --
the run length, the "crosses a run boundary" verdict and the parent word as the kernels compute them."""
import ctypes as C
import functools
import os

import hostlib as H

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostrefit", "hostrefit.cpp")


@functools.lru_cache(maxsize=None)
def lib():
    L = H.build("hostrefit", [_SRC])
    for name in ("hr_run", "hr_parent_top", "hr_parent_right", "hr_parent_id"):
        getattr(L, name).restype = C.c_uint32
    L.hr_crossing.argtypes = [C.c_uint32, C.c_uint32]
    L.hr_parent_word.argtypes = [C.c_uint32, C.c_int, C.c_int]
    L.hr_parent_word.restype = C.c_uint32
    return L


def run():
    return int(lib().hr_run())


def crossing(first, last):
    return bool(lib().hr_crossing(int(first), int(last)))


def parent_word(parent, right, top):
    return int(lib().hr_parent_word(int(parent), int(bool(right)), int(bool(top))))
