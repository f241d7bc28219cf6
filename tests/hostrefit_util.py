"""ctypes access to tests/hostrefit/libhostrefit.so: the cut of the scene query's box pass (nudge_amd/csrc/nh_query.h) built for the host with g++ --
the run length, the "crosses a run boundary" verdict and the parent word as the kernels compute them."""
import ctypes as C
import os
import subprocess

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostrefit")
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(_DIR, "libhostrefit.so")
        src = os.path.join(_DIR, "hostrefit.cpp")
        hdrs = [os.path.join(_DIR, "..", "..", "nudge_amd", "csrc", h) for h in ("nh_math.h", "nh_query.h")] + [os.path.join(_DIR, "..", "..", "include", "nudge_hip.h")]
        newest = max(os.path.getmtime(p) for p in [src] + hdrs)
        if not os.path.exists(so) or os.path.getmtime(so) < newest:
            subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++14", src, "-o", so])
        L = C.CDLL(so)
        for name in ("hr_run", "hr_parent_top", "hr_parent_right", "hr_parent_id"):
            getattr(L, name).restype = C.c_uint32
        L.hr_crossing.argtypes = [C.c_uint32, C.c_uint32]
        L.hr_parent_word.argtypes = [C.c_uint32, C.c_int, C.c_int]
        L.hr_parent_word.restype = C.c_uint32
        _LIB = L
    return _LIB


def run():
    return int(lib().hr_run())


def crossing(first, last):
    return bool(lib().hr_crossing(int(first), int(last)))


def parent_word(parent, right, top):
    return int(lib().hr_parent_word(int(parent), int(bool(right)), int(bool(top))))
