"""The builder of the tests' host libraries, and what every ctypes wrapper on top of them needs.

build() compiles C++ sources with g++ -ffp-contract=off -- so that the `__host__ __device__` arithmetic of nudge_amd/csrc returns the device's bits --
into lib<name>.so beside the first source, and loads it.  It rebuilds when a source, any header of nudge_amd/csrc/ or include/, or the oracles' shared
header is newer than the library, and puts the new library in place with one rename, so that no process ever loads a half-written one.

oracle() is the one library of all scene-query oracles (tests/hostoracle/host*.cpp); the host*_util modules are its per-family wrappers."""
import ctypes as C
import functools
import glob
import os
import subprocess

import numpy as np

_TESTS = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_TESTS)
_ORACLE = os.path.join(_TESTS, "hostoracle")
_LIBS = {}
# 12 words per collider (tests/hostoracle/oracle.h Rec, nh_query_tree.h's nh_QRec)
REC = np.dtype([("p", "<f4", 3), ("body", "<u4"), ("q", "<f4", 4), ("h", "<f4", 3), ("tag", "<u4")])


def build(name, sources, extra_flags=(), extra_deps=()):
    """The loaded lib<name>.so (one handle per name), compiled first where it is missing or older than what it is made of.  `extra_deps`: further
    files it depends on; those that do not exist are skipped."""
    if name not in _LIBS:
        so = os.path.join(os.path.dirname(sources[0]), "lib%s.so" % name)
        deps = list(sources) + glob.glob(os.path.join(_ROOT, "nudge_amd", "csrc", "*.h")) + glob.glob(os.path.join(_ROOT, "include", "*.h"))
        deps += [os.path.join(_ORACLE, "oracle.h")] + [d for d in extra_deps if os.path.exists(d)]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            tmp = "%s.%d.tmp" % (so, os.getpid())
            try:
                subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++14", "-pthread", *extra_flags, *sources, "-o", tmp])
                os.replace(tmp, so)
            finally:
                if os.path.exists(tmp):
                    os.remove(tmp)
        _LIBS[name] = C.CDLL(so)
    return _LIBS[name]


def oracle(signatures):
    """lib(): libhostoracle.so with a family's {function: (argtypes, restype)} applied; built, where that is due, and loaded by the first call."""
    @functools.lru_cache(maxsize=None)
    def lib():
        L = build("hostoracle", sorted(glob.glob(os.path.join(_ORACLE, "*.cpp"))))
        for fn, (argtypes, restype) in signatures.items():
            getattr(L, fn).argtypes, getattr(L, fn).restype = argtypes, restype
        return L
    return lib


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def f(a, n):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(n)


def threads(n=None):
    """The oracles' thread count: `n`, or every CPU up to the 16 that one command may use on the GPU machines."""
    return n or min(os.cpu_count() or 1, 16)


# a batch with offsets: records, n, nbox, queries, count, offsets, hits, capacity, threads -> the true total
BATCH = ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32], C.c_uint64)


def batch(fn, query_dtype, hit_dtype, rec, nbox, queries, capacity, hits, n_threads):
    """(offsets, hits, true total) of a BATCH function: a counting pass where capacity is None (room for every record), then the records."""
    queries = np.ascontiguousarray(queries, dtype=query_dtype)
    rec = np.ascontiguousarray(rec, dtype=REC)
    n = len(queries)
    offsets = np.zeros(n + 1, dtype=np.uint32)
    if capacity is None:
        total = fn(p(rec), len(rec), nbox, p(queries), n, p(offsets), None, 0, threads(n_threads))
        capacity = 0 if total >= 0xFFFFFFFF else int(total)
    if hits is None:
        hits = np.zeros(max(capacity, 1), dtype=hit_dtype)
    assert len(hits) >= capacity and hits.flags.c_contiguous
    total = fn(p(rec), len(rec), nbox, p(queries), n, p(offsets), p(hits) if capacity else None, capacity, threads(n_threads))
    return offsets, hits, int(total)


_records_lib = oracle({"hq_records": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 4, None)})


def records(body_transforms, scene, nbox=None, nsph=None):
    """The per-collider records of a world whose bodies stand at `body_transforms` (first nbox boxes / nsph spheres of the scene)."""
    nbox = len(scene["box_tags"]) if nbox is None else nbox
    nsph = len(scene["sphere_tags"]) if nsph is None else nsph
    bt = np.ascontiguousarray(body_transforms)
    arrs = [np.ascontiguousarray(scene[k]) for k in ("box_transforms", "box_data", "sphere_transforms", "sphere_data")]
    bx_t, sp_t = np.ascontiguousarray(scene["box_tags"], dtype=np.uint32), np.ascontiguousarray(scene["sphere_tags"], dtype=np.uint32)
    out = np.zeros(nbox + nsph, dtype=REC)
    _records_lib().hq_records(p(bt), len(bt), nbox, p(arrs[0]), p(arrs[1]), p(bx_t), nsph, p(arrs[2]), p(arrs[3]), p(sp_t), p(out))
    return out
