"""The sort and scan building blocks of nudge_amd/csrc/nh_util.hip, called directly (pytest -m gpu).

Every pipeline of the library rests on them -- broadphase, tag order, sleeping export, partition refresh, BVH build, every listing query -- and the
rest of the suite only reaches them through whole worlds, at the counts and key distributions those worlds happen to produce.  Here they are called
through tests/primitives/primitives.hip (C entry points over the C++ ones, no kernel of its own) with the counts at which the code takes another
path, and compared with plain numpy.  The operations are integer and exact: every comparison is byte for byte, there is no tolerance anywhere.

In every case the count lives in device memory, the buffers are larger than the count, and everything behind the count -- in both ping-pong buffers,
in scratch, around the device words -- holds a sentinel that must still be there afterwards.

NUDGE_HIP_LIBRARY (nudge_amd/engine.py) selects another build of the library for this file too: it is loaded first and globally, so it comes before
the shim's own dependency in the lookup order and the shim's calls bind to it (a build at another path is then loaded beside the tree's copy, which
nothing calls).  That is how deliberately wrong builds were shown to fail here (docs/HISTORY.md).

A HIP error behind any call ends the whole pytest session (pytest.exit, return code 3), other test files of the same run included: nothing more is
started on a device that has reported a fault."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nudge_amd import engine as E           # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "primitives", "primitives.so")

# ---- the constants of nh_internal.h / nh_util.hip the counts below are derived from: they move with the code --------------------
NH_SORT_GRID = 512                         # nh_internal.h: workgroups of a three-kernel pass and of a scan, one contiguous chunk each
RS_TILE = 256                              # nh_util.hip: keys per tile of rs_scatter; chunks are whole tiles
OS_KPT = 8
OS_TILE = 256 * OS_KPT                     # keys per tile of a one-kernel pass
OS_GROUP = 32                              # workgroups per publish group of a one-kernel pass
OS_MAX_GRID = 1024
OS_MAX_PASSES = 8
OS_PASS_WORDS = (OS_MAX_GRID + OS_MAX_GRID // OS_GROUP + 2) * 256
SC_IPT = 8                                 # sc_final: consecutive items per thread
SC_TILE = RS_TILE * SC_IPT                 # ... and per workgroup scan
BK_TARGET = 1024                           # default keys per bucket of the seeded sort
BK_LDS_SPLITTERS = 4096                    # splitters bk_count holds in LDS; beyond, the search finishes in global memory
WAVE = 64

HIST_WORDS = 256 * NH_SORT_GRID + 512      # nh_sort_*'s `hist`
SCAN_TMP_WORDS = 2 * NH_SORT_GRID          # nh_scan*'s `tmp`
ONE_TILE_PER_CHUNK = NH_SORT_GRID * RS_TILE        # 131072: the largest count at which every chunk of a three-kernel pass / scan is one tile

S32 = 0xA5C3F00D                           # sentinels: no generated key, value, count or sum below is compared against them by accident --
S64 = 0xA5C3F00DDEADBEEF                   # they only ever sit where nothing may be written
PAD = 261                                  # words behind the count in every buffer (odd: the tail is not vector-aligned either)

SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def _sentinel(dtype):
    return np.uint64(S64) if np.dtype(dtype) == np.uint64 else np.uint32(S32)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(SIGNED[a.dtype])).to("cuda")


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _ptr(t, word=0):
    return C.c_void_p(t.data_ptr() + word * t.element_size())


def _padded(a, cap):
    out = np.full(cap, _sentinel(a.dtype), dtype=a.dtype)
    out[:len(a)] = a
    return out


def _filled(cap, dtype):
    return np.full(cap, _sentinel(dtype), dtype=dtype)


class Word:
    """One 32-bit device word between two sentinel words (a count, a total, a switch)."""

    def __init__(self, value=S32):
        self.t = _dev(np.array([S32, value, S32], dtype=np.uint32))
        self.ptr = _ptr(self.t, 1)

    def value(self):
        h = _host(self.t, np.uint32)
        assert h[0] == S32 and h[2] == S32, "a word next to a device count / total was written"
        return int(h[1])


class Prims:
    def __init__(self):
        # the library first, globally: the shim's undefined symbols then bind to this build of it, whichever NUDGE_HIP_LIBRARY names
        C.CDLL(E._LIB_PATH, mode=C.RTLD_GLOBAL)
        self.L = E.lib()
        if not os.path.exists(SHIM):
            raise RuntimeError(f"{SHIM} is missing: run `make -C nudge_amd/csrc`")
        S = self.S = C.CDLL(SHIM)
        vp, u32, i = C.c_void_p, C.c_uint32, C.c_int
        S.nhp_sort_u32_u32.argtypes = S.nhp_sort_u64_u32.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, i]
        S.nhp_sort_u64.argtypes = [vp, vp, vp, vp, vp, i, i]
        S.nhp_sort_scratch_words.argtypes = [u32]
        S.nhp_sort_scratch_words.restype = C.c_uint64
        S.nhp_onesweep_u64_u32_two_fields.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, vp, i]
        S.nhp_os_resident.argtypes = [vp]
        S.nhp_scan_u32.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp]
        S.nhp_scan_u32.restype = None
        S.nhp_scan2_u32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u32, vp]
        S.nhp_scan2_u32.restype = None
        S.nhp_bucket_create.argtypes = [vp, u32]
        S.nhp_bucket_create.restype = vp
        S.nhp_bucket_destroy.argtypes = [vp]
        S.nhp_bucket_destroy.restype = None
        S.nhp_bucket_entries.argtypes = [vp]
        S.nhp_bucket_entries.restype = u32
        S.nhp_bucket_records_ptr.argtypes = [vp]
        S.nhp_bucket_records_ptr.restype = vp
        S.nhp_bucket_begin_round.argtypes = [vp, u32, u32, u32, u32]
        S.nhp_bucket_set_records.argtypes = [vp, u32]
        S.nhp_bucket_seed.argtypes = [vp, vp]
        S.nhp_bucket_seed.restype = None
        S.nhp_bucket_sort.argtypes = [vp, vp, vp, vp, vp, i, vp, vp]
        S.nhp_bucket_sort.restype = None
        S.nhp_bucket_read.argtypes = [vp, vp]
        S.nhp_bucket_read_tables.argtypes = [vp, vp, vp, vp]
        S.nhp_synchronize.argtypes = [vp]
        self.contexts = {}
        self.ctx = self.context()
        self.hist = _dev(_filled(HIST_WORDS + PAD, np.uint32))
        self.scan_tmp = _dev(_filled(SCAN_TMP_WORDS + PAD, np.uint32))
        words = int(S.nhp_sort_scratch_words(1 << 20))
        assert words == OS_MAX_PASSES * OS_PASS_WORDS
        self.scratch = _dev(_filled(words + PAD, np.uint32))
        self._resident = 0

    def context(self, **options):
        """A fresh, never-stepped context with the given nh_set_option values (one per set of options, kept until the module is done)."""
        key = tuple(sorted(options.items()))
        if key not in self.contexts:
            ctx = C.c_void_p()
            assert self.L.nh_create(C.byref(ctx), 0, None, 0) == 0
            for name, value in key:
                assert self.L.nh_set_option(ctx, name.encode(), int(value)) == 0, name
            self.contexts[key] = ctx
        return self.contexts[key]

    def sync(self, ctx=None):
        rc = self.S.nhp_synchronize(ctx or self.ctx)
        if rc:                              # nothing more is started on a device that has reported an error
            pytest.exit(f"HIP error {rc} behind a primitive: stopping", returncode=3)

    def check_scratch(self):
        assert (_host(self.hist[HIST_WORDS:], np.uint32) == S32).all(), "a sort wrote behind its `hist`"
        assert (_host(self.scan_tmp[SCAN_TMP_WORDS:], np.uint32) == S32).all(), "a scan wrote behind its `tmp`"
        assert (_host(self.scratch[-PAD:], np.uint32) == S32).all(), "a one-kernel sort wrote behind its scratch"

    def close(self):
        for ctx in self.contexts.values():
            self.L.nh_destroy(ctx)
        self.contexts = {}

    def resident(self):
        """Workgroups a one-kernel pass may launch on this device (the context asks once, at its first such sort: an empty one here)."""
        if not self._resident:
            onesweep(self, np.zeros(0, dtype=np.uint64), 20, capacity=OS_TILE)
            self._resident = int(self.S.nhp_os_resident(self.ctx))
            assert 16 <= self._resident <= OS_MAX_GRID
        return self._resident


@pytest.fixture(scope="module")
def P():
    p = Prims()
    yield p
    p.sync()
    p.check_scratch()
    p.close()


# =====================================================================================================================================
# three-kernel stable LSD radix sorts
# =====================================================================================================================================
RADIX_COUNTS = (0, 1, WAVE - 1, WAVE, WAVE + 1, RS_TILE - 1, RS_TILE, RS_TILE + 1,
                ONE_TILE_PER_CHUNK - 1, ONE_TILE_PER_CHUNK, ONE_TILE_PER_CHUNK + 1,        # one tile per chunk becomes two
                2 * ONE_TILE_PER_CHUNK + 37859)                                              # 300 003: three tiles per chunk, the last chunks short or empty
KEY_SETS = ("random", "equal", "sorted", "reversed", "one_byte", "top_bits", "digits")


def _keys(kind, n, dtype, rng):
    bits = np.dtype(dtype).itemsize * 8
    rnd = rng.integers(0, 1 << bits, size=n, dtype=np.uint64).astype(dtype)
    if kind == "random":
        return rnd
    if kind == "equal":
        return np.full(n, 0x9E3779B97F4A7C15 & ((1 << bits) - 1), dtype=dtype)
    if kind == "sorted":
        return np.sort(rnd)
    if kind == "reversed":
        return np.sort(rnd)[::-1].copy()
    if kind == "one_byte":                 # only bits [8, 16) vary
        return ((rnd & dtype(0xFF00)) | dtype(0x5A5A5A5A5A5A005A & ((1 << bits) - 1))).astype(dtype)
    if kind == "top_bits":                 # bit 31 and bit 63 set or clear, little else: a sign extension or a narrowing shift shows here
        k = rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(31)
        if bits == 64:
            k |= rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(63)
        return (k | rng.integers(0, 3, size=n, dtype=np.uint64)).astype(dtype)
    if kind == "digits":                   # byte 0 takes all 256 values (where n allows), byte 1 a single one, the rest are random
        low = rng.permutation(np.arange(n, dtype=np.uint64) & np.uint64(0xFF))
        return ((rnd & dtype(((1 << bits) - 1) & ~0xFFFF)) | dtype(0xC300) | low.astype(dtype)).astype(dtype)
    raise ValueError(kind)


def _stable_perm(keys, begin, end):
    """The order a stable sort over bits [begin, end) leaves: the specification of every sort here."""
    width = max(end - begin, 0)
    k = keys.astype(np.uint64)
    digit = (k >> np.uint64(begin)) & np.uint64((1 << width) - 1) if width < 64 else k
    return np.argsort(digit, kind="stable")


def radix_sort(P, which, keys, begin, end):
    """One nh_sort_* call on buffers of len(keys) + PAD entries; returns (keys, values or None) of the buffer the return value names, after checking
    that nothing behind the count moved in either buffer."""
    n, dt = len(keys), keys.dtype
    cap = n + PAD
    vals = np.arange(n, dtype=np.uint32)                  # original indices: stability outside the sorted bits shows in them
    count = Word(n)
    ka, kb = _dev(_padded(keys, cap)), _dev(_filled(cap, dt))
    with_vals = which != "u64"
    if with_vals:
        va, vb = _dev(_padded(vals, cap)), _dev(_filled(cap, np.uint32))
        fn = P.S.nhp_sort_u32_u32 if which == "u32_u32" else P.S.nhp_sort_u64_u32
        in_b = fn(P.ctx, _ptr(ka), _ptr(kb), _ptr(va), _ptr(vb), count.ptr, _ptr(P.hist), begin, end)
    else:
        in_b = P.S.nhp_sort_u64(P.ctx, _ptr(ka), _ptr(kb), count.ptr, _ptr(P.hist), begin, end)
    P.sync()
    passes = len(range(begin, end, 8))
    assert in_b == (passes & 1), "the return value names the buffer of the last pass"
    assert count.value() == n
    ha, hb = _host(ka, dt), _host(kb, dt)
    assert (ha[n:] == _sentinel(dt)).all() and (hb[n:] == _sentinel(dt)).all(), "keys behind the count were written"
    if passes == 0:
        assert np.array_equal(ha[:n], keys) and (hb == _sentinel(dt)).all(), "an empty bit range moved keys"
    out_v = None
    if with_vals:
        hva, hvb = _host(va, np.uint32), _host(vb, np.uint32)
        assert (hva[n:] == S32).all() and (hvb[n:] == S32).all(), "values behind the count were written"
        if passes == 0:
            assert np.array_equal(hva[:n], vals) and (hvb == S32).all(), "an empty bit range moved values"
        out_v = (hvb if in_b else hva)[:n]
    return (hb if in_b else ha)[:n], out_v


RADIX_CASES = [(w, b, e) for w in ("u32_u32", "u64_u32", "u64")
               for b, e in ((0, 32 if w == "u32_u32" else 64), (0, 8), (8, 24), (16, 48), (8, 8))
               if not (w == "u32_u32" and e > 32)]


@pytest.mark.parametrize("which,begin,end", RADIX_CASES, ids=[f"{w}-bits{b}to{e}" for w, b, e in RADIX_CASES])
def test_radix_sort_is_the_stable_sort_of_the_bit_range(P, which, begin, end):
    dtype = np.uint32 if which == "u32_u32" else np.uint64
    rng = np.random.default_rng(1000 + 64 * begin + end)
    for n in RADIX_COUNTS:
        for kind in KEY_SETS:
            keys = _keys(kind, n, dtype, rng)
            perm = _stable_perm(keys, begin, end)
            got_k, got_v = radix_sort(P, which, keys, begin, end)
            assert np.array_equal(got_k, keys[perm]), (which, n, kind, begin, end)
            if got_v is not None:
                assert np.array_equal(got_v, perm.astype(np.uint32)), (which, n, kind, begin, end, "values / stability")
    P.check_scratch()


# =====================================================================================================================================
# one kernel per pass: nh_onesweep_u64_u32_two_fields
# =====================================================================================================================================
def _two_fields(lo, hi):
    return lo.astype(np.uint64) | (hi.astype(np.uint64) << np.uint64(32))


def _field_keys(kind, n, bits, rng):
    top = 1 << bits
    if kind == "random":
        return _two_fields(rng.integers(0, top, size=n, dtype=np.uint64), rng.integers(0, top, size=n, dtype=np.uint64))
    if kind == "few":                      # sixteen distinct keys with both fields' extremes among them: long runs of equal keys (stability)
        lo = rng.integers(0, top, size=16, dtype=np.uint64)
        hi = rng.integers(0, top, size=16, dtype=np.uint64)
        lo[0], hi[0], lo[1], hi[1] = top - 1, top - 1, 0, 0
        pick = rng.integers(0, 16, size=n)
        return _two_fields(lo[pick], hi[pick])
    if kind == "reversed":
        k = _field_keys("random", n, bits, rng)
        return k[_field_perm(k, bits)][::-1].copy()
    raise ValueError(kind)


def _field_perm(keys, bits):
    """Stable order by (high field, low field) of keys whose fields are `bits` wide, at bit 0 and at bit 32."""
    lo, hi = keys & np.uint64(0xFFFFFFFF), keys >> np.uint64(32)
    assert (lo < (1 << bits)).all() and (hi < (1 << bits)).all(), "keys outside their fields are a contract violation, not a case"
    return np.argsort((hi << np.uint64(bits)) | lo if bits < 32 else keys, kind="stable")


# The two helpers below restate the launch arithmetic of onesweep_impl (nh_util.hip) and must be kept in step with it by hand.  They only assert that a
# case reaches the path it is meant for (one tile per workgroup, or several); no expected output depends on them.
def _os_grid(capacity, expected, resident):
    """onesweep_impl's launch: one workgroup per expected tile (+ 12 %, + 2), at most one per tile of the capacity (+ 1) and what is resident."""
    cap_tiles = (capacity + OS_TILE - 1) // OS_TILE + 1
    want = min((expected + expected // 8 + OS_TILE - 1) // OS_TILE + 2 if expected else cap_tiles, cap_tiles)
    return min(want, resident)


def _os_tiles_per_workgroup(n, capacity, expected, resident):
    ntiles = (n + OS_TILE - 1) // OS_TILE
    return -(-ntiles // _os_grid(capacity, expected, resident))


def onesweep(P, keys, bits, capacity=None, expected=0, repeat=1):
    """nh_onesweep_u64_u32_two_fields on buffers of `capacity` (+ PAD) entries, `repeat` times from the same input on the same scratch; returns the
    (keys, values) of every run."""
    n = len(keys)
    capacity = n + PAD if capacity is None else capacity
    assert n <= capacity
    cap = capacity + PAD
    vals = np.arange(n, dtype=np.uint32)
    passes = len(range(0, 2 * bits, 8))
    runs = []
    for _ in range(repeat):
        count = Word(n)
        ka, kb = _dev(_padded(keys, cap)), _dev(_filled(cap, np.uint64))
        va, vb = _dev(_padded(vals, cap)), _dev(_filled(cap, np.uint32))
        in_b = P.S.nhp_onesweep_u64_u32_two_fields(P.ctx, _ptr(ka), _ptr(kb), _ptr(va), _ptr(vb), count.ptr, capacity, expected, _ptr(P.scratch), bits)
        P.sync()
        assert in_b == (passes & 1), "the return value names the buffer of the last pass"
        assert count.value() == n
        for t, dt, s in ((ka, np.uint64, S64), (kb, np.uint64, S64), (va, np.uint32, S32), (vb, np.uint32, S32)):
            assert (_host(t, dt)[n:] == s).all(), "something behind the count was written"
        runs.append((_host(kb if in_b else ka, np.uint64)[:n].copy(), _host(vb if in_b else va, np.uint32)[:n].copy()))
    return runs


def _check_onesweep(P, keys, bits, **kw):
    perm = _field_perm(keys, bits)
    for got_k, got_v in onesweep(P, keys, bits, **kw):
        assert np.array_equal(got_k, keys[perm]), (len(keys), bits, kw)
        assert np.array_equal(got_v, perm.astype(np.uint32)), (len(keys), bits, kw, "values / stability")


OS_M1_COUNTS = (0, 1, OS_TILE - 1, OS_TILE, OS_TILE + 1,
                OS_GROUP * OS_TILE - 1, OS_GROUP * OS_TILE, OS_GROUP * OS_TILE + 1,        # 65536 keys fill one publish group: the next key opens a second
                4 * OS_GROUP * OS_TILE + OS_GROUP * OS_TILE // 2 + 11)                      # 294 923: four full groups and half a fifth, its last tile partial
# field widths whose passes differ in kind: 5 (one glued digit, three bits of the high field), 12 (glued 4 + 4 in the second pass), 20 (the tags'
# default: five passes, the third glued), 32 (eight plain bytes)
OS_WIDTHS = (5, 12, 20, 32)


@pytest.mark.parametrize("bits", OS_WIDTHS)
def test_onesweep_one_tile_per_workgroup(P, bits):
    rng = np.random.default_rng(2000 + bits)
    resident = P.resident()
    for n in OS_M1_COUNTS:
        assert _os_tiles_per_workgroup(n, n + PAD, 0, resident) <= 1, "this device keeps too few workgroups resident for the m = 1 path at this count"
        for kind in ("random", "few") + (("reversed",) if n > OS_TILE else ()):
            _check_onesweep(P, _field_keys(kind, n, bits, rng), bits)
    P.check_scratch()


OS_THREE_WORKGROUPS = 3                    # the grid `expected` = 1 asks for: (1 + 0 + OS_TILE - 1) / OS_TILE + 2
OS_MANY_COUNTS = (OS_THREE_WORKGROUPS * OS_TILE,              # 6144: three tiles, still one each
                  OS_THREE_WORKGROUPS * OS_TILE + 1,          # 6145: four tiles, two per workgroup, two workgroups: the third draws a ticket behind the last chunk
                  146 * OS_TILE + 995)                        # 300 003: 147 tiles, 49 per workgroup, the last one partial


@pytest.mark.parametrize("bits", OS_WIDTHS)
def test_onesweep_several_tiles_per_workgroup(P, bits):
    """The path a contact set takes when it jumps past its estimate: `expected` = 1 under a capacity far above the count makes the launch three workgroups."""
    rng = np.random.default_rng(2100 + bits)
    capacity = 400_000
    assert _os_grid(capacity, 1, P.resident()) == OS_THREE_WORKGROUPS
    for n, m in zip(OS_MANY_COUNTS, (1, 2, 49)):
        assert _os_tiles_per_workgroup(n, capacity, 1, P.resident()) == m
        for kind in ("random", "few"):
            _check_onesweep(P, _field_keys(kind, n, bits, rng), bits, capacity=capacity, expected=1)
    P.check_scratch()


def test_onesweep_every_field_width(P):
    """Widths 1 .. 32: the glued digit of two_field_shifts takes 1 .. 7 bits of the low field, or none; one tile per workgroup and two."""
    rng = np.random.default_rng(2200)
    for bits in range(1, 33):
        for kind in ("random", "few"):
            _check_onesweep(P, _field_keys(kind, 3 * OS_TILE + 5, bits, rng), bits)
            _check_onesweep(P, _field_keys(kind, OS_MANY_COUNTS[1], bits, rng), bits, capacity=400_000, expected=1)
    P.check_scratch()


@pytest.mark.parametrize("n,capacity,expected", [(OS_GROUP * OS_TILE + 1, None, 0), (OS_MANY_COUNTS[1], 400_000, 1), (0, OS_TILE, 0)],
                         ids=["one_tile_each", "two_tiles_each", "empty"])
def test_onesweep_twice_on_one_scratch(P, n, capacity, expected):
    """The control block (counts, group sums, histograms, tickets) is cleared per sort: a second sort on the same scratch gives the same bytes."""
    keys = _field_keys("random", n, 20, np.random.default_rng(2300 + n))
    perm = _field_perm(keys, 20)
    (k1, v1), (k2, v2) = onesweep(P, keys, 20, capacity=capacity, expected=expected, repeat=2)
    assert np.array_equal(k1, keys[perm]) and np.array_equal(v1, perm.astype(np.uint32))
    assert np.array_equal(k2, k1) and np.array_equal(v2, v1)
    P.check_scratch()


# =====================================================================================================================================
# seeded bucket sort: nh_bucket_sort_u64_u32, nh_bucket_sort_seed
# =====================================================================================================================================
def _unpack_fields(packed, bits):
    return _two_fields(packed & np.uint64((1 << bits) - 1), packed >> np.uint64(bits))


def _unique_pool(count, bits, rng):
    """`count` distinct keys of two `bits`-wide fields, ascending (one record per collider pair: the sort's contract)."""
    space = 1 << (2 * bits)
    assert space >= 4 * count
    pool = np.unique(rng.integers(0, space, size=2 * count + 1024, dtype=np.uint64))
    assert len(pool) >= count
    return _unpack_fields(np.sort(rng.permutation(pool)[:count]), bits)


class Bucket:
    """One harness of the shim (device state, splitters, counts, starts, place) on one context, and the rounds nh_collide would run on it."""

    def __init__(self, P, ctx, capacity, bits, target):
        self.P, self.ctx, self.capacity, self.bits, self.target = P, ctx, capacity, bits, target
        self.h = C.c_void_p(P.S.nhp_bucket_create(ctx, capacity))
        assert self.h.value
        self.entries = int(P.S.nhp_bucket_entries(self.h))
        assert self.entries == capacity // target + 3          # nh_bucket_sort_max_buckets + 1
        self.cap = capacity + PAD

    def close(self):
        self.P.S.nhp_bucket_destroy(self.h)

    def state(self):
        out = (C.c_uint32 * 5)()
        assert self.P.S.nhp_bucket_read(self.h, out) == 0
        return dict(zip(("records", "sort_buckets", "sort_buckets_next", "sort_reuses", "sort_valid"), (int(x) for x in out)))

    def tables(self):
        s, c, t = np.zeros(self.entries, np.uint64), np.zeros(self.entries, np.uint32), np.zeros(self.entries, np.uint32)
        assert self.P.S.nhp_bucket_read_tables(self.h, s.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p)) == 0
        return s, c, t

    def check_announced(self, sorted_keys):
        """What a sort (or the seed) leaves for the next round: the bucket count, and every target-th sorted key as a splitter."""
        n = len(sorted_keys)
        nb = max(1, -(-n // self.target))
        assert self.state()["sort_buckets_next"] == nb
        splitters, counts, _ = self.tables()
        assert np.array_equal(splitters[:nb - 1], sorted_keys[self.target::self.target][:nb - 1]), "splitters are every target-th sorted key"
        assert len(sorted_keys[self.target::self.target]) == nb - 1
        assert (counts == 0).all(), "the bucket counters are left zero for the next round"

    def seed(self, keys):
        """No history: the radix passes sort, nh_bucket_sort_seed takes the splitters from their result."""
        P, n = self.P, len(keys)
        assert n <= self.capacity
        assert P.S.nhp_bucket_set_records(self.h, n) == 0
        d_count = C.c_void_p(P.S.nhp_bucket_records_ptr(self.h))
        ka, kb = _dev(_padded(keys, self.cap)), _dev(_filled(self.cap, np.uint64))
        va, vb = _dev(_padded(np.arange(n, dtype=np.uint32), self.cap)), _dev(_filled(self.cap, np.uint32))
        in_b = P.S.nhp_onesweep_u64_u32_two_fields(self.ctx, _ptr(ka), _ptr(kb), _ptr(va), _ptr(vb), d_count, self.capacity, 0, _ptr(P.scratch), self.bits)
        srt = kb if in_b else ka
        P.S.nhp_bucket_seed(self.h, _ptr(srt))
        P.sync(self.ctx)
        expect = np.sort(keys)
        assert np.array_equal(_host(srt, np.uint64)[:n], expect)
        self.check_announced(expect)

    def round(self, keys):
        """One step's sort of `keys` (unique, any order) on top of what the last round announced."""
        P, n = self.P, len(keys)
        assert n <= self.capacity and len(np.unique(keys)) == n
        before = self.state()
        assert P.S.nhp_bucket_begin_round(self.h, n, 0, 1, before["records"]) == 0
        vals = np.arange(n, dtype=np.uint32)
        ka, va = _dev(_padded(keys, self.cap)), _dev(_padded(vals, self.cap))
        kb, vb = _dev(_filled(self.cap, np.uint64)), _dev(_filled(self.cap, np.uint32))
        ko, vo = _dev(_filled(self.cap, np.uint64)), _dev(_filled(self.cap, np.uint32))
        P.S.nhp_bucket_sort(self.h, _ptr(ka), _ptr(kb), _ptr(va), _ptr(vb), self.bits, _ptr(ko), _ptr(vo))
        P.sync(self.ctx)
        order = np.argsort(keys, kind="stable")
        hk, hv = _host(ko, np.uint64), _host(vo, np.uint32)
        assert np.array_equal(hk[:n], keys[order]), (n, "keys")
        assert np.array_equal(hv[:n], order.astype(np.uint32)), (n, "values")
        assert (hk[n:] == S64).all() and (hv[n:] == S32).all(), "the result was written behind the count"
        assert (_host(kb, np.uint64)[n:] == S64).all() and (_host(vb, np.uint32)[n:] == S32).all(), "the scratch copy was written behind the count"
        assert np.array_equal(_host(ka, np.uint64), _padded(keys, self.cap)) and np.array_equal(_host(va, np.uint32), _padded(vals, self.cap)), "the input is left as it is"
        after = self.state()
        assert after["sort_buckets"] == before["sort_buckets_next"] and after["sort_reuses"] == before["sort_reuses"] and after["records"] == n
        self.check_announced(keys[order])


# name -> (options, records of the seeding set): buckets of ~1024 in LDS / every bucket through global memory, one pass per byte / 5000 buckets of two
# keys, more splitters than bk_count's LDS holds (the search finishes in global memory) and more buckets than bk_sort's grid (a workgroup takes several)
BUCKET_KNOBS = {"defaults": ({}, 40_000), "tile_1": ({"bucket_tile": 1}, 6_000), "tile_37": ({"bucket_tile": 37}, 6_000), "target_2": ({"bucket_target": 2}, 10_000)}
BUCKET_SECOND_SETS = ("same", "replaced", "disjoint", "half", "double", "empty")


@pytest.mark.parametrize("second", BUCKET_SECOND_SETS)
@pytest.mark.parametrize("knobs", list(BUCKET_KNOBS))
def test_seeded_bucket_sort(P, knobs, second):
    options, n = BUCKET_KNOBS[knobs]
    target = options.get("bucket_target", BK_TARGET)
    if knobs == "target_2":
        assert n // target - 1 > BK_LDS_SPLITTERS and n // target > 4096
    bits = 20
    rng = np.random.default_rng(3000 + n + len(second))
    pool = _unique_pool(4 * n, bits, rng)                    # ascending
    b = Bucket(P, P.context(**options), 2 * n + 64, bits, target)
    try:
        if second == "disjoint":
            # the seed takes the middle of the pool; the second set lies wholly below and wholly above it: first bucket or last bucket, nothing between
            first, rest = pool[n:2 * n], np.concatenate([pool[:n // 2], pool[-(n - n // 2):]])
            spare = pool[2 * n:3 * n]
        else:
            picks = rng.permutation(4 * n)
            first, spare = pool[picks[:n]], pool[picks[n:]]
            if second == "same":
                rest = first
            elif second == "replaced":
                rest = first.copy()
                rest[rng.permutation(n)[:n // 100]] = spare[:n // 100]
                spare = spare[n // 100:]
            elif second == "half":
                rest = first[rng.permutation(n)[:n // 2]]
            elif second == "double":
                rest, spare = np.concatenate([first, spare[:n]]), spare[n:]
            elif second == "empty":
                rest = first[:0]
        b.seed(rng.permutation(first))
        b.round(rng.permutation(rest))
        if second == "empty":
            assert b.state()["sort_buckets_next"] == 1
            rest = first
            b.round(rng.permutation(rest))                 # one bucket, no splitter: everything through global memory
        # a third round on top: its buckets come from the splitters the second round's sort wrote
        third = rest.copy()
        k = max(1, len(third) // 100)
        third[rng.permutation(len(third))[:k]] = spare[:k]
        b.round(rng.permutation(third))
    finally:
        b.close()
    P.check_scratch()


@pytest.mark.parametrize("bits", (9, 32))
def test_seeded_bucket_sort_field_widths(P, bits):
    """Fields narrower and wider than the default: bk_sort packs the two fields side by side, sorts the bits that differ inside a bucket, unpacks."""
    n = 30_000
    rng = np.random.default_rng(3100 + bits)
    pool = rng.permutation(_unique_pool(2 * n, bits, rng))
    for options in ({}, {"bucket_tile": 37}):
        b = Bucket(P, P.context(**options), n + 64, bits, BK_TARGET)
        try:
            b.seed(pool[:n])
            mixed = pool[:n].copy()
            mixed[: n // 50] = pool[n:n + n // 50]
            b.round(rng.permutation(mixed))
            b.round(rng.permutation(pool[:n]))
        finally:
            b.close()


def test_seeded_bucket_sort_reuses_a_kept_order(P):
    """sort_valid = 1, keys_changed = 0, records == records_kept: the four kernels leave at once, the outputs keep their bytes, sort_reuses counts one."""
    n, bits = 20_000, 20
    rng = np.random.default_rng(3200)
    keys = rng.permutation(_unique_pool(n, bits, rng))
    b = Bucket(P, P.ctx, n + 64, bits, BK_TARGET)
    try:
        b.seed(keys)
        b.round(keys)
        before = b.state()
        splitters_before, _, starts_before = b.tables()
        assert P.S.nhp_bucket_begin_round(b.h, n, 1, 0, n) == 0
        other = rng.permutation(keys)                      # not what was sorted: a sort that ran would show
        ka, va = _dev(_padded(other, b.cap)), _dev(_padded(np.arange(n, dtype=np.uint32), b.cap))
        kb, vb = _dev(_filled(b.cap, np.uint64)), _dev(_filled(b.cap, np.uint32))
        ko, vo = _dev(_filled(b.cap, np.uint64)), _dev(_filled(b.cap, np.uint32))
        P.S.nhp_bucket_sort(b.h, _ptr(ka), _ptr(kb), _ptr(va), _ptr(vb), bits, _ptr(ko), _ptr(vo))
        P.sync()
        for t, dt, s in ((kb, np.uint64, S64), (ko, np.uint64, S64), (vb, np.uint32, S32), (vo, np.uint32, S32)):
            assert (_host(t, dt) == s).all(), "a re-used order leaves every output byte alone"
        after = b.state()
        assert after["sort_reuses"] == before["sort_reuses"] + 1
        assert after["sort_buckets_next"] == before["sort_buckets_next"] and after["sort_valid"] == 1
        splitters, counts, starts = b.tables()
        assert np.array_equal(splitters, splitters_before) and np.array_equal(starts, starts_before) and (counts == 0).all()
        # ... and with one of the three conditions gone the sort runs again
        b.round(other)
        assert b.state()["sort_reuses"] == after["sort_reuses"]
    finally:
        b.close()


# =====================================================================================================================================
# exclusive scans: nh_scan_u32, nh_scan2_u32
# =====================================================================================================================================
SCAN_LENGTHS = (0, 1, SC_IPT - 1, SC_IPT, SC_IPT + 1, RS_TILE - 1, RS_TILE, RS_TILE + 1, SC_TILE - 1, SC_TILE, SC_TILE + 1,
                ONE_TILE_PER_CHUNK, ONE_TILE_PER_CHUNK + 1,          # chunks of 256 items become chunks of 512
                NH_SORT_GRID * SC_TILE, NH_SORT_GRID * SC_TILE + 1,  # 1 048 576: every chunk is exactly one workgroup scan; one more item: two, the second partial
                1_200_003)                                           # chunks of 2560: a full scan tile and a quarter, the last chunks short
SCAN_INPUTS = ("flags", "u16", "wrap")


def _scan_input(kind, n, rng):
    if kind == "flags":
        return rng.integers(0, 2, size=n, dtype=np.uint64).astype(np.uint32)
    if kind == "u16":
        return rng.integers(0, 1 << 16, size=n, dtype=np.uint64).astype(np.uint32)
    if kind == "wrap":                     # two items already pass 2^32
        return (rng.integers(0, 1 << 31, size=n, dtype=np.uint64) | np.uint64(1 << 31)).astype(np.uint32)
    raise ValueError(kind)


def _exclusive(a):
    """(exclusive scan, total) modulo 2^32, computed in 64 bits: nh_overlap's overflow marker relies on exactly this wrap."""
    c = np.cumsum(a.astype(np.uint64), dtype=np.uint64)
    ex = np.concatenate([np.zeros(1, np.uint64), c[:-1]]) if len(a) else c
    return (ex & np.uint64(0xFFFFFFFF)).astype(np.uint32), int(c[-1]) & 0xFFFFFFFF if len(a) else 0


def _splits(length):
    """(device count, extra) pairs of one length: all from the device, all from `extra` (nh_overlap: a zero count + count + 1), and two mixtures."""
    s = {(length, 0), (0, length), (length // 2, length - length // 2)}
    if length:
        s.add((length - 1, 1))
    return sorted(s)


def scan(P, data, count, extra, in_place, two=False, shift=0, total=True, enable=None):
    """One nh_scan_u32 (data: one array) or nh_scan2_u32 (two=True: data is a pair) call over count + extra items.  Buffers start `shift` words into
    their allocation (1: the 4-byte alignment nh_overlap admits for `offsets`) and end in PAD sentinel words.  Checks what must not move and returns
    [(output[0 .. length), total or None), ...]."""
    arrays = list(data) if two else [data]
    length = count + extra
    assert all(len(a) == length for a in arrays)
    d_count = Word(count)
    ins = []
    for a in arrays:                        # the words in front of a shifted buffer hold the sentinel as well
        h = _filled(shift + length + PAD, np.uint32)
        h[shift:shift + length] = a
        ins.append(_dev(h))
    outs = ins if in_place else [_dev(_filled(shift + length + PAD, np.uint32)) for _ in arrays]
    totals = [Word() if total else None for _ in arrays]
    tp = [w.ptr if w else None for w in totals]
    en = None if enable is None else Word(enable)
    if two:
        assert enable is None
        P.S.nhp_scan2_u32(P.ctx, _ptr(ins[0], shift), _ptr(outs[0], shift), tp[0], _ptr(ins[1], shift), _ptr(outs[1], shift), tp[1], d_count.ptr, extra, _ptr(P.scan_tmp))
    else:
        P.S.nhp_scan_u32(P.ctx, _ptr(ins[0], shift), _ptr(outs[0], shift), d_count.ptr, extra, _ptr(P.scan_tmp), tp[0], en.ptr if en else None)
    P.sync()
    assert d_count.value() == count
    if en:
        assert en.value() == enable
    res = []
    for a, ti, to, w in zip(arrays, ins, outs, totals):
        ho = _host(to, np.uint32)
        assert (ho[:shift] == S32).all() and (ho[shift + length:] == S32).all(), "words around the scanned range were written"
        if not in_place:
            hi = _host(ti, np.uint32)
            assert np.array_equal(hi[shift:shift + length], a) and (hi[:shift] == S32).all() and (hi[shift + length:] == S32).all(), "the input of an out-of-place scan was written"
        res.append((ho[shift:shift + length].copy(), w.value() if w else None))
    return res


@pytest.mark.parametrize("in_place", (False, True), ids=("out_of_place", "in_place"))
@pytest.mark.parametrize("two", (False, True), ids=("scan", "scan2"))
def test_scan_is_the_exclusive_prefix_sum_modulo_2_32(P, two, in_place):
    rng = np.random.default_rng(4000 + 2 * two + in_place)
    for length in SCAN_LENGTHS:
        for k, kind in enumerate(SCAN_INPUTS):
            a = _scan_input(kind, length, rng)
            # the two-array form: different data in the two, so that a wrong carry in one is not covered by the other
            b = _scan_input(SCAN_INPUTS[(k + 1) % 3], length, rng)
            ea, eb = _exclusive(a), _exclusive(b)
            if kind == "wrap" and length >= 2:
                assert int(a.astype(np.uint64).sum()) >= 1 << 32
            for count, extra in _splits(length):
                got = scan(P, (a, b) if two else a, count, extra, in_place, two=two)
                for (out, tot), (eo, et), name in zip(got, (ea, eb), "ab"):
                    assert np.array_equal(out, eo), (length, kind, count, extra, name)
                    assert tot == et, (length, kind, count, extra, name, "total")
    P.check_scratch()


@pytest.mark.parametrize("two", (False, True), ids=("scan", "scan2"))
def test_scan_on_four_byte_aligned_pointers(P, two):
    """`offsets` of nh_overlap / nh_penetration / the all-hits casts needs 4-byte alignment only, and is scanned in place: a slice of a larger buffer
    that starts one word in (and two, and three), in place and out of place."""
    rng = np.random.default_rng(4100 + two)
    for length in (1, SC_IPT + 1, RS_TILE + 1, SC_TILE, SC_TILE + 1, ONE_TILE_PER_CHUNK + 1, NH_SORT_GRID * SC_TILE + 1):
        a, b = _scan_input("u16", length, rng), _scan_input("wrap", length, rng)
        for shift in (1, 2, 3):
            for in_place in (True, False):
                got = scan(P, (a, b) if two else a, 0, length, in_place, two=two, shift=shift)
                for (out, tot), src in zip(got, (a, b)):
                    eo, et = _exclusive(src)
                    assert np.array_equal(out, eo) and tot == et, (length, shift, in_place)
    P.check_scratch()


@pytest.mark.parametrize("two", (False, True), ids=("scan", "scan2"))
def test_scan_without_a_total(P, two):
    rng = np.random.default_rng(4200 + two)
    for length in (0, 1, RS_TILE + 1, ONE_TILE_PER_CHUNK + 1, NH_SORT_GRID * SC_TILE + 1):
        a, b = _scan_input("wrap", length, rng), _scan_input("u16", length, rng)
        for in_place in (True, False):
            got = scan(P, (a, b) if two else a, length, 0, in_place, two=two, total=False)
            for (out, tot), src in zip(got, (a, b)):
                assert tot is None and np.array_equal(out, _exclusive(src)[0]), (length, in_place)
    P.check_scratch()


def test_scan_switched_off_and_on_from_the_device(P):
    """*d_enable == 0: no output word changes and the total is reported as 0; *d_enable == 1: the scan as usual."""
    rng = np.random.default_rng(4300)
    for length in (0, 1, SC_TILE + 1, ONE_TILE_PER_CHUNK + 1, NH_SORT_GRID * SC_TILE + 1):
        a = _scan_input("wrap", length, rng)
        eo, et = _exclusive(a)
        for in_place in (True, False):
            for count, extra in _splits(length)[:2]:
                (out, tot), = scan(P, a, count, extra, in_place, enable=0)
                assert tot == 0
                assert np.array_equal(out, a if in_place else np.full(length, S32, np.uint32)), (length, in_place, "a switched-off scan wrote its output")
                (out, tot), = scan(P, a, count, extra, in_place, enable=1)
                assert np.array_equal(out, eo) and tot == et, (length, in_place)
                (out, tot), = scan(P, a, count, extra, in_place, enable=0, total=False)
                assert tot is None and np.array_equal(out, a if in_place else np.full(length, S32, np.uint32))
    P.check_scratch()
