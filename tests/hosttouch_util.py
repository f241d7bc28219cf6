"""ctypes access to the touched movers' oracle of tests/hostoracle/hosttouch.cpp (built by tests/hostlib.py): nh_move_touched, nh_boxmove_touched,
nh_walk_touched and nh_boxwalk_touched by brute force over all colliders -- hostmover.cpp's loops, which also write one nh_Touch per cast that found a
collider -- the oracle of the GPU's k_q_move<., ., true> and k_q_walk<., ., true>; and what the tests of both sides share: which slots a call wrote, the
byte comparison of those, and the cast records of identity T2 (include/nudge_hip.h, "nh_move_touched").

CAPSULE and BOX are the two movers in the manner of hostmover_util, with the same members."""
import ctypes as C

import numpy as np

import hostcast_util as CAST
import hostlib as H
import hostmover_util as MV
from nudge_amd import engine as E

_V, _U = C.c_void_p, C.c_uint32
lib = H.oracle({
    "ht_move": ([_U, _V, _U, _U, _V, _U, _V, _U, _V, _V, _V, _V, _U, _U], None),
    "ht_walk": ([_U, _V, _U, _U, _V, _U, _V, _U, _V, _V, _V, _V, _U, _U], None),
})
NONE = 0xFFFFFFFF
MOVE_K, WALK_K = E.NH_MOVE_MAX_SLIDES + 1, E.NH_WALK_MAX_CASTS          # the most touches a move and a walk can have


def written(counts, k):
    """(n, k) bool: the slots a call with this k wrote -- slot j of record i where j < min(counts[i], k)."""
    return np.arange(k)[None, :] < np.minimum(np.asarray(counts).astype(np.int64), k)[:, None]


def same_touches(got, got_counts, ref, ref_counts, what):
    """The counts are equal, and the written slots of `got` ((n, k) E.TOUCH) hold the bytes of the same slots of `ref` ((n, k') E.TOUCH, k' >= k)."""
    assert np.array_equal(np.asarray(got_counts).astype(np.int64), np.asarray(ref_counts).astype(np.int64)), \
        f"{what}: counts differ, first at {int(np.argmax(np.asarray(got_counts) != np.asarray(ref_counts)))}"
    k = got.shape[1]
    assert ref.shape[1] >= k
    w = written(got_counts, k)
    a, b = got.view(np.uint8).reshape(len(got), k, 64), np.ascontiguousarray(ref[:, :k]).view(np.uint8).reshape(len(got), k, 64)
    bad = (a != b).any(axis=2) & w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {int(w.sum())} touches differ, first at {tuple(int(x) for x in np.argwhere(bad)[0])}: " \
                          f"{got[tuple(np.argwhere(bad)[0])]} != {ref[tuple(np.argwhere(bad)[0])]}"


def _hit_bytes(h):
    return np.ascontiguousarray(h).view(np.uint8).reshape(-1, 32)


def check_move_identities(results, counts, touches, what):
    """Identity T3 on a call's bytes at k = MOVE_K: counts == slides + (START_OVERLAP ? 1 : 0); touch j has cast == j and phase SLIDE; where last_hit
    is a collider the last touch's hit is last_hit."""
    counts = counts.astype(np.int64)
    assert touches.shape[1] == MOVE_K and (counts <= MOVE_K).all(), what
    start = (results["flags"] & E.NH_MOVE_START_OVERLAP) != 0
    start &= results["flags"] != E.NH_MOVE_INVALID
    assert np.array_equal(counts, results["slides"].astype(np.int64) + start), what
    w = written(counts, MOVE_K)
    assert (touches["cast"][w] == np.broadcast_to(np.arange(MOVE_K), w.shape)[w]).all() and (touches["phase"][w] == E.NH_TOUCH_SLIDE).all(), what
    assert (touches["hit"]["shape"][w] != NONE).all() and (touches["hit"]["t"][w] >= 0).all() and (touches["hit"]["t"][w] <= 1).all(), what
    held = np.nonzero((results["last_hit"]["shape"] != NONE) & (results["flags"] != E.NH_MOVE_INVALID))[0]
    assert (counts[held] >= 1).all(), what
    assert (_hit_bytes(touches["hit"][held, counts[held] - 1]) == _hit_bytes(results["last_hit"][held])).all(), what
    # a last_hit that is a miss: the last cast touched nothing, and every touch before it was a taken hit
    return int(w.sum())


def check_walk_identities(results, counts, touches, what):
    """Identity T4 on a call's bytes at k = WALK_K: counts <= casts; `cast` strictly ascending and < casts; `phase` never decreasing; the touches
    with t > 0 of the kept slide (FORWARD if STEPPED, else SLIDE) number `slides`; with STEPPED the last DOWN touch's hit is `ground`; without it,
    where `ground` is a collider, the PROBE touch's hit is `ground`."""
    counts = counts.astype(np.int64)
    n, k = touches.shape
    assert k == WALK_K and (counts <= results["casts"]).all(), what
    invalid = results["flags"] == E.NH_WALK_INVALID
    assert (counts[invalid] == 0).all(), what
    w = written(counts, k)
    cast, phase = touches["cast"].astype(np.int64), touches["phase"].astype(np.int64)
    pair = w[:, 1:]                                                        # slot j + 1 is written: so is slot j
    assert (cast[:, 1:][pair] > cast[:, :-1][pair]).all() and (phase[:, 1:][pair] >= phase[:, :-1][pair]).all(), what
    assert (cast[w] < np.broadcast_to(results["casts"].astype(np.int64)[:, None], w.shape)[w]).all() and (phase[w] <= E.NH_TOUCH_PROBE).all(), what
    stepped = ((results["flags"] & E.NH_WALK_STEPPED) != 0) & ~invalid
    kept = np.where(stepped, E.NH_TOUCH_FORWARD, E.NH_TOUCH_SLIDE)
    taken = (w & (phase == kept[:, None]) & (touches["hit"]["t"] > 0)).sum(axis=1)
    assert np.array_equal(taken, results["slides"].astype(np.int64)), (what, int(np.argmax(taken != results["slides"])))
    for i in np.nonzero(stepped)[0]:
        down = np.nonzero(w[i] & (phase[i] == E.NH_TOUCH_DOWN))[0]
        assert len(down) and touches["hit"][i, down[-1]].tobytes() == results["ground"][i].tobytes(), (what, i)
    for i in np.nonzero(~stepped & ~invalid & (results["ground"]["shape"] != NONE))[0]:
        probe = np.nonzero(w[i] & (phase[i] == E.NH_TOUCH_PROBE))[0]
        assert len(probe) == 1 and touches["hit"][i, probe[0]].tobytes() == results["ground"][i].tobytes(), (what, i)
    return int(w.sum())


class Toucher:
    """One shape's touched movers: `mover` (hostmover_util.CAPSULE or BOX: the records and the plain oracle) and `cast` (hostcast_util's shape)."""

    def __init__(self, mover, cast):
        self.mover, self.cast = mover, cast
        self.shape, self.MOVE, self.WALK, self.CAST = mover.shape, mover.MOVE, mover.WALK, mover.CAST

    def _run(self, fn, dtype, result, rec, nbox, records, k, words, masks, mask, threads, touches):
        records = np.ascontiguousarray(records, dtype=dtype)
        rec = np.ascontiguousarray(rec, dtype=H.REC)
        n = len(records)
        out = np.zeros(n, dtype=result)
        counts = np.zeros(n, dtype=np.uint32)
        if touches is None:
            touches = np.zeros((n, k), dtype=E.TOUCH)
        assert touches.dtype == E.TOUCH and touches.shape == (n, k) and touches.flags.c_contiguous
        (words, pw), (masks, pm) = MV._opt(words, len(rec)), MV._opt(masks, n)
        fn(self.shape, H.p(rec), len(rec), nbox, H.p(records), n, H.p(out), k, H.p(counts), H.p(touches), pw, pm, int(mask) & NONE, H.threads(threads))
        return out, counts, touches

    def move(self, rec, nbox, m, k=MOVE_K, words=None, masks=None, mask=NONE, threads=None, touches=None):
        """(nh_MoveResult records, counts (uint32), touches ((n, k) E.TOUCH)) of the moves `m` (MOVE) by brute force over `rec`; `words`, `masks` and
        `mask` as hostmover_util's move().  `touches`: written in place where given -- the slots at or behind a move's count are left as they are."""
        return self._run(lib().ht_move, self.MOVE, E.MOVE_RESULT, rec, nbox, m, k, words, masks, mask, threads, touches)

    def walk(self, rec, nbox, w, k=WALK_K, words=None, masks=None, mask=NONE, threads=None, touches=None):
        """(nh_WalkResult records, counts (uint32), touches ((n, k) E.TOUCH)) of the walks `w` (WALK) by brute force over `rec`, likewise."""
        return self._run(lib().ht_walk, self.WALK, E.WALK_RESULT, rec, nbox, w, k, words, masks, mask, threads, touches)

    def touch_casts(self, records, counts, touches):
        """Identity T2: (the shape's cast records { origin, 1, direction, ignore_body, rotation, the shape } of every written touch in record order,
        the record index of each, the nh_RayHit of each).  `records`: the moves or the walks."""
        i, j = np.nonzero(written(counts, touches.shape[1]))
        c = np.zeros(len(i), dtype=self.CAST)
        c["origin"], c["max_t"], c["direction"] = touches["origin"][i, j], 1.0, touches["direction"][i, j]
        for name in ("ignore_body", "rotation") + self.mover.size:
            c[name] = records[name][i]
        return c, i, np.ascontiguousarray(touches["hit"][i, j])


CAPSULE, BOX = Toucher(MV.CAPSULE, CAST.CAPSULE), Toucher(MV.BOX, CAST.BOX)
