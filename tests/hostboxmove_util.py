"""ctypes access to the box-move oracle of tests/hostoracle/hostboxmove.cpp (built by tests/hostlib.py): nh_boxmove by brute force over all colliders with
the state machine of nudge_amd/csrc/nh_query.h ("move") and the device's bits, the oracle of the GPU's k_q_move<nh_QBox, .>; and one step of that state
machine alone, for the REPLAY identity."""
import ctypes as C
import numpy as np

import hostlib as H
from hostlib import records      # noqa: F401
from hostmove_util import STATE, NONE, IDENTITY
from nudge_amd import engine as E

_SIG = {
    "hbm_move": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32], None),
    "hbm_begin": ([C.c_void_p, C.c_uint32, C.c_void_p], None),
    "hbm_advance": ([C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p], None),
}
lib = H.oracle(_SIG)


def moves(origins, displacements, half_extents, rotations=None, skin=0.01, max_slides=4, ignore_body=NONE):
    """nh_BoxMove records (E.BOX_MOVE) from arrays or numbers, as World.boxmove packs them."""
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    m = np.zeros(len(o), dtype=E.BOX_MOVE)
    m["origin"], m["displacement"] = o, np.asarray(displacements, dtype=np.float32).reshape(-1, 3)
    m["skin"], m["max_slides"], m["ignore_body"] = skin, max_slides, ignore_body
    m["size"] = np.asarray(half_extents, dtype=np.float32).reshape(-1, 3)
    m["rotation"] = IDENTITY if rotations is None else np.asarray(rotations, dtype=np.float32).reshape(-1, 4)
    return m


def first_casts(m):
    """The nh_BoxCast records (E.BOX_CAST) of the moves' first casts: { origin, 1, displacement, ignore_body, rotation, size }."""
    c = np.zeros(len(m), dtype=E.BOX_CAST)
    c["origin"], c["max_t"], c["direction"], c["ignore_body"] = m["origin"], 1.0, m["displacement"], m["ignore_body"]
    c["rotation"], c["size"] = m["rotation"], m["size"]
    return c


def overlap_queries(m):
    """The NH_SHAPE_BOX nh_OverlapQuery records (E.OVERLAP_QUERY) of the boxes at the moves' origins, ignoring nothing."""
    q = np.zeros(len(m), dtype=E.OVERLAP_QUERY)
    q["center"], q["shape"], q["rotation"], q["size"], q["ignore_body"] = m["origin"], E.NH_SHAPE_BOX, m["rotation"], m["size"], NONE
    return q


def move(rec, nbox, m, words=None, masks=None, mask=NONE, threads=None, casts=False):
    """nh_MoveResult records (E.MOVE_RESULT) of the moves `m` (E.BOX_MOVE) by brute force over `rec`.  `words`: a layer word per collider, with `masks`
    (one per move) or `mask` (one for all) -- the masked world of the header; None: every collider is seen.  casts=True: (results, casts made per move)."""
    m = np.ascontiguousarray(m, dtype=E.BOX_MOVE)
    rec = np.ascontiguousarray(rec, dtype=H.REC)
    out = np.zeros(len(m), dtype=E.MOVE_RESULT)
    made = np.zeros(len(m), dtype=np.uint32)
    words = None if words is None else np.ascontiguousarray(words, dtype=np.uint32)
    masks = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint32)
    assert words is None or len(words) == len(rec)
    assert masks is None or len(masks) == len(m)
    lib().hbm_move(H.p(rec), len(rec), nbox, H.p(m), len(m), H.p(out), None if words is None else H.p(words), None if masks is None else H.p(masks),
                   int(mask) & NONE, H.p(made), H.threads(threads))
    return (out, made) if casts else out


def begin(m):
    """The states (hostmove_util.STATE) of the moves `m` before their first casts."""
    m = np.ascontiguousarray(m, dtype=E.BOX_MOVE)
    st = np.zeros(len(m), dtype=STATE)
    lib().hbm_begin(H.p(m), len(m), H.p(st))
    return st


def advance(m, st, hits):
    """nh_q_move_advance in place on every state of `st` that has not stopped, with the nh_RayHit records `hits` of the casts from st.p along st.v."""
    m = np.ascontiguousarray(m, dtype=E.BOX_MOVE)
    hits = np.ascontiguousarray(hits, dtype=E.RAY_HIT)
    assert st.dtype == STATE and st.flags.c_contiguous and len(st) == len(m) == len(hits)
    lib().hbm_advance(H.p(m), len(m), H.p(st), H.p(hits))
    return st


def state_casts(m, st):
    """The nh_BoxCast records of the next cast of every state: { p, 1, v, ... }."""
    c = first_casts(m)
    c["origin"], c["direction"] = st["p"], st["v"]
    return c


def replay(m, boxcast):
    """The REPLAY identity: the valid moves `m` run round by round from the host, boxcast(nh_BoxCast records) -> nh_RayHit records answering each round
    (the GPU's call, or the host's brute force).  Returns (nh_MoveResult records, rounds made)."""
    m = np.ascontiguousarray(m, dtype=E.BOX_MOVE)
    st = begin(m)
    last = np.zeros(len(m), dtype=E.RAY_HIT)
    last["t"], last["body"], last["collider"], last["shape"], last["tag"] = 1.0, NONE, NONE, NONE, NONE
    rounds = 0
    while (st["stopped"] == 0).any():
        live = st["stopped"] == 0
        hits = np.ascontiguousarray(boxcast(state_casts(m, st)), dtype=E.RAY_HIT)
        last[live] = hits[live]
        advance(m, st, hits)
        rounds += 1
    out = np.zeros(len(m), dtype=E.MOVE_RESULT)
    out["position"], out["remaining"], out["flags"], out["slides"], out["last_hit"] = st["p"], st["v"], st["flags"], st["slides"], last
    return out, rounds
