"""ctypes access to the move oracle of tests/hostoracle/hostmove.cpp (built by tests/hostlib.py): nh_move by brute force over all colliders with the
state machine of nudge_amd/csrc/nh_query.h ("move") and the device's bits, the oracle of the GPU's k_q_move; and one step of that state machine alone,
for the REPLAY identity."""
import ctypes as C
import numpy as np

import hostlib as H
from hostlib import records      # noqa: F401
from nudge_amd import engine as E

_SIG = {
    "hm_move": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32], None),
    "hm_begin": ([C.c_void_p, C.c_uint32, C.c_void_p], None),
    "hm_advance": ([C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p], None),
}
lib = H.oracle(_SIG)

# hostmove.cpp's MoveState
STATE = np.dtype([("p", "<f4", 3), ("slides", "<u4"), ("v", "<f4", 3), ("flags", "<u4"), ("d0", "<f4", 3), ("stopped", "<u4"), ("np", "<f4", 3), ("pad", "<u4")])
NONE = 0xFFFFFFFF
IDENTITY = (0.0, 0.0, 0.0, 1.0)


def moves(origins, displacements, radius, half_height=0.0, rotations=None, skin=0.01, max_slides=4, ignore_body=NONE):
    """nh_Move records (E.MOVE) from arrays or numbers, as World.move packs them."""
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    m = np.zeros(len(o), dtype=E.MOVE)
    m["origin"], m["displacement"] = o, np.asarray(displacements, dtype=np.float32).reshape(-1, 3)
    m["skin"], m["radius"], m["half_height"], m["max_slides"], m["ignore_body"] = skin, radius, half_height, max_slides, ignore_body
    m["rotation"] = IDENTITY if rotations is None else np.asarray(rotations, dtype=np.float32).reshape(-1, 4)
    return m


def first_casts(m):
    """The nh_CapsuleCast records (E.CAPSULE_CAST) of the moves' first casts: { origin, 1, displacement, ignore_body, rotation, radius, half_height }."""
    c = np.zeros(len(m), dtype=E.CAPSULE_CAST)
    c["origin"], c["max_t"], c["direction"], c["ignore_body"] = m["origin"], 1.0, m["displacement"], m["ignore_body"]
    c["rotation"], c["radius"], c["half_height"] = m["rotation"], m["radius"], m["half_height"]
    return c


def move(rec, nbox, m, words=None, masks=None, mask=NONE, threads=None, casts=False):
    """nh_MoveResult records (E.MOVE_RESULT) of the moves `m` (E.MOVE) by brute force over `rec`.  `words`: a layer word per collider, with `masks` (one
    per move) or `mask` (one for all) -- the masked world of the header; None: every collider is seen.  casts=True: (results, casts made per move)."""
    m = np.ascontiguousarray(m, dtype=E.MOVE)
    rec = np.ascontiguousarray(rec, dtype=H.REC)
    out = np.zeros(len(m), dtype=E.MOVE_RESULT)
    made = np.zeros(len(m), dtype=np.uint32)
    words = None if words is None else np.ascontiguousarray(words, dtype=np.uint32)
    masks = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint32)
    assert words is None or len(words) == len(rec)
    assert masks is None or len(masks) == len(m)
    lib().hm_move(H.p(rec), len(rec), nbox, H.p(m), len(m), H.p(out), None if words is None else H.p(words), None if masks is None else H.p(masks),
                  int(mask) & NONE, H.p(made), H.threads(threads))
    return (out, made) if casts else out


def begin(m):
    """The states (STATE) of the moves `m` before their first casts."""
    m = np.ascontiguousarray(m, dtype=E.MOVE)
    st = np.zeros(len(m), dtype=STATE)
    lib().hm_begin(H.p(m), len(m), H.p(st))
    return st


def advance(m, st, hits):
    """nh_q_move_advance in place on every state of `st` that has not stopped, with the nh_RayHit records `hits` of the casts from st.p along st.v."""
    m = np.ascontiguousarray(m, dtype=E.MOVE)
    hits = np.ascontiguousarray(hits, dtype=E.RAY_HIT)
    assert st.dtype == STATE and st.flags.c_contiguous and len(st) == len(m) == len(hits)
    lib().hm_advance(H.p(m), len(m), H.p(st), H.p(hits))
    return st


def state_casts(m, st):
    """The nh_CapsuleCast records of the next cast of every state: { p, 1, v, ... }."""
    c = first_casts(m)
    c["origin"], c["direction"] = st["p"], st["v"]
    return c
