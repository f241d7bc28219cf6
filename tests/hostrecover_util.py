"""ctypes access to the recover oracle of tests/hostoracle/hostrecover.cpp (built by tests/hostlib.py): nh_recover by brute force over all colliders with
the state machine of nudge_amd/csrc/nh_query.h ("recover") and the device's bits, the oracle of the GPU's k_q_recover; and one step of that state machine
alone, for the REPLAY identity."""
import ctypes as C
import numpy as np

import hostlib as H
from hostlib import records      # noqa: F401
from nudge_amd import engine as E

_SIG = {
    "hr_recover": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32], None),
    "hr_begin": ([C.c_void_p, C.c_uint32, C.c_void_p], None),
    "hr_advance": ([C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p], None),
    "hr_better": ([C.c_float, C.c_uint32, C.c_float, C.c_uint32], C.c_int),
}
lib = H.oracle(_SIG)

# hostrecover.cpp's RecoverState
STATE = np.dtype([("p", "<f4", 3), ("iterations", "<u4"), ("flags", "<u4"), ("stopped", "<u4"), ("pad", "<u4", 2)])
NONE = 0xFFFFFFFF
IDENTITY = (0.0, 0.0, 0.0, 1.0)
SKIN = 0.01


def none_record():
    """The NONE record of nh_RecoverResult.last: normal 0, depth 0, nobody."""
    r = np.zeros((), dtype=E.PENETRATION_HIT)
    r["body"] = r["collider"] = r["tag"] = NONE
    r["shape"] = E.NH_SHAPE_NONE
    return r


def recovers(centres, radii=None, half_extents=None, half_heights=None, rotations=None, skin=SKIN, max_iterations=4, ignore_body=NONE):
    """nh_Recover records (E.RECOVER) from arrays or numbers, as World.recover packs them: spheres (`radii`), capsules (`radii` with `half_heights`) or
    boxes (`half_extents`)."""
    c = np.asarray(centres, dtype=np.float32).reshape(-1, 3)
    m = np.zeros(len(c), dtype=E.RECOVER)
    m["center"] = c
    m["rotation"] = IDENTITY if rotations is None else np.asarray(rotations, dtype=np.float32).reshape(-1, 4)
    if half_extents is not None:
        m["shape"], m["size"] = E.NH_SHAPE_BOX, np.asarray(half_extents, dtype=np.float32).reshape(-1, 3)
    else:
        m["shape"] = E.NH_SHAPE_SPHERE if half_heights is None else E.NH_SHAPE_CAPSULE
        m["size"][:, 0] = radii
        if half_heights is not None:
            m["size"][:, 1] = half_heights
    m["skin"], m["max_iterations"], m["ignore_body"] = skin, max_iterations, ignore_body
    return m


def queries(m, centres=None):
    """The nh_OverlapQuery records (E.OVERLAP_QUERY) a batch of recover records starts with: its first 48 bytes, with the centres replaced where given."""
    m = np.ascontiguousarray(m, dtype=E.RECOVER)
    q = np.zeros(len(m), dtype=E.OVERLAP_QUERY)
    for k in ("center", "shape", "rotation", "size", "ignore_body"):
        q[k] = m[k]
    if centres is not None:
        q["center"] = centres
    return q


def recover(rec, nbox, m, words=None, masks=None, mask=NONE, threads=None, walks=False):
    """nh_RecoverResult records (E.RECOVER_RESULT) of the records `m` (E.RECOVER) by brute force over `rec`.  `words`: a layer word per collider, with
    `masks` (one per query) or `mask` (one for all) -- the masked world of the header; None: every collider is seen.  walks=True: (results, walks
    made per query)."""
    m = np.ascontiguousarray(m, dtype=E.RECOVER)
    rec = np.ascontiguousarray(rec, dtype=H.REC)
    out = np.zeros(len(m), dtype=E.RECOVER_RESULT)
    made = np.zeros(len(m), dtype=np.uint32)
    words = None if words is None else np.ascontiguousarray(words, dtype=np.uint32)
    masks = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint32)
    assert words is None or len(words) == len(rec)
    assert masks is None or len(masks) == len(m)
    lib().hr_recover(H.p(rec), len(rec), nbox, H.p(m), len(m), H.p(out), None if words is None else H.p(words), None if masks is None else H.p(masks),
                     int(mask) & NONE, H.p(made), H.threads(threads))
    return (out, made) if walks else out


def begin(m):
    """The states (STATE) of the records `m` before their first walks; invalid records have stopped."""
    m = np.ascontiguousarray(m, dtype=E.RECOVER)
    st = np.zeros(len(m), dtype=STATE)
    lib().hr_begin(H.p(m), len(m), H.p(st))
    return st


def advance(m, st, found, kept):
    """nh_q_recover_advance in place on every state of `st` that has not stopped, with found[i] (the set at st.p held a collider) and the
    nh_PenetrationHit record kept[i] of the deepest of them."""
    m = np.ascontiguousarray(m, dtype=E.RECOVER)
    kept = np.ascontiguousarray(kept, dtype=E.PENETRATION_HIT)
    found = np.ascontiguousarray(found, dtype=np.uint8)
    assert st.dtype == STATE and st.flags.c_contiguous and len(st) == len(m) == len(kept) == len(found)
    lib().hr_advance(H.p(m), len(m), H.p(st), H.p(found), H.p(kept))
    return st


def deepest(offsets, hits, count):
    """Per query of a penetration batch (offsets of count + 1 words, the nh_PenetrationHit records behind them): (found, the record of greatest depth --
    the first of them in the segment's order, which is by combined collider index).  Queries with an empty segment get the NONE record."""
    off = np.asarray(offsets).astype(np.int64) & NONE
    kept = np.full(count, none_record(), dtype=E.PENETRATION_HIT)
    found = np.zeros(count, dtype=np.uint8)
    for i in np.nonzero(np.diff(off[:count + 1]) > 0)[0]:
        seg = hits[off[i]:off[i + 1]]
        kept[i] = seg[int(np.argmax(seg["depth"]))]
        found[i] = 1
    return found, kept


def better(depth, c, best_depth, best_c):
    return bool(lib().hr_better(C.c_float(depth), int(c), C.c_float(best_depth), int(best_c)))
