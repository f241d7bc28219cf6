"""ctypes access to the box-walk oracle of tests/hostoracle/hostboxwalk.cpp (built by tests/hostlib.py): nh_boxwalk by brute force over all colliders
with the phase machine of nudge_amd/csrc/nh_query.h ("walk") and the device's bits, the oracle of the GPU's k_q_walk<nh_QBox, .>; and the REPLAY
identity through hostwalk_util.replay, whose helpers read a walk's rules and never its shape."""
import ctypes as C
import numpy as np

import hostlib as H
from hostlib import records      # noqa: F401
import hostboxmove_util as HBM
import hostwalk_util as HW
from hostwalk_util import cos_deg, shares      # noqa: F401
from nudge_amd import engine as E

_V, _U = C.c_void_p, C.c_uint32
lib = H.oracle({"hbw_walk": ([_V, _U, _U, _V, _U, _V, _V, _V, _U, _U], None)})

NONE = 0xFFFFFFFF
_TAIL = ("up", "step_height", "snap_distance", "min_ground_up", "options", "reserved2")


def walks(origins, displacements, half_extents, rotations=None, skin=0.01, max_slides=4, ignore_body=NONE, up=(0.0, 1.0, 0.0), step_height=0.0,
          snap_distance=0.0, min_ground_up=0.0, options=0):
    """nh_BoxWalk records (E.BOX_WALK) from arrays or numbers, as World.boxwalk packs them."""
    m = HBM.moves(origins, displacements, half_extents, rotations, skin, max_slides, ignore_body)
    w = np.zeros(len(m), dtype=E.BOX_WALK)
    for name in E.BOX_MOVE.names:
        w[name] = m[name]
    w["up"], w["step_height"], w["snap_distance"], w["min_ground_up"], w["options"] = up, step_height, snap_distance, min_ground_up, options
    return w


def head(w):
    """The nh_BoxMove records (E.BOX_MOVE) that are the first 64 bytes of the walks."""
    m = np.zeros(len(w), dtype=E.BOX_MOVE)
    for name in E.BOX_MOVE.names:
        m[name] = w[name]
    return m


def walk(rec, nbox, w, words=None, masks=None, mask=NONE, threads=None):
    """nh_WalkResult records (E.WALK_RESULT) of the walks `w` (E.BOX_WALK) by brute force over `rec`.  `words`: a layer word per collider, with `masks`
    (one per walk) or `mask` (one for all) -- the masked world of the header; None: every collider is seen."""
    w = np.ascontiguousarray(w, dtype=E.BOX_WALK)
    rec = np.ascontiguousarray(rec, dtype=H.REC)
    out = np.zeros(len(w), dtype=E.WALK_RESULT)
    words = None if words is None else np.ascontiguousarray(words, dtype=np.uint32)
    masks = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint32)
    assert words is None or len(words) == len(rec)
    assert masks is None or len(masks) == len(w)
    lib().hbw_walk(H.p(rec), len(rec), nbox, H.p(w), len(w), H.p(out), None if words is None else H.p(words), None if masks is None else H.p(masks),
                   int(mask) & NONE, H.threads(threads))
    return out


def replay(w, boxmove, boxcast):
    """The REPLAY identity for the valid box walks `w` (E.BOX_WALK): hostwalk_util.replay -- nh_query.h's decisions between the phases, kept by
    hostwalk.cpp -- with adaptors that turn the nh_Move and nh_CapsuleCast records it asks about into the nh_BoxMove and nh_BoxCast records of the
    same lanes.  boxmove(nh_BoxMove records) -> nh_MoveResult records and boxcast(nh_BoxCast records) -> nh_RayHit records answer them (the GPU's calls,
    or the host's brute force).  Returns (nh_WalkResult records, the number of boxmove and boxcast calls made)."""
    w = np.ascontiguousarray(w, dtype=E.BOX_WALK)
    # the capsule-headed twin: every field the phase machine reads (the capsule's own radius and half height it never does)
    cw = np.zeros(len(w), dtype=E.WALK)
    for name in ("origin", "skin", "displacement", "ignore_body", "rotation", "max_slides") + _TAIL:
        cw[name] = w[name]

    def move(m):
        assert len(m) == len(w)
        b = np.zeros(len(m), dtype=E.BOX_MOVE)
        for name in ("origin", "skin", "displacement", "ignore_body", "rotation", "max_slides"):
            b[name] = m[name]
        b["size"] = w["size"]
        return boxmove(b)

    def cast(c):
        assert len(c) == len(w)
        b = np.zeros(len(c), dtype=E.BOX_CAST)
        for name in ("origin", "max_t", "direction", "ignore_body", "rotation"):
            b[name] = c[name]
        b["size"] = w["size"]
        return boxcast(b)

    return HW.replay(cw, move, cast)
