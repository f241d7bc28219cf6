"""ctypes access to the walk oracle of tests/hostoracle/hostwalk.cpp (built by tests/hostlib.py): nh_walk by brute force over all colliders with the
phase machine of nudge_amd/csrc/nh_query.h ("walk") and the device's bits, the oracle of the GPU's k_q_walk; and the phases one at a time, for the
REPLAY identity."""
import ctypes as C
import numpy as np

import hostlib as H
from hostlib import records      # noqa: F401
import hostmove_util as HM
from nudge_amd import engine as E

_V, _U = C.c_void_p, C.c_uint32
_SIG = {
    "hw_walk": ([_V, _U, _U, _V, _U, _V, _V, _V, _U, _U], None),
    "hw_replay_state_size": ([], _U),
    "hw_replay_begin": ([_V, _U, _V], None),
    "hw_replay_moves": ([_V, _U, _V, _U, _V, _V], None),
    "hw_replay_phase": ([_V, _U, _V, _U, _V, _V, _V], None),
    "hw_replay_casts": ([_V, _U, _V, _V, _V], None),
    "hw_replay_probe": ([_V, _U, _V, _V, _V], None),
    "hw_replay_finish": ([_V, _U, _V, _V], _U),
    "hw_steep": ([_V, _U, _V, _V], None),
}
lib = H.oracle(_SIG)

NONE = 0xFFFFFFFF
IDENTITY = HM.IDENTITY
# nh_query.h's phases of a walk that run a move loop
PHASE_A, PHASE_U, PHASE_F, PHASE_D = 0, 2, 3, 4
MOVE_FLAGS = E.NH_MOVE_HIT | E.NH_MOVE_START_OVERLAP | E.NH_MOVE_SLIDES_OUT | E.NH_MOVE_WEDGED


def walks(origins, displacements, radius, half_height=0.0, rotations=None, skin=0.01, max_slides=4, ignore_body=NONE, up=(0.0, 1.0, 0.0), step_height=0.0,
          snap_distance=0.0, min_ground_up=0.0, options=0):
    """nh_Walk records (E.WALK) from arrays or numbers, as World.walk packs them."""
    m = HM.moves(origins, displacements, radius, half_height, rotations, skin, max_slides, ignore_body)
    w = np.zeros(len(m), dtype=E.WALK)
    for name in E.MOVE.names:
        w[name] = m[name]
    w["up"], w["step_height"], w["snap_distance"], w["min_ground_up"], w["options"] = up, step_height, snap_distance, min_ground_up, options
    return w


def cos_deg(degrees):
    """min_ground_up of a slope limit in degrees, as float32 (0 degrees given as 0 means no limit: min_ground_up = 0)."""
    d = np.asarray(degrees, dtype=np.float64)
    return np.where(d == 0, 0.0, np.cos(np.deg2rad(d))).astype(np.float32)


def head(w):
    """The nh_Move records (E.MOVE) that are the first 64 bytes of the walks."""
    m = np.zeros(len(w), dtype=E.MOVE)
    for name in E.MOVE.names:
        m[name] = w[name]
    return m


def walk(rec, nbox, w, words=None, masks=None, mask=NONE, threads=None):
    """nh_WalkResult records (E.WALK_RESULT) of the walks `w` (E.WALK) by brute force over `rec`.  `words`: a layer word per collider, with `masks` (one
    per walk) or `mask` (one for all) -- the masked world of the header; None: every collider is seen."""
    w = np.ascontiguousarray(w, dtype=E.WALK)
    rec = np.ascontiguousarray(rec, dtype=H.REC)
    out = np.zeros(len(w), dtype=E.WALK_RESULT)
    words = None if words is None else np.ascontiguousarray(words, dtype=np.uint32)
    masks = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint32)
    assert words is None or len(words) == len(rec)
    assert masks is None or len(masks) == len(w)
    lib().hw_walk(H.p(rec), len(rec), nbox, H.p(w), len(w), H.p(out), None if words is None else H.p(words), None if masks is None else H.p(masks),
                  int(mask) & NONE, H.threads(threads))
    return out


def steep(w, hits):
    """Per walk: is hits[i] (E.RAY_HIT) a taken hit -- a collider at t > 0 -- whose normal is steep for walk i?"""
    w = np.ascontiguousarray(w, dtype=E.WALK)
    hits = np.ascontiguousarray(hits, dtype=E.RAY_HIT)
    out = np.zeros(len(w), dtype=np.uint32)
    lib().hw_steep(H.p(w), len(w), H.p(hits), H.p(out))
    return out != 0


def replay(w, move, capsulecast):
    """The REPLAY identity: the walks `w` (valid records) run phase by phase from the host.  move(nh_Move records) -> nh_MoveResult records and
    capsulecast(nh_CapsuleCast records) -> nh_RayHit records answer the casts (the GPU's calls, or the host's brute force); nh_query.h's decisions are
    kept between them.  `blocked` -- whether a taken hit of A was steep -- is read off nh_move's own replay of A, one capsulecast per round.
    Returns (nh_WalkResult records, the number of move and capsulecast calls made)."""
    w = np.ascontiguousarray(w, dtype=E.WALK)
    n = len(w)
    L = lib()
    st = np.zeros((n, L.hw_replay_state_size()), dtype=np.uint8)
    L.hw_replay_begin(H.p(w), n, H.p(st))
    calls = 0
    # blocked: nh_move's REPLAY of A
    m = head(w)
    ms = HM.begin(m)
    blocked = np.zeros(n, dtype=np.uint32)
    while (ms["stopped"] == 0).any():
        live = ms["stopped"] == 0
        hits = capsulecast(HM.state_casts(m, ms))
        calls += 1
        blocked |= (steep(w, hits) & live).astype(np.uint32)
        HM.advance(m, ms, hits)
    moves = np.zeros(n, dtype=E.MOVE)
    active = np.zeros(n, dtype=np.uint32)
    for phase in (PHASE_A, PHASE_U, PHASE_F, PHASE_D):
        L.hw_replay_moves(H.p(w), n, H.p(st), phase, H.p(moves), H.p(active))
        if not active.any():
            continue
        res = np.ascontiguousarray(move(moves), dtype=E.MOVE_RESULT)
        calls += 1
        L.hw_replay_phase(H.p(w), n, H.p(st), phase, H.p(active), H.p(res), H.p(blocked))
    casts = np.zeros(n, dtype=E.CAPSULE_CAST)
    L.hw_replay_casts(H.p(w), n, H.p(st), H.p(casts), H.p(active))
    if active.any():
        hits = np.ascontiguousarray(capsulecast(casts), dtype=E.RAY_HIT)
        calls += 1
        L.hw_replay_probe(H.p(w), n, H.p(st), H.p(active), H.p(hits))
    out = np.zeros(n, dtype=E.WALK_RESULT)
    left = L.hw_replay_finish(H.p(w), n, H.p(st), H.p(out))
    assert left == 0, f"{left} replayed walks have not ended"
    return out, calls


def shares(w, results):
    """The shares of a batch's results: stepped, grounded, snapped, steep, airborne (the probe was made and missed), slid (slides >= 1)."""
    f = results["flags"]
    probed = ((f & (E.NH_WALK_INVALID | E.NH_MOVE_START_OVERLAP | E.NH_WALK_STEPPED)) == 0) & (w["snap_distance"] > 0)
    return dict(stepped=float(((f & E.NH_WALK_STEPPED) != 0).mean()), grounded=float(((f & E.NH_WALK_GROUNDED) != 0).mean()),
                snapped=float(((f & E.NH_WALK_SNAPPED) != 0).mean()), steep=float(((f & E.NH_WALK_STEEP) != 0).mean()),
                airborne=float((probed & (results["ground"]["shape"] == NONE)).mean()), slid=float((results["slides"] >= 1).mean()))
