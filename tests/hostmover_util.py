"""ctypes access to the mover oracle of tests/hostoracle/hostmover.cpp (built by tests/hostlib.py): nh_move, nh_boxmove, nh_walk and nh_boxwalk by brute
force over all colliders with the state machine ("move") and the phase machine ("walk") of nudge_amd/csrc/nh_query.h and the device's bits, the oracle
of the GPU's k_q_move and k_q_walk; and the steps of those machines alone, for the REPLAY identities.

CAPSULE and BOX are the two movers, with the same members: what differs is the records and the fields that hold the shape's size."""
import ctypes as C
import numpy as np

import hostlib as H
from hostlib import records      # noqa: F401
from nudge_amd import engine as E

_V, _U = C.c_void_p, C.c_uint32
_SIG = {
    "hm_move": ([_U, _V, _U, _U, _V, _U, _V, _V, _V, _U, _V, _U], None),
    "hm_begin": ([_U, _V, _U, _V], None),
    "hm_advance": ([_U, _V, _U, _V, _V], None),
    "hw_walk": ([_U, _V, _U, _U, _V, _U, _V, _V, _V, _U, _U], None),
    "hw_replay_state_size": ([], _U),
    "hw_replay_begin": ([_U, _V, _U, _V], None),
    "hw_replay_moves": ([_U, _V, _U, _V, _U, _V, _V], None),
    "hw_replay_phase": ([_U, _V, _U, _V, _U, _V, _V, _V], None),
    "hw_replay_casts": ([_U, _V, _U, _V, _V, _V], None),
    "hw_replay_probe": ([_U, _V, _U, _V, _V, _V], None),
    "hw_replay_finish": ([_U, _V, _U, _V, _V], _U),
    "hw_steep": ([_V, _U, _V, _V], None),
}
lib = H.oracle(_SIG)

# hostmover.cpp's MoveState
STATE = np.dtype([("p", "<f4", 3), ("slides", "<u4"), ("v", "<f4", 3), ("flags", "<u4"), ("d0", "<f4", 3), ("stopped", "<u4"), ("np", "<f4", 3), ("pad", "<u4")])
NONE = 0xFFFFFFFF
IDENTITY = (0.0, 0.0, 0.0, 1.0)
# nh_query.h's phases of a walk that run a move loop
PHASE_A, PHASE_U, PHASE_F, PHASE_D = 0, 2, 3, 4
MOVE_FLAGS = E.NH_MOVE_HIT | E.NH_MOVE_START_OVERLAP | E.NH_MOVE_SLIDES_OUT | E.NH_MOVE_WEDGED


def cos_deg(degrees):
    """min_ground_up of a slope limit in degrees, as float32 (0 degrees given as 0 means no limit: min_ground_up = 0)."""
    d = np.asarray(degrees, dtype=np.float64)
    return np.where(d == 0, 0.0, np.cos(np.deg2rad(d))).astype(np.float32)


def shares(w, results):
    """The shares of a batch's results: stepped, grounded, snapped, steep, airborne (the probe was made and missed), slid (slides >= 1)."""
    f = results["flags"]
    probed = ((f & (E.NH_WALK_INVALID | E.NH_MOVE_START_OVERLAP | E.NH_WALK_STEPPED)) == 0) & (w["snap_distance"] > 0)
    return dict(stepped=float(((f & E.NH_WALK_STEPPED) != 0).mean()), grounded=float(((f & E.NH_WALK_GROUNDED) != 0).mean()),
                snapped=float(((f & E.NH_WALK_SNAPPED) != 0).mean()), steep=float(((f & E.NH_WALK_STEEP) != 0).mean()),
                airborne=float((probed & (results["ground"]["shape"] == NONE)).mean()), slid=float((results["slides"] >= 1).mean()))


def _opt(a, n):
    """(the array as uint32 or None, its pointer or None); an array has n entries"""
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=np.uint32)
    assert len(a) == n
    return a, H.p(a)


class Mover:
    """One shape's movers: `shape` (E.NH_SHAPE_*), its record dtypes MOVE, WALK and CAST, and the fields `size` of all three that hold the shape."""

    def __init__(self, shape, move, walk, cast, size):
        self.shape, self.MOVE, self.WALK, self.CAST, self.size = shape, move, walk, cast, size

    def _copy(self, out, src, names):
        for name in names:
            out[name] = src[name]
        return out

    # ---- records --------------------------------------------------------------------------------------------------------------------------
    def moves(self, origins, displacements, *size, rotations=None, skin=0.01, max_slides=4, ignore_body=NONE, dtype=None):
        """The shape's move records (MOVE) from arrays or numbers, as World.move / World.boxmove pack them.  `size`: radius[, half_height = 0] of
        the capsule, half_extents of the box.  (`dtype`: WALK, for walks().)"""
        o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
        m = np.zeros(len(o), dtype=dtype or self.MOVE)
        m["origin"], m["displacement"] = o, np.asarray(displacements, dtype=np.float32).reshape(-1, 3)
        m["skin"], m["max_slides"], m["ignore_body"] = skin, max_slides, ignore_body
        if self.shape == E.NH_SHAPE_BOX:
            (half_extents,) = size
            m["size"] = np.asarray(half_extents, dtype=np.float32).reshape(-1, 3)
        else:
            m["radius"], m["half_height"] = size if len(size) == 2 else (*size, 0.0)
        m["rotation"] = IDENTITY if rotations is None else np.asarray(rotations, dtype=np.float32).reshape(-1, 4)
        return m

    def walks(self, origins, displacements, *size, up=(0.0, 1.0, 0.0), step_height=0.0, snap_distance=0.0, min_ground_up=0.0, options=0, **head):
        """The shape's walk records (WALK) from arrays or numbers, as World.walk / World.boxwalk pack them: moves()'s arguments and the walk's own."""
        w = self.moves(origins, displacements, *size, dtype=self.WALK, **head)
        w["up"], w["step_height"], w["snap_distance"], w["min_ground_up"], w["options"] = up, step_height, snap_distance, min_ground_up, options
        return w

    def head(self, w):
        """The move records (MOVE) that are the first 64 bytes of the walks."""
        return self._copy(np.zeros(len(w), dtype=self.MOVE), w, self.MOVE.names)

    def first_casts(self, m):
        """The shape's cast records (CAST) of the moves' first casts: { origin, 1, displacement, ignore_body, rotation, the shape's size }."""
        c = np.zeros(len(m), dtype=self.CAST)
        c["origin"], c["max_t"], c["direction"] = m["origin"], 1.0, m["displacement"]
        return self._copy(c, m, ("ignore_body", "rotation") + self.size)

    def state_casts(self, m, st):
        """The cast records of the next cast of every state: { p, 1, v, ... }."""
        c = self.first_casts(m)
        c["origin"], c["direction"] = st["p"], st["v"]
        return c

    def overlap_queries(self, m):
        """The nh_OverlapQuery records (E.OVERLAP_QUERY) of the shapes at the moves' origins, ignoring nothing."""
        q = np.zeros(len(m), dtype=E.OVERLAP_QUERY)
        q["center"], q["shape"], q["rotation"], q["ignore_body"] = m["origin"], self.shape, m["rotation"], NONE
        if self.shape == E.NH_SHAPE_BOX:
            q["size"] = m["size"]
        else:
            q["size"][:, 0], q["size"][:, 1] = m["radius"], m["half_height"]
        return q

    # ---- move -----------------------------------------------------------------------------------------------------------------------------
    def move(self, rec, nbox, m, words=None, masks=None, mask=NONE, threads=None, casts=False):
        """nh_MoveResult records (E.MOVE_RESULT) of the moves `m` (MOVE) by brute force over `rec`.  `words`: a layer word per collider, with `masks`
        (one per move) or `mask` (one for all) -- the masked world of the header; None: every collider is seen.  casts=True: (results, casts made per
        move)."""
        m = np.ascontiguousarray(m, dtype=self.MOVE)
        rec = np.ascontiguousarray(rec, dtype=H.REC)
        out = np.zeros(len(m), dtype=E.MOVE_RESULT)
        made = np.zeros(len(m), dtype=np.uint32)
        (words, pw), (masks, pm) = _opt(words, len(rec)), _opt(masks, len(m))
        lib().hm_move(self.shape, H.p(rec), len(rec), nbox, H.p(m), len(m), H.p(out), pw, pm, int(mask) & NONE, H.p(made), H.threads(threads))
        return (out, made) if casts else out

    def begin(self, m):
        """The states (STATE) of the moves `m` before their first casts."""
        m = np.ascontiguousarray(m, dtype=self.MOVE)
        st = np.zeros(len(m), dtype=STATE)
        lib().hm_begin(self.shape, H.p(m), len(m), H.p(st))
        return st

    def advance(self, m, st, hits):
        """nh_q_move_advance in place on every state of `st` that has not stopped, with the nh_RayHit records `hits` of the casts from st.p along st.v."""
        m = np.ascontiguousarray(m, dtype=self.MOVE)
        hits = np.ascontiguousarray(hits, dtype=E.RAY_HIT)
        assert st.dtype == STATE and st.flags.c_contiguous and len(st) == len(m) == len(hits)
        lib().hm_advance(self.shape, H.p(m), len(m), H.p(st), H.p(hits))
        return st

    def replay_move(self, m, cast):
        """The REPLAY identity: the valid moves `m` run round by round from the host, cast(CAST records) -> nh_RayHit records answering each round
        (the GPU's call, or the host's brute force).  Returns (nh_MoveResult records, rounds made)."""
        m = np.ascontiguousarray(m, dtype=self.MOVE)
        st = self.begin(m)
        last = np.zeros(len(m), dtype=E.RAY_HIT)
        last["t"], last["body"], last["collider"], last["shape"], last["tag"] = 1.0, NONE, NONE, NONE, NONE
        rounds = 0
        while (st["stopped"] == 0).any():
            live = st["stopped"] == 0
            hits = np.ascontiguousarray(cast(self.state_casts(m, st)), dtype=E.RAY_HIT)
            last[live] = hits[live]
            self.advance(m, st, hits)
            rounds += 1
        out = np.zeros(len(m), dtype=E.MOVE_RESULT)
        out["position"], out["remaining"], out["flags"], out["slides"], out["last_hit"] = st["p"], st["v"], st["flags"], st["slides"], last
        return out, rounds

    # ---- walk -----------------------------------------------------------------------------------------------------------------------------
    def walk(self, rec, nbox, w, words=None, masks=None, mask=NONE, threads=None):
        """nh_WalkResult records (E.WALK_RESULT) of the walks `w` (WALK) by brute force over `rec`.  `words`: a layer word per collider, with `masks`
        (one per walk) or `mask` (one for all) -- the masked world of the header; None: every collider is seen."""
        w = np.ascontiguousarray(w, dtype=self.WALK)
        rec = np.ascontiguousarray(rec, dtype=H.REC)
        out = np.zeros(len(w), dtype=E.WALK_RESULT)
        (words, pw), (masks, pm) = _opt(words, len(rec)), _opt(masks, len(w))
        lib().hw_walk(self.shape, H.p(rec), len(rec), nbox, H.p(w), len(w), H.p(out), pw, pm, int(mask) & NONE, H.threads(threads))
        return out

    def steep(self, w, hits):
        """Per walk: is hits[i] (E.RAY_HIT) a taken hit -- a collider at t > 0 -- whose normal is steep for walk i?"""
        w = np.ascontiguousarray(w, dtype=self.WALK)
        hits = np.ascontiguousarray(hits, dtype=E.RAY_HIT)
        out = np.zeros(len(w), dtype=np.uint32)
        lib().hw_steep(H.p(w), len(w), H.p(hits), H.p(out))
        return out != 0

    def replay_walk(self, w, move, cast):
        """The REPLAY identity: the walks `w` (valid records) run phase by phase from the host.  move(MOVE records) -> nh_MoveResult records and
        cast(CAST records) -> nh_RayHit records answer the casts (the GPU's calls, or the host's brute force); nh_query.h's decisions are kept
        between them.  `blocked` -- whether a taken hit of A was steep -- is read off the move's own replay of A, one cast call per round.
        Returns (nh_WalkResult records, the number of move and cast calls made)."""
        w = np.ascontiguousarray(w, dtype=self.WALK)
        n = len(w)
        L = lib()
        st = np.zeros((n, L.hw_replay_state_size()), dtype=np.uint8)
        L.hw_replay_begin(self.shape, H.p(w), n, H.p(st))
        calls = 0
        # blocked: the move's REPLAY of A
        m = self.head(w)
        ms = self.begin(m)
        blocked = np.zeros(n, dtype=np.uint32)
        while (ms["stopped"] == 0).any():
            live = ms["stopped"] == 0
            hits = cast(self.state_casts(m, ms))
            calls += 1
            blocked |= (self.steep(w, hits) & live).astype(np.uint32)
            self.advance(m, ms, hits)
        moves = np.zeros(n, dtype=self.MOVE)
        active = np.zeros(n, dtype=np.uint32)
        for phase in (PHASE_A, PHASE_U, PHASE_F, PHASE_D):
            L.hw_replay_moves(self.shape, H.p(w), n, H.p(st), phase, H.p(moves), H.p(active))
            if not active.any():
                continue
            res = np.ascontiguousarray(move(moves), dtype=E.MOVE_RESULT)
            calls += 1
            L.hw_replay_phase(self.shape, H.p(w), n, H.p(st), phase, H.p(active), H.p(res), H.p(blocked))
        casts = np.zeros(n, dtype=self.CAST)
        L.hw_replay_casts(self.shape, H.p(w), n, H.p(st), H.p(casts), H.p(active))
        if active.any():
            hits = np.ascontiguousarray(cast(casts), dtype=E.RAY_HIT)
            calls += 1
            L.hw_replay_probe(self.shape, H.p(w), n, H.p(st), H.p(active), H.p(hits))
        out = np.zeros(n, dtype=E.WALK_RESULT)
        left = L.hw_replay_finish(self.shape, H.p(w), n, H.p(st), H.p(out))
        assert left == 0, f"{left} replayed walks have not ended"
        return out, calls


CAPSULE = Mover(E.NH_SHAPE_CAPSULE, E.MOVE, E.WALK, E.CAPSULE_CAST, ("radius", "half_height"))
BOX = Mover(E.NH_SHAPE_BOX, E.BOX_MOVE, E.BOX_WALK, E.BOX_CAST, ("size",))
