// hostmover.cpp -- CPU build of nh_move, nh_boxmove, nh_walk and nh_boxwalk (include/nudge_hip.h): the state machine ("move") and the phase machine ("walk")
// of nudge_amd/csrc/nh_query.h around oracle.h's brute-force closest-hit cast, the oracle of the GPU's k_q_move<Shape, .> and k_q_walk<Shape, .>
// (tests/hostmover_util.py).  Written once over a mover's traits, the host's counterpart of nh_query.hip's nh_QMover<Shape>; every entry point takes the
// shape (NH_SHAPE_CAPSULE or NH_SHAPE_BOX) and the shape's own records.
//   hm_move            every move by brute force: each round's cast is the record { p, 1, v, ignore_body, rotation, the shape } over all colliders.  A layer
//                      filter is the masked world of the header: colliders whose word the move's mask sees nothing of do not exist (words / masks given:
//                      done here per move, without a copy of the records)
//   hm_begin, _advance the state of every move before its first cast, and one application of nh_q_move_advance to a state and a cast's record, for the
//                      REPLAY test
//   hw_walk            every walk by brute force, likewise
//   hw_replay_*        the phases of a walk one at a time, for the REPLAY identity: the caller makes move calls for A, U, F and D and a closest-hit cast
//                      call for C, and these keep nh_q_walk_phase_end / nh_q_walk_advance between them
//   hw_steep           is a hit normal steep for a walk? (nh_q_walk_walkable), for the replay's `blocked`
#include <stddef.h>
#include "oracle.h"

// What the two movers do not share: the records, the swept shape of a record, the record's validity, and the shape's fields from one record to another
struct CapsuleMover {
	typedef nh_Move Move; typedef nh_Walk Walk; typedef nh_CapsuleCast Cast;
	template <class M> static SweptCapsule shape(const M& m) { return SweptCapsule{ q4(m.rotation), m.radius, m.half_height }; }
	static bool valid(const Move& m) { return nh_q_move_valid(v3(m.origin), v3(m.displacement), q4(m.rotation), m.radius, m.half_height, m.skin, m.max_slides); }
	static bool valid(const nh_QWalkIn& W, const Walk& w) { return nh_q_walk_valid(W, q4(w.rotation), w.radius, w.half_height); }
	template <class R, class M> static void copy_shape(R& r, const M& m) { r.radius = m.radius; r.half_height = m.half_height; }
};
struct BoxMover {
	typedef nh_BoxMove Move; typedef nh_BoxWalk Walk; typedef nh_BoxCast Cast;
	template <class M> static SweptBox shape(const M& m) { return SweptBox{ q4(m.rotation), v3(m.size) }; }
	static bool valid(const Move& m) { return nh_q_boxmove_valid(v3(m.origin), v3(m.displacement), q4(m.rotation), v3(m.size), m.skin, m.max_slides); }
	static bool valid(const nh_QWalkIn& W, const Walk& w) { return nh_q_boxwalk_valid(W, q4(w.rotation), v3(w.size)); }
	template <class R, class M> static void copy_shape(R& r, const M& m) { for (int k = 0; k < 3; ++k) r.size[k] = m.size[k]; }
};
// hw_steep reads a walk's `up` and `min_ground_up` alone, which both records keep at the same place
static_assert(offsetof(nh_Walk, up) == offsetof(nh_BoxWalk, up) && offsetof(nh_Walk, min_ground_up) == offsetof(nh_BoxWalk, min_ground_up), "hw_steep");

// f<CapsuleMover>(...) or f<BoxMover>(...) by the entry point's shape argument
#define BY_SHAPE(shape, f, ...) ((shape) == NH_SHAPE_BOX ? f<BoxMover>(__VA_ARGS__) : f<CapsuleMover>(__VA_ARGS__))

static inline void put3(float out[3], nh_f3 a) { out[0] = a.x; out[1] = a.y; out[2] = a.z; }

// the records of the mover `w` (a move or a walk) from o along d: its cast { o, 1, d, ... }, and its move { o, skin, d, ..., max_slides }
template <class T, class M> static typename T::Cast cast_record(const M& w, nh_f3 o, nh_f3 d) {
	typename T::Cast c = typename T::Cast();
	put3(c.origin, o); put3(c.direction, d); c.max_t = 1.0f; c.ignore_body = w.ignore_body;
	for (int k = 0; k < 4; ++k) c.rotation[k] = w.rotation[k];
	T::copy_shape(c, w);
	return c;
}
template <class T, class M> static typename T::Move move_record(const M& w, nh_f3 o, nh_f3 d, uint32_t max_slides) {
	typename T::Move m = typename T::Move();
	put3(m.origin, o); put3(m.displacement, d); m.skin = w.skin; m.ignore_body = w.ignore_body; m.max_slides = max_slides;
	for (int k = 0; k < 4; ++k) m.rotation[k] = w.rotation[k];
	T::copy_shape(m, w);
	return m;
}

// one cast of the mover `w` from o along d with max_t = 1, as closest_hit leaves it
template <class T, class M>
static bool mover_cast(const Rec* rec, uint32_t n, uint32_t nbox, const M& w, nh_f3 o, nh_f3 d, const uint32_t* words, uint32_t mask, float& bt, uint32_t& bc, nh_f3& bn) {
	return closest_hit(rec, n, nbox, T::shape(w), o, d, 1.0f, w.ignore_body, words, mask, -1, bt, bc, bn);
}

// ---- move ----------------------------------------------------------------------------------------------------------------------------------------
template <class T>
static void move_one(const Rec* rec, uint32_t n, uint32_t nbox, const typename T::Move& m, nh_MoveResult& out, const uint32_t* words, uint32_t mask, uint32_t* casts) {
	const nh_f3 o = v3(m.origin), d = v3(m.displacement);
	uint32_t made = 0u;
	if (!T::valid(m)) {
		for (int k = 0; k < 3; ++k) { out.position[k] = m.origin[k]; out.remaining[k] = m.displacement[k]; }
		out.flags = NH_MOVE_INVALID; out.slides = 0u;
		write_ray_miss(out.last_hit, false, 1.0f);
		if (casts) *casts = 0u;
		return;
	}
	nh_QMove s = nh_q_move_begin(o, d);
	write_ray_miss(out.last_hit, true, 1.0f);
	while (nh_q_move_go(s)) {
		float bt; uint32_t bc; nh_f3 bn;
		const bool ok = mover_cast<T>(rec, n, nbox, m, s.p, s.v, words, mask, bt, bc, bn);
		write_cast(out.last_hit, rec, nbox, ok, 1.0f, bt, bc, bn);
		++made;
		if (!nh_q_move_advance(s, bc != 0xffffffffu, bt, bn, m.skin, m.max_slides)) break;
	}
	put3(out.position, s.p); put3(out.remaining, s.v);
	out.flags = s.flags; out.slides = s.slides;
	if (casts) *casts = made;
}

template <class T>
static void move_all(const Rec* rec, uint32_t n, uint32_t nbox, const void* moves_, uint32_t count, nh_MoveResult* results, const uint32_t* words,
                     const uint32_t* masks, uint32_t mask, uint32_t* casts, uint32_t threads) {
	const typename T::Move* moves = (const typename T::Move*)moves_;
	parallel(count, threads, [=](uint32_t i) { move_one<T>(rec, n, nbox, moves[i], results[i], words, masks ? masks[i] : mask, casts ? casts + i : nullptr); });
}

// The state of one move between two casts, as the REPLAY test keeps it: nh_QMove and whether the move has stopped
struct MoveState { float p[3]; uint32_t slides; float v[3]; uint32_t flags; float d0[3]; uint32_t stopped; float np[3]; uint32_t pad; };
static_assert(sizeof(MoveState) == 64, "MoveState is hostmover_util.STATE");

template <class T> static void move_begin(const void* moves_, uint32_t count, MoveState* st) {
	const typename T::Move* moves = (const typename T::Move*)moves_;
	for (uint32_t i = 0; i < count; ++i) {
		const nh_QMove s = nh_q_move_begin(v3(moves[i].origin), v3(moves[i].displacement));
		MoveState& o = st[i];
		put3(o.p, s.p); put3(o.v, s.v); put3(o.d0, s.d0); put3(o.np, s.np);
		o.slides = s.slides; o.flags = s.flags; o.pad = 0u;
		o.stopped = nh_q_move_go(s) ? 0u : 1u;
	}
}

template <class T> static void move_advance(const void* moves_, uint32_t count, MoveState* st, const nh_RayHit* hits) {
	const typename T::Move* moves = (const typename T::Move*)moves_;
	for (uint32_t i = 0; i < count; ++i) {
		MoveState& o = st[i];
		if (o.stopped) continue;
		nh_QMove s;
		s.p = v3(o.p); s.v = v3(o.v); s.d0 = v3(o.d0); s.np = v3(o.np); s.slides = o.slides; s.flags = o.flags;
		const bool on = nh_q_move_advance(s, hits[i].shape != NH_SHAPE_NONE, hits[i].t, v3(hits[i].normal), moves[i].skin, moves[i].max_slides);
		put3(o.p, s.p); put3(o.v, s.v); put3(o.np, s.np);
		o.slides = s.slides; o.flags = s.flags;
		o.stopped = (on && nh_q_move_go(s)) ? 0u : 1u;
	}
}

// ---- walk ----------------------------------------------------------------------------------------------------------------------------------------
template <class W_> static nh_QWalkIn walk_in(const W_& w) {
	nh_QWalkIn W;
	W.origin = v3(w.origin); W.disp = v3(w.displacement); W.up = v3(w.up);
	W.skin = w.skin; W.step_height = w.step_height; W.snap = w.snap_distance; W.mgu = w.min_ground_up;
	W.max_slides = w.max_slides; W.options = w.options;
	return W;
}

// a state's hit as its nh_RayHit: a collider by its combined index, or the miss record (t = 1, or NaN where the cast was invalid: the state holds either)
static void write_walk_hit(nh_RayHit& out, const Rec* rec, uint32_t nbox, const nh_QWalkHit& h) {
	if (h.c == NH_Q_WALK_NOBODY) { write_ray_miss(out, true, h.t); return; }
	write_ray_hit(out, rec, nbox, h.c, h.t, h.n);
}

static void write_head(const nh_QWalk& s, const nh_QWalkIn& W, nh_WalkResult& out) {
	put3(out.position, s.kp); put3(out.remaining, s.kv);
	out.flags = s.kflags; out.slides = s.kslides;
	out.step_up = s.step_up; out.drop = nh_q_walk_drop(s, W); out.casts = s.casts; out.reserved = 0u;
}

template <class T>
static void walk_one(const Rec* rec, uint32_t n, uint32_t nbox, const typename T::Walk& w, nh_WalkResult& out, const uint32_t* words, uint32_t mask) {
	const nh_QWalkIn W = walk_in(w);
	if (!T::valid(W, w)) {
		for (int k = 0; k < 3; ++k) { out.position[k] = w.origin[k]; out.remaining[k] = w.displacement[k]; }
		out.flags = NH_WALK_INVALID; out.slides = 0u; out.step_up = 0.0f; out.drop = 0.0f; out.casts = 0u; out.reserved = 0u;
		write_ray_miss(out.last_hit, false, 1.0f);
		write_ray_miss(out.ground, false, 1.0f);
		return;
	}
	nh_QWalk s = nh_q_walk_begin(W);
	while (nh_q_walk_cast(s, W)) {
		float bt; uint32_t bc; nh_f3 bn;
		const bool ok = mover_cast<T>(rec, n, nbox, w, s.m.p, s.m.v, words, mask, bt, bc, bn);
		nh_q_walk_advance(s, W, bc != 0xffffffffu, bt, bc, bn, ok);
	}
	write_head(s, W, out);
	write_walk_hit(out.last_hit, rec, nbox, s.klast);
	write_walk_hit(out.ground, rec, nbox, nh_q_walk_ground(s));
}

template <class T>
static void walk_all(const Rec* rec, uint32_t n, uint32_t nbox, const void* walks_, uint32_t count, nh_WalkResult* results, const uint32_t* words,
                     const uint32_t* masks, uint32_t mask, uint32_t threads) {
	const typename T::Walk* walks = (const typename T::Walk*)walks_;
	parallel(count, threads, [=](uint32_t i) { walk_one<T>(rec, n, nbox, walks[i], results[i], words, masks ? masks[i] : mask); });
}

// The replay's state of one walk: the phase machine's, and the record each phase's last cast wrote (a state's hit names it by c = the phase)
struct ReplayState { nh_QWalk s; nh_RayHit rec[8]; };

static nh_QWalkHit replay_hit(const nh_RayHit& h, uint32_t phase) {
	nh_QWalkHit o;
	o.t = h.t; o.n = v3(h.normal); o.c = h.shape != NH_SHAPE_NONE ? phase : NH_Q_WALK_NOBODY;
	return o;
}

static void replay_write_hit(nh_RayHit& out, const ReplayState& r, const nh_QWalkHit& h) {
	if (h.c == NH_Q_WALK_NOBODY) write_ray_miss(out, true, h.t);
	else out = r.rec[h.c];
}

template <class T> static void replay_begin(const void* walks_, uint32_t count, ReplayState* st) {
	const typename T::Walk* walks = (const typename T::Walk*)walks_;
	for (uint32_t i = 0; i < count; ++i) {
		st[i].s = nh_q_walk_begin(walk_in(walks[i]));
		for (int k = 0; k < 8; ++k) write_ray_miss(st[i].rec[k], true, 1.0f);
	}
}

template <class T> static void replay_moves(const void* walks_, uint32_t count, const ReplayState* st, uint32_t phase, void* moves_, uint32_t* active) {
	const typename T::Walk* walks = (const typename T::Walk*)walks_;
	typename T::Move* moves = (typename T::Move*)moves_;
	for (uint32_t i = 0; i < count; ++i) {
		const typename T::Walk& w = walks[i];
		const nh_QWalk& s = st[i].s;
		active[i] = (s.phase == phase || (phase == NH_Q_WALK_A && s.phase == NH_Q_WALK_AB)) ? 1u : 0u;
		if (active[i]) moves[i] = move_record<T>(w, s.m.p, s.m.v, nh_q_walk_slides(s, walk_in(w)));
		else moves[i] = move_record<T>(w, v3(w.origin), nh_make3(0.0f, 0.0f, 0.0f), 0u);
	}
}

template <class T>
static void replay_phase(const void* walks_, uint32_t count, ReplayState* st, uint32_t phase, const uint32_t* active, const nh_MoveResult* res, const uint32_t* blocked) {
	const typename T::Walk* walks = (const typename T::Walk*)walks_;
	for (uint32_t i = 0; i < count; ++i) {
		if (!active[i]) continue;
		nh_QWalk& s = st[i].s;
		const nh_QWalkIn W = walk_in(walks[i]);
		const nh_MoveResult& r = res[i];
		const bool went = nh_q_move_go(s.m);
		s.m.p = v3(r.position); s.m.v = v3(r.remaining); s.m.slides = r.slides; s.m.flags = r.flags;
		s.last = replay_hit(r.last_hit, phase);
		st[i].rec[phase] = r.last_hit;
		// the casts the move call made, from its result: every taken hit is one (slides).  The loop then ended in one of these ways:
		//   v.v == 0 before the first cast (!went)      no cast; last_hit is the initial miss record
		//   WEDGED / v = 0 after a hit, or SLIDES_OUT    no further cast; last_hit is the last taken hit (a collider)
		//   a cast that missed                          one more; last_hit is a miss (shape NONE)
		//   a cast from an overflowed p (invalid)       one more; it answers as a miss with t = NaN, shape NONE as well
		//   a cast that started in overlap (t == 0)     one more; START_OVERLAP, last_hit is a collider
		s.casts += r.slides + ((r.flags & NH_MOVE_START_OVERLAP) ? 1u : 0u) + ((went && r.last_hit.shape == NH_SHAPE_NONE) ? 1u : 0u);
		if (phase == NH_Q_WALK_A && blocked[i]) s.phase = NH_Q_WALK_AB;
		nh_q_walk_phase_end(s, W);
	}
}

template <class T> static void replay_casts(const void* walks_, uint32_t count, const ReplayState* st, void* casts_, uint32_t* active) {
	const typename T::Walk* walks = (const typename T::Walk*)walks_;
	typename T::Cast* casts = (typename T::Cast*)casts_;
	for (uint32_t i = 0; i < count; ++i) {
		const typename T::Walk& w = walks[i];
		const nh_QWalk& s = st[i].s;
		active[i] = s.phase == NH_Q_WALK_C ? 1u : 0u;
		casts[i] = cast_record<T>(w, active[i] ? s.m.p : v3(w.origin), active[i] ? s.m.v : v3(w.displacement));
	}
}

template <class T> static void replay_probe(const void* walks_, uint32_t count, ReplayState* st, const uint32_t* active, const nh_RayHit* hits) {
	const typename T::Walk* walks = (const typename T::Walk*)walks_;
	for (uint32_t i = 0; i < count; ++i) {
		if (!active[i]) continue;
		const nh_RayHit& h = hits[i];
		st[i].rec[NH_Q_WALK_C] = h;
		const bool hit = h.shape != NH_SHAPE_NONE;
		nh_q_walk_advance(st[i].s, walk_in(walks[i]), hit, hit ? h.t : 1.0f, NH_Q_WALK_C, v3(h.normal), hit || h.t == h.t);
	}
}

template <class T> static uint32_t replay_finish(const void* walks_, uint32_t count, const ReplayState* st, nh_WalkResult* results) {
	const typename T::Walk* walks = (const typename T::Walk*)walks_;
	uint32_t left = 0u;
	for (uint32_t i = 0; i < count; ++i) {
		const nh_QWalk& s = st[i].s;
		if (s.phase < NH_Q_WALK_END) ++left;
		write_head(s, walk_in(walks[i]), results[i]);
		replay_write_hit(results[i].last_hit, st[i], s.klast);
		replay_write_hit(results[i].ground, st[i], nh_q_walk_ground(s));
	}
	return left;
}

extern "C" {

// words: one layer word per collider, or NULL; masks: one mask per move, or NULL (every move uses `mask`).  casts: the casts each move made, or NULL
void hm_move(uint32_t shape, const Rec* rec, uint32_t n, uint32_t nbox, const void* moves, uint32_t count, nh_MoveResult* results, const uint32_t* words,
             const uint32_t* masks, uint32_t mask, uint32_t* casts, uint32_t threads) {
	BY_SHAPE(shape, move_all, rec, n, nbox, moves, count, results, words, masks, mask, casts, threads);
}

// begin: the state of moves[i] before its first cast; stopped = 1 where rule 1 ends it at once (an invalid record is not the state machine's: the caller
// leaves those out)
void hm_begin(uint32_t shape, const void* moves, uint32_t count, MoveState* st) { BY_SHAPE(shape, move_begin, moves, count, st); }

// advance: for every state that has not stopped, nh_q_move_advance with hits[i] (the record the shape's cast from st[i].p along st[i].v with max_t = 1
// wrote), then rule 1; states that have stopped are left alone
void hm_advance(uint32_t shape, const void* moves, uint32_t count, MoveState* st, const nh_RayHit* hits) { BY_SHAPE(shape, move_advance, moves, count, st, hits); }

// words: one layer word per collider, or NULL; masks: one mask per walk, or NULL (every walk uses `mask`)
void hw_walk(uint32_t shape, const Rec* rec, uint32_t n, uint32_t nbox, const void* walks, uint32_t count, nh_WalkResult* results, const uint32_t* words,
             const uint32_t* masks, uint32_t mask, uint32_t threads) {
	BY_SHAPE(shape, walk_all, rec, n, nbox, walks, count, results, words, masks, mask, threads);
}

uint32_t hw_replay_state_size() { return (uint32_t)sizeof(ReplayState); }

// begin: the state of every walk before A (invalid records are not the phase machine's: the caller leaves them out)
void hw_replay_begin(uint32_t shape, const void* walks, uint32_t count, ReplayState* st) { BY_SHAPE(shape, replay_begin, walks, count, st); }

// the shape's move records of the phase `phase` (NH_Q_WALK_A, _U, _F, _D): for a walk in that phase its running loop { p, v, the phase's slides }, active = 1;
// for any other a record that moves nowhere, active = 0
void hw_replay_moves(uint32_t shape, const void* walks, uint32_t count, const ReplayState* st, uint32_t phase, void* moves, uint32_t* active) {
	BY_SHAPE(shape, replay_moves, walks, count, st, phase, moves, active);
}

// behind the move call of a phase: for every active walk the loop's end as the call wrote it, then nh_q_walk_phase_end.  blocked (phase A only): whether a
// taken hit of A was steep.  The casts a move made: one per hit taken, and the last one where it ended in a miss or a start overlap.
void hw_replay_phase(uint32_t shape, const void* walks, uint32_t count, ReplayState* st, uint32_t phase, const uint32_t* active, const nh_MoveResult* res,
                     const uint32_t* blocked) {
	BY_SHAPE(shape, replay_phase, walks, count, st, phase, active, res, blocked);
}

// the shape's cast records of the probes: for a walk in phase C { p, 1, v, ... }, active = 1; for any other its first cast, active = 0
void hw_replay_casts(uint32_t shape, const void* walks, uint32_t count, const ReplayState* st, void* casts, uint32_t* active) {
	BY_SHAPE(shape, replay_casts, walks, count, st, casts, active);
}

// behind the cast call of the probes: nh_q_walk_advance with each active walk's record (an invalid cast wrote the miss record with t = NaN)
void hw_replay_probe(uint32_t shape, const void* walks, uint32_t count, ReplayState* st, const uint32_t* active, const nh_RayHit* hits) {
	BY_SHAPE(shape, replay_probe, walks, count, st, active, hits);
}

// the nh_WalkResult records of the replayed walks; left: how many have not ended
uint32_t hw_replay_finish(uint32_t shape, const void* walks, uint32_t count, const ReplayState* st, nh_WalkResult* results) {
	return BY_SHAPE(shape, replay_finish, walks, count, st, results);
}

// steep[i] = 1 where hits[i] is a taken hit (a collider, t > 0) whose normal is not walkable for walks[i] (a box walk's record serves as well: above)
void hw_steep(const nh_Walk* walks, uint32_t count, const nh_RayHit* hits, uint32_t* steep) {
	for (uint32_t i = 0; i < count; ++i)
		steep[i] = (hits[i].shape != NH_SHAPE_NONE && hits[i].t != 0.0f && !nh_q_walk_walkable(v3(hits[i].normal), walk_in(walks[i]))) ? 1u : 0u;
}

}
