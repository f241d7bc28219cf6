// hosttouch.cpp -- CPU build of nh_move_touched, nh_boxmove_touched, nh_walk_touched and nh_boxwalk_touched (include/nudge_hip.h): the loops of hostmover.cpp
// -- the state machine ("move") and the phase machine ("walk") of nudge_amd/csrc/nh_query.h around oracle.h's brute-force closest-hit cast -- which write,
// beside each result, one nh_Touch for every cast that found a collider: the oracle of the GPU's k_q_move<Shape, ., true> and k_q_walk<Shape, ., true>
// (tests/hosttouch_util.py).  The touch is taken where the kernel takes it: behind the cast and BEFORE the advance, while the state holds the cast's origin
// and direction.  counts[i] counts every touch; only the first min(counts[i], k) slots of record i are written, and the oracle never clears `touches`, so the
// "slots behind the count are not written" rule can be tested on it as on the GPU.
//   ht_move   every move by brute force (hm_move's arguments, and k, counts, touches)
//   ht_walk   every walk by brute force (hw_walk's arguments, and k, counts, touches)
#include <stddef.h>
#include "oracle.h"

static_assert(sizeof(nh_Touch) == 64 && offsetof(nh_Touch, origin) == 32 && offsetof(nh_Touch, direction) == 48, "nh_Touch is hosttouch_util's E.TOUCH");
static_assert(NH_Q_TOUCH_SLIDE == NH_TOUCH_SLIDE && NH_Q_TOUCH_UP == NH_TOUCH_UP && NH_Q_TOUCH_FORWARD == NH_TOUCH_FORWARD && NH_Q_TOUCH_DOWN == NH_TOUCH_DOWN &&
              NH_Q_TOUCH_PROBE == NH_TOUCH_PROBE, "nh_query.h's touch phases are the header's");

namespace {

// What the two movers do not share (hostmover.cpp's traits are local to that file): the records, the swept shape of a record and the record's validity
struct CapsuleMover {
	typedef nh_Move Move; typedef nh_Walk Walk;
	template <class M> static SweptCapsule shape(const M& m) { return SweptCapsule{ q4(m.rotation), m.radius, m.half_height }; }
	static bool valid(const Move& m) { return nh_q_move_valid(v3(m.origin), v3(m.displacement), q4(m.rotation), m.radius, m.half_height, m.skin, m.max_slides); }
	static bool valid(const nh_QWalkIn& W, const Walk& w) { return nh_q_walk_valid(W, q4(w.rotation), w.radius, w.half_height); }
};
struct BoxMover {
	typedef nh_BoxMove Move; typedef nh_BoxWalk Walk;
	template <class M> static SweptBox shape(const M& m) { return SweptBox{ q4(m.rotation), v3(m.size) }; }
	static bool valid(const Move& m) { return nh_q_boxmove_valid(v3(m.origin), v3(m.displacement), q4(m.rotation), v3(m.size), m.skin, m.max_slides); }
	static bool valid(const nh_QWalkIn& W, const Walk& w) { return nh_q_boxwalk_valid(W, q4(w.rotation), v3(w.size)); }
};

void put3(float out[3], nh_f3 a) { out[0] = a.x; out[1] = a.y; out[2] = a.z; }

// The touches of one record: the k slots it owns and how many touches it has had
struct Touches {
	nh_Touch* slots; uint32_t k, count;
	// the cast from o along d found collider c at t with normal n
	void take(const Rec* rec, uint32_t nbox, uint32_t c, float t, nh_f3 n, nh_f3 o, nh_f3 d, uint32_t phase, uint32_t cast) {
		if (count < k) {
			nh_Touch& out = slots[count];
			write_ray_hit(out.hit, rec, nbox, c, t, n);
			put3(out.origin, o); put3(out.direction, d);
			out.phase = phase; out.cast = cast;
		}
		++count;
	}
};

template <class T, class M>
bool mover_cast(const Rec* rec, uint32_t n, uint32_t nbox, const M& w, nh_f3 o, nh_f3 d, const uint32_t* words, uint32_t mask, float& bt, uint32_t& bc, nh_f3& bn) {
	return closest_hit(rec, n, nbox, T::shape(w), o, d, 1.0f, w.ignore_body, words, mask, -1, bt, bc, bn);
}

// ---- move ----------------------------------------------------------------------------------------------------------------------------------------
template <class T>
void move_one(const Rec* rec, uint32_t n, uint32_t nbox, const typename T::Move& m, nh_MoveResult& out, Touches& touched, const uint32_t* words, uint32_t mask) {
	if (!T::valid(m)) {
		for (int k = 0; k < 3; ++k) { out.position[k] = m.origin[k]; out.remaining[k] = m.displacement[k]; }
		out.flags = NH_MOVE_INVALID; out.slides = 0u;
		write_ray_miss(out.last_hit, false, 1.0f);
		return;
	}
	nh_QMove s = nh_q_move_begin(v3(m.origin), v3(m.displacement));
	write_ray_miss(out.last_hit, true, 1.0f);
	for (uint32_t round = 0u; nh_q_move_go(s); ++round) {
		float bt; uint32_t bc; nh_f3 bn;
		const bool ok = mover_cast<T>(rec, n, nbox, m, s.p, s.v, words, mask, bt, bc, bn);
		write_cast(out.last_hit, rec, nbox, ok, 1.0f, bt, bc, bn);
		if (bc != 0xffffffffu) touched.take(rec, nbox, bc, bt, bn, s.p, s.v, NH_TOUCH_SLIDE, round);
		if (!nh_q_move_advance(s, bc != 0xffffffffu, bt, bn, m.skin, m.max_slides)) break;
	}
	put3(out.position, s.p); put3(out.remaining, s.v);
	out.flags = s.flags; out.slides = s.slides;
}

// ---- walk ----------------------------------------------------------------------------------------------------------------------------------------
template <class W_> nh_QWalkIn walk_in(const W_& w) {
	nh_QWalkIn W;
	W.origin = v3(w.origin); W.disp = v3(w.displacement); W.up = v3(w.up);
	W.skin = w.skin; W.step_height = w.step_height; W.snap = w.snap_distance; W.mgu = w.min_ground_up;
	W.max_slides = w.max_slides; W.options = w.options;
	return W;
}

void write_walk_hit(nh_RayHit& out, const Rec* rec, uint32_t nbox, const nh_QWalkHit& h) {
	if (h.c == NH_Q_WALK_NOBODY) { write_ray_miss(out, true, h.t); return; }
	write_ray_hit(out, rec, nbox, h.c, h.t, h.n);
}

template <class T>
void walk_one(const Rec* rec, uint32_t n, uint32_t nbox, const typename T::Walk& w, nh_WalkResult& out, Touches& touched, const uint32_t* words, uint32_t mask) {
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
		if (bc != 0xffffffffu) touched.take(rec, nbox, bc, bt, bn, s.m.p, s.m.v, nh_q_walk_touch_phase(s.phase), s.casts);
		nh_q_walk_advance(s, W, bc != 0xffffffffu, bt, bc, bn, ok);
	}
	put3(out.position, s.kp); put3(out.remaining, s.kv);
	out.flags = s.kflags; out.slides = s.kslides;
	out.step_up = s.step_up; out.drop = nh_q_walk_drop(s, W); out.casts = s.casts; out.reserved = 0u;
	write_walk_hit(out.last_hit, rec, nbox, s.klast);
	write_walk_hit(out.ground, rec, nbox, nh_q_walk_ground(s));
}

// every record of a batch: record i owns touches[i * k ..] and counts[i]
template <class In, class Out, class One>
void all(const void* in_, uint32_t count, Out* results, uint32_t k, uint32_t* counts, nh_Touch* touches, const uint32_t* masks, uint32_t mask, uint32_t threads, One one) {
	const In* in = (const In*)in_;
	parallel(count, threads, [=](uint32_t i) {
		Touches touched = { touches + (size_t)i * k, k, 0u };
		one(in[i], results[i], touched, masks ? masks[i] : mask);
		counts[i] = touched.count;
	});
}

template <class T>
void move_all(const Rec* rec, uint32_t n, uint32_t nbox, const void* moves, uint32_t count, nh_MoveResult* results, uint32_t k, uint32_t* counts, nh_Touch* touches,
              const uint32_t* words, const uint32_t* masks, uint32_t mask, uint32_t threads) {
	all<typename T::Move>(moves, count, results, k, counts, touches, masks, mask, threads,
		[=](const typename T::Move& m, nh_MoveResult& out, Touches& touched, uint32_t mk) { move_one<T>(rec, n, nbox, m, out, touched, words, mk); });
}

template <class T>
void walk_all(const Rec* rec, uint32_t n, uint32_t nbox, const void* walks, uint32_t count, nh_WalkResult* results, uint32_t k, uint32_t* counts, nh_Touch* touches,
              const uint32_t* words, const uint32_t* masks, uint32_t mask, uint32_t threads) {
	all<typename T::Walk>(walks, count, results, k, counts, touches, masks, mask, threads,
		[=](const typename T::Walk& w, nh_WalkResult& out, Touches& touched, uint32_t mk) { walk_one<T>(rec, n, nbox, w, out, touched, words, mk); });
}

}

extern "C" {

// shape: NH_SHAPE_CAPSULE or NH_SHAPE_BOX, with the shape's own records.  words: one layer word per collider, or NULL; masks: one mask per record, or NULL
// (every record uses `mask`).  touches: count * k records, of which record i's first min(counts[i], k) are written
void ht_move(uint32_t shape, const Rec* rec, uint32_t n, uint32_t nbox, const void* moves, uint32_t count, nh_MoveResult* results, uint32_t k, uint32_t* counts,
             nh_Touch* touches, const uint32_t* words, const uint32_t* masks, uint32_t mask, uint32_t threads) {
	if (shape == NH_SHAPE_BOX) move_all<BoxMover>(rec, n, nbox, moves, count, results, k, counts, touches, words, masks, mask, threads);
	else move_all<CapsuleMover>(rec, n, nbox, moves, count, results, k, counts, touches, words, masks, mask, threads);
}

void ht_walk(uint32_t shape, const Rec* rec, uint32_t n, uint32_t nbox, const void* walks, uint32_t count, nh_WalkResult* results, uint32_t k, uint32_t* counts,
             nh_Touch* touches, const uint32_t* words, const uint32_t* masks, uint32_t mask, uint32_t threads) {
	if (shape == NH_SHAPE_BOX) walk_all<BoxMover>(rec, n, nbox, walks, count, results, k, counts, touches, words, masks, mask, threads);
	else walk_all<CapsuleMover>(rec, n, nbox, walks, count, results, k, counts, touches, words, masks, mask, threads);
}

}
