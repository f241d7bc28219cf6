// hostwalk.cpp -- CPU build of nh_walk (include/nudge_hip.h): the phase machine of nudge_amd/csrc/nh_query.h, "walk", around a brute-force capsule cast,
// the oracle of the GPU's k_q_walk (tests/hostwalk_util.py).
//   hw_walk            every walk by brute force: each cast is hostcapsule.cpp's closest-hit cast (the same rules, mirrored here as hostmove.cpp mirrors them)
//                      of the record { p, 1, v, ignore_body, rotation, radius, half_height } over all colliders, under the masked world of the header
//                      (words / masks given: done here per walk, without a copy of the records)
//   hw_replay_*        the phases of a walk one at a time, for the REPLAY identity: the caller makes nh_move calls for A, U, F and D and an nh_capsulecast
//                      call for C, and these keep nh_q_walk_phase_end / nh_q_walk_advance between them
//   hw_steep           is a hit normal steep for a walk? (nh_q_walk_walkable), for the replay's `blocked`
#include "oracle.h"

static nh_QWalkIn walk_in(const nh_Walk& w) {
	nh_QWalkIn W;
	W.origin = v3(w.origin); W.disp = v3(w.displacement); W.up = v3(w.up);
	W.skin = w.skin; W.step_height = w.step_height; W.snap = w.snap_distance; W.mgu = w.min_ground_up;
	W.max_slides = w.max_slides; W.options = w.options;
	return W;
}

// hostmove.cpp's move_cast, answering with the combined index: (bt, bc, bn) as nh_q_cast_one leaves them, and whether the cast was valid
static bool walk_cast(const Rec* rec, uint32_t n, uint32_t nbox, const nh_Walk& wk, nh_f3 o, nh_f3 d, const uint32_t* words, uint32_t mask, float& bt, uint32_t& bc, nh_f3& bn) {
	const nh_quat qa = q4(wk.rotation);
	const float r = wk.radius, hh = wk.half_height;
	const bool ok = finite(o.x) && finite(o.y) && finite(o.z) && finite(d.x) && finite(d.y) && finite(d.z) && finite(r) && finite(hh) && !(r < 0.0f) &&
	                !(hh < 0.0f) && (hh == 0.0f || (finite(qa.x) && finite(qa.y) && finite(qa.z) && finite(qa.s)));
	const nh_f3 inv = nh_make3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
	const nh_f3 e = nh_q_capsule_extent(nh_q_capsule_axis(qa, hh), r);
	const float s = nh_q_cast_pad(o, fmaxf(fmaxf(e.x, e.y), e.z));
	const nh_f3 w = nh_make3(e.x + s, e.y + s, e.z + s);
	const bool reach = r > 0.0f || hh > 0.0f;
	bt = 1.0f; bc = 0xffffffffu; bn = nh_make3(0.0f, 0.0f, 0.0f);
	for (uint32_t c = ok ? 0u : n; c < n; ++c) {
		const Rec& rc = rec[c];
		if (rc.body == wk.ignore_body) continue;
		if (words && !(words[c] & mask)) continue;
		const bool box = c < nbox;
		const nh_f3 p = rec_pos(rc), h = rec_half(rc);
		const nh_quat q = rec_rot(rc);
		nh_QHit hit = box ? nh_q_sweep_capsule_box(o, d, qa, r, hh, p, q, h) : nh_q_sweep_capsule_sphere(o, d, qa, r, hh, p, h.x);
		if (!hit.hit) continue;
		if (reach) {
			nh_f3 lo, hi;
			nh_q_leaf_box(p, q, h, box, lo, hi);
			float t0;
			if (!nh_q_cast_node3(lo, hi, o, inv, w, t0)) continue;
			if (t0 > hit.t) hit.t = t0;
		}
		if (nh_q_better(hit.t, c, 1.0f, bt, bc)) { bt = hit.t; bc = c; bn = hit.n; }
	}
	return ok;
}

// a state's hit as its nh_RayHit: a collider by its combined index, or the miss record (t = 1, or NaN where the cast was invalid: the state holds either)
static void write_walk_hit(nh_RayHit& out, const Rec* rec, uint32_t nbox, const nh_QWalkHit& h) {
	if (h.c == NH_Q_WALK_NOBODY) { write_ray_miss(out, true, h.t); return; }
	write_ray_hit(out, rec, nbox, h.c, h.t, h.n);
}

static void write_invalid(const nh_Walk& w, nh_WalkResult& out) {
	for (int k = 0; k < 3; ++k) { out.position[k] = w.origin[k]; out.remaining[k] = w.displacement[k]; }
	out.flags = NH_WALK_INVALID; out.slides = 0u; out.step_up = 0.0f; out.drop = 0.0f; out.casts = 0u; out.reserved = 0u;
	write_ray_miss(out.last_hit, false, 1.0f);
	write_ray_miss(out.ground, false, 1.0f);
}

static void write_head(const nh_QWalk& s, const nh_QWalkIn& W, nh_WalkResult& out) {
	out.position[0] = s.kp.x; out.position[1] = s.kp.y; out.position[2] = s.kp.z;
	out.remaining[0] = s.kv.x; out.remaining[1] = s.kv.y; out.remaining[2] = s.kv.z;
	out.flags = s.kflags; out.slides = s.kslides;
	out.step_up = s.step_up; out.drop = nh_q_walk_drop(s, W); out.casts = s.casts; out.reserved = 0u;
}

static void walk_one(const Rec* rec, uint32_t n, uint32_t nbox, const nh_Walk& w, nh_WalkResult& out, const uint32_t* words, uint32_t mask) {
	const nh_QWalkIn W = walk_in(w);
	if (!nh_q_walk_valid(W, q4(w.rotation), w.radius, w.half_height)) { write_invalid(w, out); return; }
	nh_QWalk s = nh_q_walk_begin(W);
	while (nh_q_walk_cast(s, W)) {
		float bt; uint32_t bc; nh_f3 bn;
		const bool ok = walk_cast(rec, n, nbox, w, s.m.p, s.m.v, words, mask, bt, bc, bn);
		nh_q_walk_advance(s, W, bc != 0xffffffffu, bt, bc, bn, ok);
	}
	write_head(s, W, out);
	write_walk_hit(out.last_hit, rec, nbox, s.klast);
	write_walk_hit(out.ground, rec, nbox, nh_q_walk_ground(s));
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

extern "C" {

// words: one layer word per collider, or NULL; masks: one mask per walk, or NULL (every walk uses `mask`)
void hw_walk(const Rec* rec, uint32_t n, uint32_t nbox, const nh_Walk* walks, uint32_t count, nh_WalkResult* results, const uint32_t* words,
             const uint32_t* masks, uint32_t mask, uint32_t threads) {
	parallel(count, threads, [=](uint32_t i) { walk_one(rec, n, nbox, walks[i], results[i], words, masks ? masks[i] : mask); });
}

uint32_t hw_replay_state_size() { return (uint32_t)sizeof(ReplayState); }

// begin: the state of every walk before A (invalid records are not the phase machine's: the caller leaves them out)
void hw_replay_begin(const nh_Walk* walks, uint32_t count, ReplayState* st) {
	for (uint32_t i = 0; i < count; ++i) {
		st[i].s = nh_q_walk_begin(walk_in(walks[i]));
		for (int k = 0; k < 8; ++k) write_ray_miss(st[i].rec[k], true, 1.0f);
	}
}

// the nh_Move records of the phase `phase` (NH_Q_WALK_A, _U, _F, _D): for a walk in that phase its running loop { p, v, the phase's slides }, active = 1; for
// any other a record that moves nowhere, active = 0
void hw_replay_moves(const nh_Walk* walks, uint32_t count, const ReplayState* st, uint32_t phase, nh_Move* moves, uint32_t* active) {
	for (uint32_t i = 0; i < count; ++i) {
		const nh_Walk& w = walks[i];
		const nh_QWalk& s = st[i].s;
		nh_Move& m = moves[i];
		active[i] = (s.phase == phase || (phase == NH_Q_WALK_A && s.phase == NH_Q_WALK_AB)) ? 1u : 0u;
		for (int k = 0; k < 3; ++k) { m.origin[k] = w.origin[k]; m.displacement[k] = 0.0f; }
		for (int k = 0; k < 4; ++k) m.rotation[k] = w.rotation[k];
		m.skin = w.skin; m.ignore_body = w.ignore_body; m.radius = w.radius; m.half_height = w.half_height; m.max_slides = 0u; m.reserved = 0u;
		if (!active[i]) continue;
		m.origin[0] = s.m.p.x; m.origin[1] = s.m.p.y; m.origin[2] = s.m.p.z;
		m.displacement[0] = s.m.v.x; m.displacement[1] = s.m.v.y; m.displacement[2] = s.m.v.z;
		m.max_slides = nh_q_walk_slides(s, walk_in(w));
	}
}

// behind the nh_move call of a phase: for every active walk the loop's end as nh_move wrote it, then nh_q_walk_phase_end.  blocked (phase A only): whether a
// taken hit of A was steep.  The casts a move made: one per hit taken, and the last one where it ended in a miss or a start overlap.
void hw_replay_phase(const nh_Walk* walks, uint32_t count, ReplayState* st, uint32_t phase, const uint32_t* active, const nh_MoveResult* res, const uint32_t* blocked) {
	for (uint32_t i = 0; i < count; ++i) {
		if (!active[i]) continue;
		nh_QWalk& s = st[i].s;
		const nh_QWalkIn W = walk_in(walks[i]);
		const nh_MoveResult& r = res[i];
		const bool went = nh_q_move_go(s.m);
		s.m.p = v3(r.position); s.m.v = v3(r.remaining); s.m.slides = r.slides; s.m.flags = r.flags;
		s.last = replay_hit(r.last_hit, phase);
		st[i].rec[phase] = r.last_hit;
		// the casts nh_move made, from its result: every taken hit is one (slides).  The loop then ended in one of these ways:
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

// the nh_CapsuleCast records of the probes: for a walk in phase C { p, 1, v, ... }, active = 1; for any other its first cast, active = 0
void hw_replay_casts(const nh_Walk* walks, uint32_t count, const ReplayState* st, nh_CapsuleCast* casts, uint32_t* active) {
	for (uint32_t i = 0; i < count; ++i) {
		const nh_Walk& w = walks[i];
		const nh_QWalk& s = st[i].s;
		nh_CapsuleCast& c = casts[i];
		active[i] = s.phase == NH_Q_WALK_C ? 1u : 0u;
		const nh_f3 o = active[i] ? s.m.p : v3(w.origin), d = active[i] ? s.m.v : v3(w.displacement);
		c.origin[0] = o.x; c.origin[1] = o.y; c.origin[2] = o.z; c.max_t = 1.0f;
		c.direction[0] = d.x; c.direction[1] = d.y; c.direction[2] = d.z; c.ignore_body = w.ignore_body;
		for (int k = 0; k < 4; ++k) c.rotation[k] = w.rotation[k];
		c.radius = w.radius; c.half_height = w.half_height; c.reserved[0] = c.reserved[1] = 0u;
	}
}

// behind the nh_capsulecast call of the probes: nh_q_walk_advance with each active walk's record (an invalid cast wrote the miss record with t = NaN)
void hw_replay_probe(const nh_Walk* walks, uint32_t count, ReplayState* st, const uint32_t* active, const nh_RayHit* hits) {
	for (uint32_t i = 0; i < count; ++i) {
		if (!active[i]) continue;
		const nh_RayHit& h = hits[i];
		st[i].rec[NH_Q_WALK_C] = h;
		const bool hit = h.shape != NH_SHAPE_NONE;
		nh_q_walk_advance(st[i].s, walk_in(walks[i]), hit, hit ? h.t : 1.0f, NH_Q_WALK_C, v3(h.normal), hit || h.t == h.t);
	}
}

// the nh_WalkResult records of the replayed walks; left: how many have not ended
uint32_t hw_replay_finish(const nh_Walk* walks, uint32_t count, const ReplayState* st, nh_WalkResult* results) {
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

// steep[i] = 1 where hits[i] is a taken hit (a collider, t > 0) whose normal is not walkable for walks[i]
void hw_steep(const nh_Walk* walks, uint32_t count, const nh_RayHit* hits, uint32_t* steep) {
	for (uint32_t i = 0; i < count; ++i)
		steep[i] = (hits[i].shape != NH_SHAPE_NONE && hits[i].t != 0.0f && !nh_q_walk_walkable(v3(hits[i].normal), walk_in(walks[i]))) ? 1u : 0u;
}

}
