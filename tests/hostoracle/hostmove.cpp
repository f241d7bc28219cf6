// hostmove.cpp -- CPU build of nh_move (include/nudge_hip.h): the state machine of nudge_amd/csrc/nh_query.h, "move", around a brute-force capsule cast,
// the oracle of the GPU's k_q_move (tests/hostmove_util.py).
//   hm_move     every move by brute force: each round's cast is hostcapsule.cpp's closest-hit cast (the same rules, mirrored here: invalid casts, hh = 0 as
//               a sphere cast, ignore_body, ties, the reach rule unless r = hh = 0) of the record { p, 1, v, ignore_body, rotation, radius, half_height }
//               over all colliders.  A layer filter is the masked world of the header: the caller passes records with a NaN position where the move's mask
//               sees nothing of the collider's word (words / masks given: done here per move, without a copy of the records)
//   hm_advance  one application of nh_q_move_advance to a state and a cast's record, for the REPLAY test
#include "oracle.h"

// hostcapsule.cpp's cast_one; `words`, `mask`: colliders whose word shares no bit with the mask do not exist for this cast (words = NULL: all are seen)
static void move_cast(const Rec* rec, uint32_t n, uint32_t nbox, const nh_CapsuleCast& cc, nh_RayHit& out, const uint32_t* words, uint32_t mask) {
	const nh_f3 o = v3(cc.origin), d = v3(cc.direction);
	const nh_quat qa = q4(cc.rotation);
	const float r = cc.radius, hh = cc.half_height;
	const bool ok = finite(o.x) && finite(o.y) && finite(o.z) && finite(d.x) && finite(d.y) && finite(d.z) && finite(r) && finite(hh) && !(r < 0.0f) &&
	                !(hh < 0.0f) && (hh == 0.0f || (finite(qa.x) && finite(qa.y) && finite(qa.z) && finite(qa.s)));
	const nh_f3 inv = nh_make3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
	const nh_f3 e = nh_q_capsule_extent(nh_q_capsule_axis(qa, hh), r);
	const float s = nh_q_cast_pad(o, fmaxf(fmaxf(e.x, e.y), e.z));
	const nh_f3 w = nh_make3(e.x + s, e.y + s, e.z + s);
	const bool reach = r > 0.0f || hh > 0.0f;
	float bt = cc.max_t; uint32_t bc = 0xffffffffu; nh_f3 bn = nh_make3(0.0f, 0.0f, 0.0f);
	for (uint32_t c = ok ? 0u : n; c < n; ++c) {
		const Rec& rc = rec[c];
		if (rc.body == cc.ignore_body) continue;
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
		if (nh_q_better(hit.t, c, cc.max_t, bt, bc)) { bt = hit.t; bc = c; bn = hit.n; }
	}
	if (bc == 0xffffffffu) write_ray_miss(out, ok, cc.max_t);
	else write_ray_hit(out, rec, nbox, bc, bt, bn);
}

static void move_one(const Rec* rec, uint32_t n, uint32_t nbox, const nh_Move& m, nh_MoveResult& out, const uint32_t* words, uint32_t mask, uint32_t* casts) {
	const nh_f3 o = v3(m.origin), d = v3(m.displacement);
	uint32_t made = 0u;
	if (!nh_q_move_valid(o, d, q4(m.rotation), m.radius, m.half_height, m.skin, m.max_slides)) {
		for (int k = 0; k < 3; ++k) { out.position[k] = m.origin[k]; out.remaining[k] = m.displacement[k]; }
		out.flags = NH_MOVE_INVALID; out.slides = 0u;
		write_ray_miss(out.last_hit, false, 1.0f);
		if (casts) *casts = 0u;
		return;
	}
	nh_QMove s = nh_q_move_begin(o, d);
	write_ray_miss(out.last_hit, true, 1.0f);
	while (nh_q_move_go(s)) {
		nh_CapsuleCast cc;
		cc.origin[0] = s.p.x; cc.origin[1] = s.p.y; cc.origin[2] = s.p.z; cc.max_t = 1.0f;
		cc.direction[0] = s.v.x; cc.direction[1] = s.v.y; cc.direction[2] = s.v.z; cc.ignore_body = m.ignore_body;
		for (int k = 0; k < 4; ++k) cc.rotation[k] = m.rotation[k];
		cc.radius = m.radius; cc.half_height = m.half_height; cc.reserved[0] = cc.reserved[1] = 0u;
		move_cast(rec, n, nbox, cc, out.last_hit, words, mask);
		++made;
		if (!nh_q_move_advance(s, out.last_hit.shape != NH_SHAPE_NONE, out.last_hit.t, v3(out.last_hit.normal), m.skin, m.max_slides)) break;
	}
	out.position[0] = s.p.x; out.position[1] = s.p.y; out.position[2] = s.p.z;
	out.remaining[0] = s.v.x; out.remaining[1] = s.v.y; out.remaining[2] = s.v.z;
	out.flags = s.flags; out.slides = s.slides;
	if (casts) *casts = made;
}

// The state of one move between two casts, as the REPLAY test keeps it: nh_QMove and whether the move has stopped
struct MoveState { float p[3]; uint32_t slides; float v[3]; uint32_t flags; float d0[3]; uint32_t stopped; float np[3]; uint32_t pad; };
static_assert(sizeof(MoveState) == 64, "MoveState is hostmove_util.STATE");

extern "C" {

// words: one layer word per collider, or NULL; masks: one mask per move, or NULL (every move uses `mask`).  casts: the casts each move made, or NULL
void hm_move(const Rec* rec, uint32_t n, uint32_t nbox, const nh_Move* moves, uint32_t count, nh_MoveResult* results, const uint32_t* words,
             const uint32_t* masks, uint32_t mask, uint32_t* casts, uint32_t threads) {
	parallel(count, threads, [=](uint32_t i) { move_one(rec, n, nbox, moves[i], results[i], words, masks ? masks[i] : mask, casts ? casts + i : nullptr); });
}

// begin: the state of moves[i] before its first cast; stopped = 1 where rule 1 ends it at once (an invalid record is not the state machine's: the caller
// leaves those out)
void hm_begin(const nh_Move* moves, uint32_t count, MoveState* st) {
	for (uint32_t i = 0; i < count; ++i) {
		const nh_QMove s = nh_q_move_begin(v3(moves[i].origin), v3(moves[i].displacement));
		MoveState& o = st[i];
		o.p[0] = s.p.x; o.p[1] = s.p.y; o.p[2] = s.p.z; o.v[0] = s.v.x; o.v[1] = s.v.y; o.v[2] = s.v.z;
		o.d0[0] = s.d0.x; o.d0[1] = s.d0.y; o.d0[2] = s.d0.z; o.np[0] = s.np.x; o.np[1] = s.np.y; o.np[2] = s.np.z;
		o.slides = s.slides; o.flags = s.flags; o.pad = 0u;
		o.stopped = nh_q_move_go(s) ? 0u : 1u;
	}
}

// advance: for every state that has not stopped, nh_q_move_advance with hits[i] (the record a capsule cast from st[i].p along st[i].v with max_t = 1 wrote),
// then rule 1; states that have stopped are left alone
void hm_advance(const nh_Move* moves, uint32_t count, MoveState* st, const nh_RayHit* hits) {
	for (uint32_t i = 0; i < count; ++i) {
		MoveState& o = st[i];
		if (o.stopped) continue;
		nh_QMove s;
		s.p = v3(o.p); s.v = v3(o.v); s.d0 = v3(o.d0); s.np = v3(o.np); s.slides = o.slides; s.flags = o.flags;
		const bool on = nh_q_move_advance(s, hits[i].shape != NH_SHAPE_NONE, hits[i].t, v3(hits[i].normal), moves[i].skin, moves[i].max_slides);
		o.p[0] = s.p.x; o.p[1] = s.p.y; o.p[2] = s.p.z; o.v[0] = s.v.x; o.v[1] = s.v.y; o.v[2] = s.v.z;
		o.np[0] = s.np.x; o.np[1] = s.np.y; o.np[2] = s.np.z;
		o.slides = s.slides; o.flags = s.flags;
		o.stopped = (on && nh_q_move_go(s)) ? 0u : 1u;
	}
}

}
