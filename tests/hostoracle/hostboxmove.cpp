// hostboxmove.cpp -- CPU build of nh_boxmove (include/nudge_hip.h): the state machine of nudge_amd/csrc/nh_query.h, "move", around a brute-force box cast,
// the oracle of the GPU's k_q_move<nh_QBox, .> (tests/hostboxmove_util.py).
//   hbm_move      every move by brute force: each round's cast is hostboxcast.cpp's closest-hit cast (the same rules, mirrored here as hostmove.cpp mirrors
//                 the capsule cast: invalid casts, size 0 as a ray that does not read the rotation, ignore_body, ties, the reach rule for a nonzero size) of
//                 the record { p, 1, v, ignore_body, rotation, size } over all colliders, under the masked world of the header (words / masks given: done
//                 here per move, without a copy of the records)
//   hbm_begin     the state of every move before its first cast (hostmove.cpp's MoveState)
//   hbm_advance   one application of nh_q_move_advance to a state and a cast's record, for the REPLAY test
//   hbm_cast      the cast alone, by combined index, for hostboxwalk.cpp
#include "oracle.h"

// hostboxcast.cpp's cast_one with max_t = 1; `words`, `mask`: colliders whose word shares no bit with the mask do not exist for this cast (words = NULL: all
// are seen).  Leaves (bt, bc, bn) as nh_q_cast_one leaves them and returns whether the cast was valid.
bool hbm_cast(const Rec* rec, uint32_t n, uint32_t nbox, nh_f3 o, nh_f3 d, uint32_t ignore_body, nh_quat qa, nh_f3 ha, const uint32_t* words, uint32_t mask,
              float& bt, uint32_t& bc, nh_f3& bn) {
	const bool ray = ha.x == 0.0f && ha.y == 0.0f && ha.z == 0.0f;
	const bool ok = finite(o.x) && finite(o.y) && finite(o.z) && finite(d.x) && finite(d.y) && finite(d.z) && finite(ha.x) && finite(ha.y) && finite(ha.z) &&
	                !(ha.x < 0.0f) && !(ha.y < 0.0f) && !(ha.z < 0.0f) && (ray || (finite(qa.x) && finite(qa.y) && finite(qa.z) && finite(qa.s)));
	const nh_f3 inv = nh_make3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
	const nh_f3 e = ray ? nh_make3(0.0f, 0.0f, 0.0f) : nh_q_box_extent(qa, ha);
	const float s = nh_q_cast_pad(o, fmaxf(fmaxf(e.x, e.y), e.z));
	const nh_f3 w = nh_make3(e.x + s, e.y + s, e.z + s);
	bt = 1.0f; bc = 0xffffffffu; bn = nh_make3(0.0f, 0.0f, 0.0f);
	for (uint32_t c = ok ? 0u : n; c < n; ++c) {
		const Rec& r = rec[c];
		if (r.body == ignore_body) continue;
		if (words && !(words[c] & mask)) continue;
		const bool box = c < nbox;
		const nh_f3 p = rec_pos(r), h = rec_half(r);
		const nh_quat q = rec_rot(r);
		nh_QHit hit = box ? nh_q_sweep_box_box(o, d, qa, ha, p, q, h) : nh_q_sweep_box_sphere(o, d, qa, ha, p, h.x);
		if (!hit.hit) continue;
		if (!ray) {
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

static void boxmove_one(const Rec* rec, uint32_t n, uint32_t nbox, const nh_BoxMove& m, nh_MoveResult& out, const uint32_t* words, uint32_t mask, uint32_t* casts) {
	const nh_f3 o = v3(m.origin), d = v3(m.displacement);
	uint32_t made = 0u;
	if (!nh_q_boxmove_valid(o, d, q4(m.rotation), v3(m.size), m.skin, m.max_slides)) {
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
		const bool ok = hbm_cast(rec, n, nbox, s.p, s.v, m.ignore_body, q4(m.rotation), v3(m.size), words, mask, bt, bc, bn);
		if (bc == 0xffffffffu) write_ray_miss(out.last_hit, ok, 1.0f);
		else write_ray_hit(out.last_hit, rec, nbox, bc, bt, bn);
		++made;
		if (!nh_q_move_advance(s, bc != 0xffffffffu, bt, bn, m.skin, m.max_slides)) break;
	}
	out.position[0] = s.p.x; out.position[1] = s.p.y; out.position[2] = s.p.z;
	out.remaining[0] = s.v.x; out.remaining[1] = s.v.y; out.remaining[2] = s.v.z;
	out.flags = s.flags; out.slides = s.slides;
	if (casts) *casts = made;
}

// hostmove.cpp's MoveState (hostmove_util.STATE)
struct BoxMoveState { float p[3]; uint32_t slides; float v[3]; uint32_t flags; float d0[3]; uint32_t stopped; float np[3]; uint32_t pad; };
static_assert(sizeof(BoxMoveState) == 64, "BoxMoveState is hostmove_util.STATE");

extern "C" {

// words: one layer word per collider, or NULL; masks: one mask per move, or NULL (every move uses `mask`).  casts: the casts each move made, or NULL
void hbm_move(const Rec* rec, uint32_t n, uint32_t nbox, const nh_BoxMove* moves, uint32_t count, nh_MoveResult* results, const uint32_t* words,
              const uint32_t* masks, uint32_t mask, uint32_t* casts, uint32_t threads) {
	parallel(count, threads, [=](uint32_t i) { boxmove_one(rec, n, nbox, moves[i], results[i], words, masks ? masks[i] : mask, casts ? casts + i : nullptr); });
}

// begin: the state of moves[i] before its first cast; stopped = 1 where rule 1 ends it at once (the caller leaves invalid records out)
void hbm_begin(const nh_BoxMove* moves, uint32_t count, BoxMoveState* st) {
	for (uint32_t i = 0; i < count; ++i) {
		const nh_QMove s = nh_q_move_begin(v3(moves[i].origin), v3(moves[i].displacement));
		BoxMoveState& o = st[i];
		o.p[0] = s.p.x; o.p[1] = s.p.y; o.p[2] = s.p.z; o.v[0] = s.v.x; o.v[1] = s.v.y; o.v[2] = s.v.z;
		o.d0[0] = s.d0.x; o.d0[1] = s.d0.y; o.d0[2] = s.d0.z; o.np[0] = s.np.x; o.np[1] = s.np.y; o.np[2] = s.np.z;
		o.slides = s.slides; o.flags = s.flags; o.pad = 0u;
		o.stopped = nh_q_move_go(s) ? 0u : 1u;
	}
}

// advance: for every state that has not stopped, nh_q_move_advance with hits[i] (the record a box cast from st[i].p along st[i].v with max_t = 1 wrote), then
// rule 1; states that have stopped are left alone
void hbm_advance(const nh_BoxMove* moves, uint32_t count, BoxMoveState* st, const nh_RayHit* hits) {
	for (uint32_t i = 0; i < count; ++i) {
		BoxMoveState& o = st[i];
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
