// hostboxwalk.cpp -- CPU build of nh_boxwalk (include/nudge_hip.h): the phase machine of nudge_amd/csrc/nh_query.h, "walk", around hostboxmove.cpp's
// brute-force box cast, the oracle of the GPU's k_q_walk<nh_QBox, .> (tests/hostboxwalk_util.py).
//   hbw_walk     every walk by brute force: each cast is the record { p, 1, v, ignore_body, rotation, size } over all colliders, under the masked world of
//                the header (words / masks given: done here per walk, without a copy of the records)
// The REPLAY identity needs nothing here: hostwalk.cpp's phase-by-phase helpers read only the rules of a walk, never its shape, and
// tests/hostboxwalk_util.py hands them callables that answer their move and cast records for a box.
#include "oracle.h"

bool hbm_cast(const Rec* rec, uint32_t n, uint32_t nbox, nh_f3 o, nh_f3 d, uint32_t ignore_body, nh_quat qa, nh_f3 ha, const uint32_t* words, uint32_t mask,
              float& bt, uint32_t& bc, nh_f3& bn);

static nh_QWalkIn boxwalk_in(const nh_BoxWalk& w) {
	nh_QWalkIn W;
	W.origin = v3(w.origin); W.disp = v3(w.displacement); W.up = v3(w.up);
	W.skin = w.skin; W.step_height = w.step_height; W.snap = w.snap_distance; W.mgu = w.min_ground_up;
	W.max_slides = w.max_slides; W.options = w.options;
	return W;
}

// a state's hit as its nh_RayHit: a collider by its combined index, or the miss record (t = 1, or NaN where the cast was invalid: the state holds either)
static void write_boxwalk_hit(nh_RayHit& out, const Rec* rec, uint32_t nbox, const nh_QWalkHit& h) {
	if (h.c == NH_Q_WALK_NOBODY) { write_ray_miss(out, true, h.t); return; }
	write_ray_hit(out, rec, nbox, h.c, h.t, h.n);
}

static void boxwalk_one(const Rec* rec, uint32_t n, uint32_t nbox, const nh_BoxWalk& w, nh_WalkResult& out, const uint32_t* words, uint32_t mask) {
	const nh_QWalkIn W = boxwalk_in(w);
	if (!nh_q_boxwalk_valid(W, q4(w.rotation), v3(w.size))) {
		for (int k = 0; k < 3; ++k) { out.position[k] = w.origin[k]; out.remaining[k] = w.displacement[k]; }
		out.flags = NH_WALK_INVALID; out.slides = 0u; out.step_up = 0.0f; out.drop = 0.0f; out.casts = 0u; out.reserved = 0u;
		write_ray_miss(out.last_hit, false, 1.0f);
		write_ray_miss(out.ground, false, 1.0f);
		return;
	}
	nh_QWalk s = nh_q_walk_begin(W);
	while (nh_q_walk_cast(s, W)) {
		float bt; uint32_t bc; nh_f3 bn;
		const bool ok = hbm_cast(rec, n, nbox, s.m.p, s.m.v, w.ignore_body, q4(w.rotation), v3(w.size), words, mask, bt, bc, bn);
		nh_q_walk_advance(s, W, bc != 0xffffffffu, bt, bc, bn, ok);
	}
	out.position[0] = s.kp.x; out.position[1] = s.kp.y; out.position[2] = s.kp.z;
	out.remaining[0] = s.kv.x; out.remaining[1] = s.kv.y; out.remaining[2] = s.kv.z;
	out.flags = s.kflags; out.slides = s.kslides;
	out.step_up = s.step_up; out.drop = nh_q_walk_drop(s, W); out.casts = s.casts; out.reserved = 0u;
	write_boxwalk_hit(out.last_hit, rec, nbox, s.klast);
	write_boxwalk_hit(out.ground, rec, nbox, nh_q_walk_ground(s));
}

extern "C" {

// words: one layer word per collider, or NULL; masks: one mask per walk, or NULL (every walk uses `mask`)
void hbw_walk(const Rec* rec, uint32_t n, uint32_t nbox, const nh_BoxWalk* walks, uint32_t count, nh_WalkResult* results, const uint32_t* words,
              const uint32_t* masks, uint32_t mask, uint32_t threads) {
	parallel(count, threads, [=](uint32_t i) { boxwalk_one(rec, n, nbox, walks[i], results[i], words, masks ? masks[i] : mask); });
}

}
