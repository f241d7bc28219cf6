// hostboxcast.cpp -- CPU build of the box-cast arithmetic of nudge_amd/csrc/nh_query.h, the oracle of the GPU's nh_boxcast (tests/hostboxcast_util.py).
//   hb_boxcast     closest hit (or the hit of one collider) by brute force over all colliders, with the header's exact rules -- invalid casts,
//                  size 0 as a ray, ignore_body, ties, the reach rule for a nonzero size (the leaf box rebuilt as the build stores it) -- on several threads
//   hb_*           the single-collider predicates alone
#include "oracle.h"

static void cast_one(const Rec* rec, uint32_t n, uint32_t nbox, const nh_BoxCast& bc_, nh_RayHit& out, int64_t only) {
	const nh_f3 o = v3(bc_.origin), d = v3(bc_.direction);
	const nh_f3 ha = v3(bc_.size);
	const nh_quat qa = q4(bc_.rotation);
	const bool ray = ha.x == 0.0f && ha.y == 0.0f && ha.z == 0.0f;
	const bool ok = finite(o.x) && finite(o.y) && finite(o.z) && finite(d.x) && finite(d.y) && finite(d.z) && finite(ha.x) && finite(ha.y) && finite(ha.z) &&
	                !(ha.x < 0.0f) && !(ha.y < 0.0f) && !(ha.z < 0.0f) && (ray || (finite(qa.x) && finite(qa.y) && finite(qa.z) && finite(qa.s)));
	const nh_f3 inv = nh_make3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
	const nh_f3 e = ray ? nh_make3(0.0f, 0.0f, 0.0f) : nh_q_box_extent(qa, ha);
	const float s = nh_q_cast_pad(o, fmaxf(fmaxf(e.x, e.y), e.z));
	const nh_f3 w = nh_make3(e.x + s, e.y + s, e.z + s);
	float bt = bc_.max_t; uint32_t bc = 0xffffffffu; nh_f3 bn = nh_make3(0.0f, 0.0f, 0.0f);
	const uint32_t c0 = only >= 0 ? (uint32_t)only : 0u, c1 = only >= 0 ? (uint32_t)only + 1u : n;
	for (uint32_t c = ok ? c0 : c1; c < c1; ++c) {
		const Rec& r = rec[c];
		if (r.body == bc_.ignore_body) continue;
		const bool box = c < nbox;
		const nh_f3 p = rec_pos(r), h = rec_half(r);
		const nh_quat q = rec_rot(r);
		nh_QHit hit = box ? nh_q_sweep_box_box(o, d, qa, ha, p, q, h) : nh_q_sweep_box_sphere(o, d, qa, ha, p, h.x);
		if (!hit.hit) continue;
		if (!ray) {
			// the reach rule: the leaf box must be entered, and the hit is no earlier than that entry
			nh_f3 lo, hi;
			nh_q_leaf_box(p, q, h, box, lo, hi);
			float t0;
			if (!nh_q_cast_node3(lo, hi, o, inv, w, t0)) continue;
			if (t0 > hit.t) hit.t = t0;
		}
		if (nh_q_better(hit.t, c, bc_.max_t, bt, bc)) { bt = hit.t; bc = c; bn = hit.n; }
	}
	if (bc == 0xffffffffu) write_ray_miss(out, ok, bc_.max_t);
	else write_ray_hit(out, rec, nbox, bc, bt, bn);
}

extern "C" {

// only >= 0: the answer of that one collider (combined index) alone, as the closest-hit rule would give it
void hb_boxcast(const Rec* rec, uint32_t n, uint32_t nbox, const nh_BoxCast* casts, uint32_t count, nh_RayHit* hits, int64_t only, uint32_t threads) {
	parallel(count, threads, [=](uint32_t i) { cast_one(rec, n, nbox, casts[i], hits[i], only); });
}

// one collider alone, the predicate without the reach rule (the geometry tests): out = t, normal[3], hit (1.0 / 0.0)
void hb_sweep_box_box(const float o[3], const float d[3], const float qa[4], const float ha[3], const float p[3], const float qb[4], const float hb[3], float out[5]) {
	out5(nh_q_sweep_box_box(v3(o), v3(d), q4(qa), v3(ha), v3(p), q4(qb), v3(hb)), out);
}

void hb_sweep_box_sphere(const float o[3], const float d[3], const float qa[4], const float ha[3], const float c[3], float R, float out[5]) {
	out5(nh_q_sweep_box_sphere(v3(o), v3(d), q4(qa), v3(ha), v3(c), R), out);
}

}
