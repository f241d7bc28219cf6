// hostsweep.cpp -- CPU build of the sphere-cast arithmetic of nudge_amd/csrc/nh_query.h, the oracle of the GPU's nh_spherecast (tests/hostsweep_util.py).
//   hs_spherecast  closest hit (or the hit of one collider) by brute force over all colliders, with the header's exact rules -- invalid casts,
//                  ignore_body, ties, the reach rule for r > 0 (the leaf box rebuilt as the build stores it) -- on several threads
//   hs_*           the single-collider predicates alone
#include "oracle.h"

static void cast_one(const Rec* rec, uint32_t n, uint32_t nbox, const nh_SphereCast& sc, nh_RayHit& out, int64_t only) {
	const nh_f3 o = v3(sc.origin), d = v3(sc.direction);
	const float r = sc.radius;
	const bool ok = finite(o.x) && finite(o.y) && finite(o.z) && finite(d.x) && finite(d.y) && finite(d.z) && finite(r) && !(r < 0.0f);
	const nh_f3 inv = nh_make3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
	const float w = r + nh_q_cast_pad(o, r);
	float bt = sc.max_t; uint32_t bc = 0xffffffffu; nh_f3 bn = nh_make3(0.0f, 0.0f, 0.0f);
	const uint32_t c0 = only >= 0 ? (uint32_t)only : 0u, c1 = only >= 0 ? (uint32_t)only + 1u : n;
	for (uint32_t c = ok ? c0 : c1; c < c1; ++c) {
		const Rec& e = rec[c];
		if (e.body == sc.ignore_body) continue;
		const bool box = c < nbox;
		const nh_f3 p = rec_pos(e), h = rec_half(e);
		const nh_quat q = rec_rot(e);
		nh_QHit hit = box ? nh_q_sweep_box(o, d, r, p, q, h) : nh_q_sweep_sphere(o, d, r, p, h.x);
		if (!hit.hit) continue;
		if (r > 0.0f) {
			// the reach rule: the leaf box must be entered, and the hit is no earlier than that entry
			nh_f3 lo, hi;
			nh_q_leaf_box(p, q, h, box, lo, hi);
			float t0;
			if (!nh_q_cast_node(lo, hi, o, inv, w, t0)) continue;
			if (t0 > hit.t) hit.t = t0;
		}
		if (nh_q_better(hit.t, c, sc.max_t, bt, bc)) { bt = hit.t; bc = c; bn = hit.n; }
	}
	if (bc == 0xffffffffu) write_ray_miss(out, ok, sc.max_t);
	else write_ray_hit(out, rec, nbox, bc, bt, bn);
}

extern "C" {

// only >= 0: the answer of that one collider (combined index) alone, as the closest-hit rule would give it
void hs_spherecast(const Rec* rec, uint32_t n, uint32_t nbox, const nh_SphereCast* casts, uint32_t count, nh_RayHit* hits, int64_t only, uint32_t threads) {
	parallel(count, threads, [=](uint32_t i) { cast_one(rec, n, nbox, casts[i], hits[i], only); });
}

// one collider alone, the predicate without the reach rule (the geometry tests): out = t, normal[3], hit (1.0 / 0.0)
void hs_sweep_box(const float o[3], const float d[3], float r, const float p[3], const float q[4], const float h[3], float out[5]) {
	out5(nh_q_sweep_box(v3(o), v3(d), r, v3(p), q4(q), v3(h)), out);
}

void hs_sweep_sphere(const float o[3], const float d[3], float r, const float c[3], float R, float out[5]) {
	out5(nh_q_sweep_sphere(v3(o), v3(d), r, v3(c), R), out);
}

}
