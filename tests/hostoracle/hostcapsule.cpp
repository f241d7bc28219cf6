// hostcapsule.cpp -- CPU build of the capsule arithmetic of nudge_amd/csrc/nh_query.h, the oracle of the GPU's nh_capsulecast (tests/hostcapsule_util.py).
// nh_overlap's capsule queries are judged by hostoverlap.cpp's hc_overlap.
//   hc_capsulecast  closest hit (or the hit of one collider) by brute force over all colliders, with the header's exact rules -- invalid casts,
//                   hh = 0 as a sphere cast, ignore_body, ties, the reach rule unless r = hh = 0 (the leaf box rebuilt as the build stores it)
//   hc_*            the single-collider predicates alone
#include "oracle.h"

static void cast_one(const Rec* rec, uint32_t n, uint32_t nbox, const nh_CapsuleCast& cc, nh_RayHit& out, int64_t only) {
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
	const uint32_t c0 = only >= 0 ? (uint32_t)only : 0u, c1 = only >= 0 ? (uint32_t)only + 1u : n;
	for (uint32_t c = ok ? c0 : c1; c < c1; ++c) {
		const Rec& rc = rec[c];
		if (rc.body == cc.ignore_body) continue;
		const bool box = c < nbox;
		const nh_f3 p = rec_pos(rc), h = rec_half(rc);
		const nh_quat q = rec_rot(rc);
		nh_QHit hit = box ? nh_q_sweep_capsule_box(o, d, qa, r, hh, p, q, h) : nh_q_sweep_capsule_sphere(o, d, qa, r, hh, p, h.x);
		if (!hit.hit) continue;
		if (reach) {
			// the reach rule: the leaf box must be entered, and the hit is no earlier than that entry
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

extern "C" {

// only >= 0: the answer of that one collider (combined index) alone, as the closest-hit rule would give it
void hc_capsulecast(const Rec* rec, uint32_t n, uint32_t nbox, const nh_CapsuleCast* casts, uint32_t count, nh_RayHit* hits, int64_t only, uint32_t threads) {
	parallel(count, threads, [=](uint32_t i) { cast_one(rec, n, nbox, casts[i], hits[i], only); });
}

// one collider alone, the predicate without the reach rule (the geometry tests): out = t, normal[3], hit (1.0 / 0.0)
void hc_sweep_capsule_box(const float o[3], const float d[3], const float q[4], float r, float hh, const float p[3], const float qb[4], const float hb[3], float out[5]) {
	out5(nh_q_sweep_capsule_box(v3(o), v3(d), q4(q), r, hh, v3(p), q4(qb), v3(hb)), out);
}

void hc_sweep_capsule_sphere(const float o[3], const float d[3], const float q[4], float r, float hh, const float c[3], float R, float out[5]) {
	out5(nh_q_sweep_capsule_sphere(v3(o), v3(d), q4(q), r, hh, v3(c), R), out);
}

int hc_overlap_capsule_box(const float c[3], const float q[4], float r, float hh, const float p[3], const float qb[4], const float hb[3]) {
	return nh_q_overlap_capsule_box(v3(c), q4(q), r, hh, v3(p), q4(qb), v3(hb)) ? 1 : 0;
}

int hc_overlap_capsule_sphere(const float c[3], const float q[4], float r, float hh, const float p[3], float R) {
	return nh_q_overlap_capsule_sphere(v3(c), q4(q), r, hh, v3(p), R) ? 1 : 0;
}

// the capsule's half axis a = rotate(q, (0, hh, 0)) as the predicates compute it
void hc_capsule_axis(const float q[4], float hh, float out[3]) {
	const nh_f3 a = nh_q_capsule_axis(q4(q), hh);
	out[0] = a.x; out[1] = a.y; out[2] = a.z;
}

}
