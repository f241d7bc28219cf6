// hostcapsule.cpp -- CPU build of the capsule arithmetic of nudge_amd/csrc/nh_query.h, the oracle of the GPU's nh_capsulecast (tests/hostcapsule_util.py).
// nh_overlap's capsule queries are judged by hostoverlap.cpp's hc_overlap.
//   hc_capsulecast  closest hit (or the hit of one collider) by brute force over all colliders (oracle.h's closest_hit of a SweptCapsule), with the header's
//                   exact rules -- invalid casts, hh = 0 as a sphere cast, ignore_body, ties, the reach rule unless r = hh = 0 (the leaf box rebuilt as
//                   the build stores it)
//   hc_*            the single-collider predicates alone
#include "oracle.h"

extern "C" {

// only >= 0: the answer of that one collider (combined index) alone, as the closest-hit rule would give it
void hc_capsulecast(const Rec* rec, uint32_t n, uint32_t nbox, const nh_CapsuleCast* casts, uint32_t count, nh_RayHit* hits, int64_t only, uint32_t threads) {
	parallel(count, threads, [=](uint32_t i) {
		const nh_CapsuleCast& cc = casts[i];
		float bt; uint32_t bc; nh_f3 bn;
		const bool ok = closest_hit(rec, n, nbox, SweptCapsule{ q4(cc.rotation), cc.radius, cc.half_height }, v3(cc.origin), v3(cc.direction), cc.max_t, cc.ignore_body, nullptr, 0u, only, bt, bc, bn);
		write_cast(hits[i], rec, nbox, ok, cc.max_t, bt, bc, bn);
	});
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
