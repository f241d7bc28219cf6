// hostpoint.cpp -- CPU build of the closest-point arithmetic of nudge_amd/csrc/nh_query.h, the oracle of the GPU's nh_closest (tests/hostpoint_util.py).
//   hp_closest      the nearest collider (or the answer of one collider) by brute force over all colliders, with the header's exact rules -- invalid
//                   queries, ignore_body, max_distance, ties, the reach rule (oracle.h's rec_point)
//   hp_*            the single-collider predicates, the node distance and the key alone
#include "oracle.h"

static void closest_one(const Rec* rec, uint32_t n, uint32_t nbox, const nh_PointQuery& pq, nh_PointHit& out, int64_t only) {
	const nh_f3 p = v3(pq.point);
	const float max_d = pq.max_distance;
	const bool ok = finite(p.x) && finite(p.y) && finite(p.z) && max_d >= 0.0f;
	float bd = max_d; uint32_t bc = 0xffffffffu; nh_QPoint best = {};
	const uint32_t c0 = only >= 0 ? (uint32_t)only : 0u, c1 = only >= 0 ? (uint32_t)only + 1u : n;
	for (uint32_t c = ok ? c0 : c1; c < c1; ++c) {
		if (rec[c].body == pq.ignore_body) continue;
		float k;
		const nh_QPoint h = rec_point(rec[c], c < nbox, p, k);
		if (nh_q_closer(k, c, max_d, bd, bc)) { bd = k; bc = c; best = h; }
	}
	if (bc == 0xffffffffu) write_point_miss(out, ok, max_d);
	else write_point_hit(out, rec, nbox, bc, bd, best);
}

extern "C" {

// only >= 0: the answer of that one collider (combined index) alone, as the nearest rule would give it
void hp_closest(const Rec* rec, uint32_t n, uint32_t nbox, const nh_PointQuery* queries, uint32_t count, nh_PointHit* hits, int64_t only, uint32_t threads) {
	parallel(count, threads, [=](uint32_t i) { closest_one(rec, n, nbox, queries[i], hits[i], only); });
}

// one collider alone, the predicate without the reach rule: out = distance, normal[3], point[3]
void hp_point_box(const float p[3], const float c[3], const float q[4], const float h[3], float out[7]) { out7(nh_q_point_box(v3(p), v3(c), q4(q), v3(h)), out); }

void hp_point_sphere(const float p[3], const float c[3], float R, float out[7]) { out7(nh_q_point_sphere(v3(p), v3(c), R), out); }

// the walk's squared node distance, and the reach rule's key
float hp_point_node(const float lo[3], const float hi[3], const float p[3]) { return nh_q_point_node(v3(lo), v3(hi), v3(p)); }

float hp_point_key(float d, float d2) { return nh_q_point_key(d, d2); }

// the leaf box of a collider as the build stores it: out = lo[3], hi[3]
void hp_leaf_box(const float p[3], const float q[4], const float h[3], int box, float out[6]) {
	nh_f3 lo, hi;
	nh_q_leaf_box(v3(p), q4(q), v3(h), box != 0, lo, hi);
	out[0] = lo.x; out[1] = lo.y; out[2] = lo.z; out[3] = hi.x; out[4] = hi.y; out[5] = hi.z;
}

}
