// hostpoint.cpp -- CPU build of the closest-point arithmetic of nudge_amd/csrc/nh_query.h, the oracle of the GPU's nh_closest.  Built with
// g++ -ffp-contract=off (tests/hostpoint_util.py), so that every function returns the device's bits; loaded with ctypes.
//   hp_closest      the nearest collider (or the answer of one collider) by brute force over all colliders, with the header's exact rules -- invalid
//                   queries, ignore_body, max_distance, ties, the reach rule (the leaf box rebuilt as the build stores it)
//   hp_*            the single-collider predicates, the node distance and the key alone
#include <stdint.h>
#include <math.h>
#include <thread>
#include <vector>
#include "../../include/nudge_hip.h"
#include "../../nudge_amd/csrc/nh_query.h"

// 12 words per collider (tests/hostquery_util.py REC, nh_query.hip's nh_QRec): position, bits(body), rotation, half extents | radius (x3), bits(tag)
struct Rec { float p[3]; uint32_t body; float q[4]; float h[3]; uint32_t tag; };

static bool finite(float x) { return (nh_asuint(x) & 0x7f800000u) != 0x7f800000u; }

template <class F> static void parallel(uint32_t count, uint32_t threads, F f) {
	if (threads < 1) threads = 1;
	std::vector<std::thread> pool;
	for (uint32_t k = 0; k < threads; ++k) pool.emplace_back([=]() { for (uint32_t i = k; i < count; i += threads) f(i); });
	for (auto& t : pool) t.join();
}

static nh_QPoint point_of(const Rec& rc, bool box, nh_f3 p) {
	const nh_f3 c = nh_make3(rc.p[0], rc.p[1], rc.p[2]), h = nh_make3(rc.h[0], rc.h[1], rc.h[2]);
	const nh_quat q = { rc.q[0], rc.q[1], rc.q[2], rc.q[3] };
	return box ? nh_q_point_box(p, c, q, h) : nh_q_point_sphere(p, c, h.x);
}

static void closest_one(const Rec* rec, uint32_t n, uint32_t nbox, const nh_PointQuery& pq, nh_PointHit& out, int64_t only) {
	const nh_f3 p = nh_make3(pq.point[0], pq.point[1], pq.point[2]);
	const float max_d = pq.max_distance;
	const bool ok = finite(p.x) && finite(p.y) && finite(p.z) && max_d >= 0.0f;
	float bd = max_d; uint32_t bc = 0xffffffffu; nh_QPoint best = {};
	const uint32_t c0 = only >= 0 ? (uint32_t)only : 0u, c1 = only >= 0 ? (uint32_t)only + 1u : n;
	for (uint32_t c = ok ? c0 : c1; c < c1; ++c) {
		const Rec& rc = rec[c];
		if (rc.body == pq.ignore_body) continue;
		const bool box = c < nbox;
		const nh_QPoint h = point_of(rc, box, p);
		// the reach rule: the distance is at least that of the leaf box, where p lies outside it
		nh_f3 lo, hi;
		nh_q_leaf_box(nh_make3(rc.p[0], rc.p[1], rc.p[2]), nh_quat{ rc.q[0], rc.q[1], rc.q[2], rc.q[3] }, nh_make3(rc.h[0], rc.h[1], rc.h[2]), box, lo, hi);
		const float k = nh_q_point_key(h.d, nh_q_point_node(lo, hi, p));
		if (nh_q_closer(k, c, max_d, bd, bc)) { bd = k; bc = c; best = h; }
	}
	out.reserved = 0u;
	if (bc == 0xffffffffu) {
		out.distance = ok ? max_d : nh_asfloat(0x7fc00000u);
		out.normal[0] = out.normal[1] = out.normal[2] = 0.0f; out.point[0] = out.point[1] = out.point[2] = 0.0f;
		out.body = out.collider = out.tag = 0xffffffffu; out.shape = NH_SHAPE_NONE;
	} else {
		out.distance = bd;
		out.normal[0] = best.n.x; out.normal[1] = best.n.y; out.normal[2] = best.n.z;
		out.point[0] = best.x.x; out.point[1] = best.x.y; out.point[2] = best.x.z;
		out.body = rec[bc].body; out.collider = bc < nbox ? bc : bc - nbox; out.shape = bc < nbox ? NH_SHAPE_BOX : NH_SHAPE_SPHERE; out.tag = rec[bc].tag;
	}
}

static void out7(const nh_QPoint& r, float out[7]) { out[0] = r.d; out[1] = r.n.x; out[2] = r.n.y; out[3] = r.n.z; out[4] = r.x.x; out[5] = r.x.y; out[6] = r.x.z; }

extern "C" {

// only >= 0: the answer of that one collider (combined index) alone, as the nearest rule would give it
void hp_closest(const Rec* rec, uint32_t n, uint32_t nbox, const nh_PointQuery* queries, uint32_t count, nh_PointHit* hits, int64_t only, uint32_t threads) {
	parallel(count, threads, [=](uint32_t i) { closest_one(rec, n, nbox, queries[i], hits[i], only); });
}

// one collider alone, the predicate without the reach rule: out = distance, normal[3], point[3]
void hp_point_box(const float p[3], const float c[3], const float q[4], const float h[3], float out[7]) {
	out7(nh_q_point_box(nh_make3(p[0], p[1], p[2]), nh_make3(c[0], c[1], c[2]), nh_quat{ q[0], q[1], q[2], q[3] }, nh_make3(h[0], h[1], h[2])), out);
}

void hp_point_sphere(const float p[3], const float c[3], float R, float out[7]) {
	out7(nh_q_point_sphere(nh_make3(p[0], p[1], p[2]), nh_make3(c[0], c[1], c[2]), R), out);
}

// the walk's squared node distance, and the reach rule's key
float hp_point_node(const float lo[3], const float hi[3], const float p[3]) {
	return nh_q_point_node(nh_make3(lo[0], lo[1], lo[2]), nh_make3(hi[0], hi[1], hi[2]), nh_make3(p[0], p[1], p[2]));
}

float hp_point_key(float d, float d2) { return nh_q_point_key(d, d2); }

// the leaf box of a collider as the build stores it: out = lo[3], hi[3]
void hp_leaf_box(const float p[3], const float q[4], const float h[3], int box, float out[6]) {
	nh_f3 lo, hi;
	nh_q_leaf_box(nh_make3(p[0], p[1], p[2]), nh_quat{ q[0], q[1], q[2], q[3] }, nh_make3(h[0], h[1], h[2]), box != 0, lo, hi);
	out[0] = lo.x; out[1] = lo.y; out[2] = lo.z; out[3] = hi.x; out[4] = hi.y; out[5] = hi.z;
}

}
