// hostnearest.cpp -- the oracle of the GPU's nh_closest_k, built with g++ -ffp-contract=off (tests/hostnearest_util.py) so that every function returns
// the device's bits; loaded with ctypes.
//   hn_closest_k    the k nearest colliders by brute force: every collider evaluated exactly as tests/hostpoint/hostpoint.cpp's closest_one does (the
//                   predicate, the leaf box rebuilt as the build stores it, the reach rule's key), ALL candidates sorted with std::sort under
//                   nh_q_closer's order, the first k taken.  It does not use nh_q_nearest_insert: the list under test is no part of its own oracle
//   hn_insert       a candidate stream through nh_q_nearest_insert (nudge_amd/csrc/nh_query.h) over storage with a given stride
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include <thread>
#include <vector>
#include "../../include/nudge_hip.h"
#include "../../nudge_amd/csrc/nh_query.h"

// 12 words per collider (tests/hostquery_util.py REC, nh_query.hip's nh_QRec): position, bits(body), rotation, half extents | radius (x3), bits(tag)
struct Rec { float p[3]; uint32_t body; float q[4]; float h[3]; uint32_t tag; };

struct Cand { float key; uint32_t c; nh_QPoint h; };

static bool finite(float x) { return (nh_asuint(x) & 0x7f800000u) != 0x7f800000u; }

template <class F> static void parallel(uint32_t count, uint32_t threads, F f) {
	if (threads < 1) threads = 1;
	std::vector<std::thread> pool;
	for (uint32_t k = 0; k < threads; ++k) pool.emplace_back([=]() { for (uint32_t i = k; i < count; i += threads) f(i); });
	for (auto& t : pool) t.join();
}

static uint32_t closest_k_one(const Rec* rec, uint32_t n, uint32_t nbox, const nh_PointQuery& pq, uint32_t k, nh_PointHit* out) {
	const nh_f3 p = nh_make3(pq.point[0], pq.point[1], pq.point[2]);
	const float max_d = pq.max_distance;
	const bool ok = finite(p.x) && finite(p.y) && finite(p.z) && max_d >= 0.0f;
	std::vector<Cand> all;
	for (uint32_t c = 0; ok && c < n; ++c) {
		const Rec& rc = rec[c];
		if (rc.body == pq.ignore_body) continue;
		const bool box = c < nbox;
		const nh_f3 cp = nh_make3(rc.p[0], rc.p[1], rc.p[2]), ch = nh_make3(rc.h[0], rc.h[1], rc.h[2]);
		const nh_quat cq = { rc.q[0], rc.q[1], rc.q[2], rc.q[3] };
		const nh_QPoint h = box ? nh_q_point_box(p, cp, cq, ch) : nh_q_point_sphere(p, cp, ch.x);
		nh_f3 lo, hi;
		nh_q_leaf_box(cp, cq, ch, box, lo, hi);
		const float key = nh_q_point_key(h.d, nh_q_point_node(lo, hi, p));
		if (!(key <= max_d)) continue;                 // (a NaN key -- a NaN pose -- is no candidate either)
		all.push_back(Cand{ key, c, h });
	}
	std::sort(all.begin(), all.end(), [](const Cand& a, const Cand& b) { return a.key < b.key || (a.key == b.key && a.c < b.c); });
	const uint32_t m = all.size() < k ? (uint32_t)all.size() : k;
	for (uint32_t j = 0; j < k; ++j) {
		nh_PointHit& o = out[j];
		o.reserved = 0u;
		if (j < m) {
			const Cand& a = all[j];
			o.distance = a.key;
			o.normal[0] = a.h.n.x; o.normal[1] = a.h.n.y; o.normal[2] = a.h.n.z;
			o.point[0] = a.h.x.x; o.point[1] = a.h.x.y; o.point[2] = a.h.x.z;
			o.body = rec[a.c].body; o.collider = a.c < nbox ? a.c : a.c - nbox; o.shape = a.c < nbox ? NH_SHAPE_BOX : NH_SHAPE_SPHERE; o.tag = rec[a.c].tag;
		} else {
			o.distance = ok ? max_d : nh_asfloat(0x7fc00000u);
			o.normal[0] = o.normal[1] = o.normal[2] = 0.0f; o.point[0] = o.point[1] = o.point[2] = 0.0f;
			o.body = o.collider = o.tag = 0xffffffffu; o.shape = NH_SHAPE_NONE;
		}
	}
	return m;
}

extern "C" {

void hn_closest_k(const Rec* rec, uint32_t n, uint32_t nbox, const nh_PointQuery* queries, uint32_t count, uint32_t k, uint32_t* counts, nh_PointHit* hits,
                  uint32_t threads) {
	parallel(count, threads, [=](uint32_t i) { counts[i] = closest_k_one(rec, n, nbox, queries[i], k, hits + (size_t)i * k); });
}

// `count` candidates (keys[i], idx[i]) in their order through nh_q_nearest_insert; the list is slot j at store[j * stride] of (key, index) pairs (2 words
// each).  Returns the number held; changed[i] = what the i-th call returned.
uint32_t hn_insert(const float* keys, const uint32_t* idx, uint32_t count, uint32_t k, uint32_t stride, float max_d, uint32_t* store, uint8_t* changed) {
	uint32_t held = 0u;
	nh_QNear* base = reinterpret_cast<nh_QNear*>(store);
	for (uint32_t i = 0; i < count; ++i) changed[i] = nh_q_nearest_insert(base, stride, k, &held, keys[i], idx[i], max_d) ? 1 : 0;
	return held;
}

}
