// hostnearest.cpp -- the oracle of the GPU's nh_closest_k (tests/hostnearest_util.py).
//   hn_closest_k    the k nearest colliders by brute force: every collider evaluated as hostpoint.cpp's closest_one does (oracle.h's rec_point: the
//                   predicate, the leaf box rebuilt as the build stores it, the reach rule's key), ALL candidates sorted with std::sort under
//                   nh_q_closer's order, the first k taken.  It does not use nh_q_nearest_insert: the list under test is no part of its own oracle
//   hn_insert       a candidate stream through nh_q_nearest_insert (nudge_amd/csrc/nh_query.h) over storage with a given stride
#include <algorithm>
#include "oracle.h"

struct Cand { float key; uint32_t c; nh_QPoint h; };

static uint32_t closest_k_one(const Rec* rec, uint32_t n, uint32_t nbox, const nh_PointQuery& pq, uint32_t k, nh_PointHit* out) {
	const nh_f3 p = v3(pq.point);
	const float max_d = pq.max_distance;
	const bool ok = finite(p.x) && finite(p.y) && finite(p.z) && max_d >= 0.0f;
	std::vector<Cand> all;
	for (uint32_t c = 0; ok && c < n; ++c) {
		if (rec[c].body == pq.ignore_body) continue;
		float key;
		const nh_QPoint h = rec_point(rec[c], c < nbox, p, key);
		if (!(key <= max_d)) continue;                 // (a NaN key -- a NaN pose -- is no candidate either)
		all.push_back(Cand{ key, c, h });
	}
	std::sort(all.begin(), all.end(), [](const Cand& a, const Cand& b) { return a.key < b.key || (a.key == b.key && a.c < b.c); });
	const uint32_t m = all.size() < k ? (uint32_t)all.size() : k;
	for (uint32_t j = 0; j < k; ++j) {
		if (j < m) write_point_hit(out[j], rec, nbox, all[j].c, all[j].key, all[j].h);
		else write_point_miss(out[j], ok, max_d);
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
