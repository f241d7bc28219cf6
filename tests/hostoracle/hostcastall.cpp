// hostcastall.cpp -- CPU build of the all-hits casts (nh_raycast_all / nh_spherecast_all of include/nudge_hip.h), the oracle of the GPU's chain
// (tests/hostcastall_util.py).
//   hc_castall  per cast, a brute force over all colliders in index order with the header's exact rules -- invalid casts, ignore_body, the reach rule
//               for r > 0 on the leaf box rebuilt as the build stores it, 0 <= t <= max_t -- then std::stable_sort by t over the index-ordered hits,
//               the offsets by an exclusive scan, the capacity prefix of whole segments and the overflow marker; on several threads
#include <algorithm>
#include "oracle.h"

struct Hit { float t; nh_f3 n; uint32_t c; };

// the hits of one cast, ordered; `out` == nullptr: the count alone
template <bool SWEEP>
static uint32_t cast_one(const Rec* rec, uint32_t n, uint32_t nbox, const void* cast, std::vector<Hit>* out) {
	const nh_Ray& ray = *static_cast<const nh_Ray*>(cast);          // (nh_SphereCast's first 32 bytes are nh_Ray's)
	const nh_f3 o = v3(ray.origin), d = v3(ray.direction);
	const float r = SWEEP ? static_cast<const nh_SphereCast*>(cast)->radius : 0.0f;
	bool ok = finite(o.x) && finite(o.y) && finite(o.z) && finite(d.x) && finite(d.y) && finite(d.z);
	if (SWEEP) ok = ok && finite(r) && !(r < 0.0f);
	if (!ok) return 0u;
	const nh_f3 inv = nh_make3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
	const float w = r + nh_q_cast_pad(o, r);
	uint32_t k = 0u;
	for (uint32_t c = 0u; c < n; ++c) {
		const Rec& e = rec[c];
		if (e.body == ray.ignore_body) continue;
		const bool box = c < nbox;
		const nh_f3 p = rec_pos(e), h = rec_half(e);
		const nh_quat q = rec_rot(e);
		float t0 = 0.0f;
		// the reach rule: the collider's own leaf box must be entered, and the hit is no earlier than that entry
		if (SWEEP && r > 0.0f && !nh_q_leaf_entry(o, inv, w, p, q, h, box, t0)) continue;
		const nh_QHit s = nh_q_all_hit<SWEEP>(o, d, r, ray.max_t, t0, p, q, h, box);
		if (!s.hit) continue;
		if (out) out->push_back(Hit{ s.t, s.n, c });
		++k;
	}
	// (float comparison: -0 equals +0; stable: equal t stay in index order)
	if (out) std::stable_sort(out->begin(), out->end(), [](const Hit& a, const Hit& b) { return a.t < b.t; });
	return k;
}

template <bool SWEEP>
static uint64_t castall(const Rec* rec, uint32_t n, uint32_t nbox, const uint8_t* casts, uint32_t count, uint32_t* offsets, nh_RayHit* hits,
                        uint32_t capacity, uint32_t threads) {
	const size_t stride = SWEEP ? sizeof(nh_SphereCast) : sizeof(nh_Ray);
	std::vector<uint32_t> counts(count);
	parallel(count, threads, [&](uint32_t i) { counts[i] = cast_one<SWEEP>(rec, n, nbox, casts + stride * i, nullptr); });
	uint64_t total = 0;
	for (uint32_t i = 0; i < count; ++i) { offsets[i] = (uint32_t)total; total += counts[i]; }
	offsets[count] = (uint32_t)total;
	if (total >= 0xffffffffull) { offsets[count] = 0xffffffffu; return total; }      // the marker: no record at all
	if (!hits || !capacity) return total;
	parallel(count, threads, [&](uint32_t i) {
		if (!(offsets[i + 1] <= capacity) || !counts[i]) return;      // whole segments that fit
		std::vector<Hit> found;
		cast_one<SWEEP>(rec, n, nbox, casts + stride * i, &found);
		for (uint32_t j = 0; j < found.size(); ++j) write_ray_hit(hits[offsets[i] + j], rec, nbox, found[j].c, found[j].t, found[j].n);
	});
	return total;
}

extern "C" {

// offsets: count + 1 words, always written; hits: `capacity` records or null (count only), written for the segments that fit and left alone
// elsewhere.  Returns the true total.
uint64_t hc_raycast_all(const Rec* rec, uint32_t n, uint32_t nbox, const nh_Ray* rays, uint32_t count, uint32_t* offsets, nh_RayHit* hits, uint32_t capacity,
                        uint32_t threads) {
	return castall<false>(rec, n, nbox, reinterpret_cast<const uint8_t*>(rays), count, offsets, hits, capacity, threads);
}

uint64_t hc_spherecast_all(const Rec* rec, uint32_t n, uint32_t nbox, const nh_SphereCast* casts, uint32_t count, uint32_t* offsets, nh_RayHit* hits,
                           uint32_t capacity, uint32_t threads) {
	return castall<true>(rec, n, nbox, reinterpret_cast<const uint8_t*>(casts), count, offsets, hits, capacity, threads);
}

}
