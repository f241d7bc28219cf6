// hostcast.cpp -- CPU build of the casts of include/nudge_hip.h for all four shapes (ray, sphere, box, capsule: oracle.h's swept shapes), the oracle of the
// GPU's walks (tests/hostcast_util.py).  Two loops, written apart because the tests check one against the other: they share the shape's description and
// neither the per-collider decision nor the list handling.
//   hc_cast      closest hit (or the hit of one collider): oracle.h's closest_hit over the shapes' sweeps, with the header's exact rules -- invalid casts,
//                ignore_body, ties, the reach rule for a shape with a size (the leaf box rebuilt as the build stores it)
//   hc_cast_all  all hits: per cast, a brute force over all colliders in index order over the shapes' nh_q_all_hit* -- invalid casts, ignore_body, the reach
//                rule on the leaf box grown per axis by the cast's own extent, 0 <= t <= max_t -- then std::stable_sort by t over the index-ordered hits,
//                the offsets by an exclusive scan, the capacity prefix of whole segments and the overflow marker
// Both run on several threads.
#include <algorithm>
#include "oracle.h"

namespace {

struct Found { float t; nh_f3 n; uint32_t c; };

// the hits of one cast, ordered; `out` == nullptr: the count alone
template <class R>
uint32_t list_one(const Rec* rec, uint32_t n, uint32_t nbox, const R& cast, std::vector<Found>* out) {
	const auto a = swept(cast);
	const nh_f3 o = v3(cast.origin), d = v3(cast.direction);
	if (!(finite3(o) && finite3(d) && a.valid())) return 0u;
	const nh_f3 inv = nh_make3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z), w = cast_grow(a, o);
	const bool reach = a.reach();
	uint32_t m = 0u;
	for (uint32_t c = 0u; c < n; ++c) {
		const Rec& e = rec[c];
		if (e.body == cast.ignore_body) continue;
		const bool box = c < nbox;
		const nh_f3 p = rec_pos(e), h = rec_half(e);
		const nh_quat q = rec_rot(e);
		float t0 = 0.0f;
		// the reach rule: the collider's own leaf box must be entered, and the hit is no earlier than that entry
		if (reach && !nh_q_leaf_entry3(o, inv, w, p, q, h, box, t0)) continue;
		const nh_QHit s = a.all_hit(o, d, cast.max_t, t0, p, q, h, box);
		if (!s.hit) continue;
		if (out) out->push_back(Found{ s.t, s.n, c });
		++m;
	}
	// (float comparison: -0 equals +0; stable: equal t stay in index order)
	if (out) std::stable_sort(out->begin(), out->end(), [](const Found& a, const Found& b) { return a.t < b.t; });
	return m;
}

template <class R>
uint64_t castall(const Rec* rec, uint32_t n, uint32_t nbox, const R* casts, uint32_t count, uint32_t* offsets, nh_RayHit* hits, uint32_t capacity, uint32_t threads) {
	std::vector<uint32_t> counts(count);
	parallel(count, threads, [&](uint32_t i) { counts[i] = list_one(rec, n, nbox, casts[i], nullptr); });
	uint64_t total = 0;
	for (uint32_t i = 0; i < count; ++i) { offsets[i] = (uint32_t)total; total += counts[i]; }
	offsets[count] = (uint32_t)total;
	if (total >= 0xffffffffull) { offsets[count] = 0xffffffffu; return total; }      // the marker: no record at all
	if (!hits || !capacity) return total;
	parallel(count, threads, [&](uint32_t i) {
		if (!(offsets[i + 1] <= capacity) || !counts[i]) return;      // whole segments that fit
		std::vector<Found> found;
		list_one(rec, n, nbox, casts[i], &found);
		for (uint32_t j = 0; j < found.size(); ++j) write_ray_hit(hits[offsets[i] + j], rec, nbox, found[j].c, found[j].t, found[j].n);
	});
	return total;
}

}

extern "C" {

// shape: 0 nh_Ray, 1 nh_SphereCast, 2 nh_BoxCast, 3 nh_CapsuleCast records in `casts`.  only >= 0: the answer of that one collider (combined index)
// alone, as the closest-hit rule would give it
void hc_cast(uint32_t shape, const Rec* rec, uint32_t n, uint32_t nbox, const void* casts, uint32_t count, nh_RayHit* hits, int64_t only, uint32_t threads) {
	by_shape(shape, casts, [=](auto* typed) {
		parallel(count, threads, [=](uint32_t i) {
			const auto& cc = typed[i];
			float bt; uint32_t bc; nh_f3 bn;
			const bool ok = closest_hit(rec, n, nbox, swept(cc), v3(cc.origin), v3(cc.direction), cc.max_t, cc.ignore_body, nullptr, 0u, only, bt, bc, bn);
			write_cast(hits[i], rec, nbox, ok, cc.max_t, bt, bc, bn);
		});
		return 0ull;
	});
}

// offsets: count + 1 words, always written; hits: `capacity` records or null (count only), written for the segments that fit and left alone
// elsewhere.  Returns the true total.
uint64_t hc_cast_all(uint32_t shape, const Rec* rec, uint32_t n, uint32_t nbox, const void* casts, uint32_t count, uint32_t* offsets, nh_RayHit* hits,
                     uint32_t capacity, uint32_t threads) {
	return by_shape(shape, casts, [=](auto* typed) { return castall(rec, n, nbox, typed, count, offsets, hits, capacity, threads); });
}

}
