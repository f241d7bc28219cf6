// hostcastk.cpp -- the pruning premise of the first-k casts (nh_raycast_k / nh_spherecast_k / nh_boxcast_k / nh_capsulecast_k of include/nudge_hip.h;
// DESIGN 10.13), checked at the leaf on the host (tests/hostcastk_util.py).  The k walk skips a node whose entry t0 exceeds its bound, and the bound is
// never below the t of a collider of the answer; so no collider may be listed at a t below the entry of its OWN leaf box, as the walk's node test
// computes that entry (every ancestor's box contains the leaf box, and the node tests are monotone in the box).
//   hk_premise   for every (cast, collider) pair of an all-hits list (the brute force's offsets and records): the leaf box rebuilt as the build stores
//               it (nh_q_leaf_box), its entry under the k walk's node test -- a ray-like shape: nh_q_cast_node under grow + nh_q_all_pad (+ `extra`
//               times nh_q_all_pad: a wider pad to try); a shape with a size: nh_q_leaf_entry3 -- and the number of pairs whose box
//               is not entered or whose entry is greater than the listed t.  Nothing here keeps a list or walks a tree.
#include "oracle.h"

namespace {

template <class R>
uint64_t premise(const Rec* rec, uint32_t n, uint32_t nbox, const R* casts, uint32_t count, const uint32_t* offsets, const nh_RayHit* hits,
                 float extra, uint32_t threads) {
	std::vector<uint64_t> bad(count, 0);
	parallel(count, threads, [&](uint32_t i) {
		// what the node test needs of the cast: its grow per axis, and whether the shape is ray-like (no reach rule: one grow, the all-hits pad on top)
		const auto a = swept(casts[i]);
		const nh_f3 o = v3(casts[i].origin), inv = nh_make3(1.0f / casts[i].direction[0], 1.0f / casts[i].direction[1], 1.0f / casts[i].direction[2]), w = cast_grow(a, o);
		for (uint32_t j = offsets[i]; j < offsets[i + 1]; ++j) {
			const nh_RayHit& hit = hits[j];
			const uint32_t c = hit.shape == NH_SHAPE_BOX ? hit.collider : hit.collider + nbox;
			if (c >= n) { ++bad[i]; continue; }
			const bool box = c < nbox;
			const nh_f3 p = rec_pos(rec[c]), h = rec_half(rec[c]);
			const nh_quat q = rec_rot(rec[c]);
			float t0 = 0.0f;
			bool in;
			if (!a.reach()) {
				nh_f3 lo, hi;
				nh_q_leaf_box(p, q, h, box, lo, hi);
				const float pad = nh_q_all_pad(lo, hi, o);
				in = nh_q_cast_node(lo, hi, o, inv, w.x + pad + extra * pad, t0);
			} else {
				in = nh_q_leaf_entry3(o, inv, w, p, q, h, box, t0);
			}
			if (!in || !(t0 <= hit.t)) ++bad[i];
		}
	});
	uint64_t total = 0;
	for (uint64_t b : bad) total += b;
	return total;
}

}

extern "C" {

// shape: 0 nh_Ray, 1 nh_SphereCast, 2 nh_BoxCast, 3 nh_CapsuleCast records in `casts`; offsets (count + 1) and hits: an all-hits list of those casts
// over `rec`.  extra: 0 for the k walk's own pad.  Returns the number of listed pairs that break the premise.
uint64_t hk_premise(const Rec* rec, uint32_t n, uint32_t nbox, uint32_t shape, const void* casts, uint32_t count, const uint32_t* offsets, const nh_RayHit* hits,
                    float extra, uint32_t threads) {
	return by_shape(shape, casts, [=](auto* typed) { return premise(rec, n, nbox, typed, count, offsets, hits, extra, threads); });
}

}
