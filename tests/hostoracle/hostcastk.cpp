// hostcastk.cpp -- the pruning premise of the first-k casts (nh_raycast_k / nh_spherecast_k / nh_boxcast_k / nh_capsulecast_k of include/nudge_hip.h;
// DESIGN 10.13), checked at the leaf on the host (tests/hostcastk_util.py).  The k walk skips a node whose entry t0 exceeds its bound, and the bound is
// never below the t of a collider of the answer; so no collider may be listed at a t below the entry of its OWN leaf box, as the walk's node test
// computes that entry (every ancestor's box contains the leaf box, and the node tests are monotone in the box).
//   hk_premise   for every (cast, collider) pair of an all-hits list (the brute force's offsets and records): the leaf box rebuilt as the build stores
//               it (nh_q_leaf_box), its entry under the k walk's node test -- a ray-like shape: nh_q_cast_node under grow + nh_q_all_pad (+ `extra`
//               times nh_q_all_pad: a wider pad to try); a shape with a size: nh_q_leaf_entry / nh_q_leaf_entry3 -- and the number of pairs whose box
//               is not entered or whose entry is greater than the listed t.  Nothing here keeps a list or walks a tree.
#include "oracle.h"

namespace {

// the words every cast starts with, and what the node test needs of each shape: the grow (one number or three) and whether the shape is ray-like
struct Head {
	nh_f3 o, inv;
	void head(const float origin[3], const float direction[3]) {
		o = v3(origin);
		inv = nh_make3(1.0f / direction[0], 1.0f / direction[1], 1.0f / direction[2]);
	}
};

struct Ray : Head {
	typedef nh_Ray Record;
	float w;
	explicit Ray(const nh_Ray& r) { head(r.origin, r.direction); w = nh_q_cast_pad(o, 0.0f); }
	bool raylike() const { return true; }
	float grow() const { return w; }
	bool entry(nh_f3 p, nh_quat q, nh_f3 h, bool box, float& t0) const { return nh_q_leaf_entry(o, inv, w, p, q, h, box, t0); }
};

struct Ball : Head {
	typedef nh_SphereCast Record;
	float r, w;
	explicit Ball(const nh_SphereCast& c) { head(c.origin, c.direction); r = c.radius; w = r + nh_q_cast_pad(o, r); }
	bool raylike() const { return !(r > 0.0f); }
	float grow() const { return w; }
	bool entry(nh_f3 p, nh_quat q, nh_f3 h, bool box, float& t0) const { return nh_q_leaf_entry(o, inv, w, p, q, h, box, t0); }
};

struct Sized : Head {
	nh_f3 w;
	bool ray;
	void extent(nh_f3 e) {
		const float s = nh_q_cast_pad(o, fmaxf(fmaxf(e.x, e.y), e.z));
		w = nh_make3(e.x + s, e.y + s, e.z + s);
	}
	bool raylike() const { return ray; }
	float grow() const { return w.x; }
	bool entry(nh_f3 p, nh_quat q, nh_f3 h, bool box, float& t0) const { return nh_q_leaf_entry3(o, inv, w, p, q, h, box, t0); }
};

struct Box : Sized {
	typedef nh_BoxCast Record;
	explicit Box(const nh_BoxCast& b) {
		head(b.origin, b.direction);
		const nh_f3 ha = v3(b.size);
		ray = ha.x == 0.0f && ha.y == 0.0f && ha.z == 0.0f;
		extent(ray ? nh_make3(0.0f, 0.0f, 0.0f) : nh_q_box_extent(q4(b.rotation), ha));
	}
};

struct Capsule : Sized {
	typedef nh_CapsuleCast Record;
	explicit Capsule(const nh_CapsuleCast& c) {
		head(c.origin, c.direction);
		ray = c.radius == 0.0f && c.half_height == 0.0f;
		extent(nh_q_capsule_extent(nh_q_capsule_axis(q4(c.rotation), c.half_height), c.radius));
	}
};

template <class Shape>
uint64_t premise(const Rec* rec, uint32_t n, uint32_t nbox, const typename Shape::Record* casts, uint32_t count, const uint32_t* offsets, const nh_RayHit* hits,
                 float extra, uint32_t threads) {
	std::vector<uint64_t> bad(count, 0);
	parallel(count, threads, [&](uint32_t i) {
		const Shape k(casts[i]);
		for (uint32_t j = offsets[i]; j < offsets[i + 1]; ++j) {
			const nh_RayHit& hit = hits[j];
			const uint32_t c = hit.shape == NH_SHAPE_BOX ? hit.collider : hit.collider + nbox;
			if (c >= n) { ++bad[i]; continue; }
			const bool box = c < nbox;
			const nh_f3 p = rec_pos(rec[c]), h = rec_half(rec[c]);
			const nh_quat q = rec_rot(rec[c]);
			float t0 = 0.0f;
			bool in;
			if (k.raylike()) {
				nh_f3 lo, hi;
				nh_q_leaf_box(p, q, h, box, lo, hi);
				const float pad = nh_q_all_pad(lo, hi, k.o);
				in = nh_q_cast_node(lo, hi, k.o, k.inv, k.grow() + pad + extra * pad, t0);
			} else {
				in = k.entry(p, q, h, box, t0);
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
	switch (shape) {
	case 0: return premise<Ray>(rec, n, nbox, static_cast<const nh_Ray*>(casts), count, offsets, hits, extra, threads);
	case 1: return premise<Ball>(rec, n, nbox, static_cast<const nh_SphereCast*>(casts), count, offsets, hits, extra, threads);
	case 2: return premise<Box>(rec, n, nbox, static_cast<const nh_BoxCast*>(casts), count, offsets, hits, extra, threads);
	case 3: return premise<Capsule>(rec, n, nbox, static_cast<const nh_CapsuleCast*>(casts), count, offsets, hits, extra, threads);
	}
	return ~0ull;
}

}
