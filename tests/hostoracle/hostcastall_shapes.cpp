// hostcastall_shapes.cpp -- CPU build of the all-hits box and capsule casts (nh_boxcast_all / nh_capsulecast_all of include/nudge_hip.h), the oracle of the
// GPU's chain (tests/hostcastall_shapes_util.py).
//   hs_boxcast_all / hs_capsulecast_all   per cast, a brute force over all colliders in index order with the header's exact rules -- invalid casts,
//               ignore_body, the reach rule for a shape with a size on the leaf box rebuilt as the build stores it, grown per axis by the cast's own
//               extent, 0 <= t <= max_t -- then std::stable_sort by t over the index-ordered hits, the offsets by an exclusive scan, the capacity
//               prefix of whole segments and the overflow marker; on several threads
#include <algorithm>
#include "oracle.h"

namespace {

struct Found { float t; nh_f3 n; uint32_t c; };

// what the two shapes share: the head of the record, the per-axis grow of the leaf boxes, and whether the reach rule applies
struct Head {
	nh_f3 o, d, inv, w;
	float max_t;
	uint32_t ignore;
	bool ok, reach;
	void head(const float origin[3], float mt, const float direction[3], uint32_t ignore_body) {
		o = v3(origin); d = v3(direction); max_t = mt; ignore = ignore_body;
		ok = finite(o.x) && finite(o.y) && finite(o.z) && finite(d.x) && finite(d.y) && finite(d.z);
		inv = nh_make3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
	}
	void grow(nh_f3 e) {
		const float s = nh_q_cast_pad(o, fmaxf(fmaxf(e.x, e.y), e.z));
		w = nh_make3(e.x + s, e.y + s, e.z + s);
	}
};

struct Box : Head {
	typedef nh_BoxCast Record;
	nh_quat qa;
	nh_f3 ha;
	explicit Box(const nh_BoxCast& b) {
		head(b.origin, b.max_t, b.direction, b.ignore_body);
		qa = q4(b.rotation); ha = v3(b.size);
		const bool ray = ha.x == 0.0f && ha.y == 0.0f && ha.z == 0.0f;
		ok = ok && finite(ha.x) && finite(ha.y) && finite(ha.z) && !(ha.x < 0.0f) && !(ha.y < 0.0f) && !(ha.z < 0.0f) &&
		     (ray || (finite(qa.x) && finite(qa.y) && finite(qa.z) && finite(qa.s)));
		reach = !ray;
		grow(ray ? nh_make3(0.0f, 0.0f, 0.0f) : nh_q_box_extent(qa, ha));
	}
	nh_QHit hit(float t0, nh_f3 p, nh_quat q, nh_f3 h, bool box) const { return nh_q_all_hit_box(o, d, qa, ha, max_t, t0, p, q, h, box); }
};

struct Capsule : Head {
	typedef nh_CapsuleCast Record;
	nh_quat qa;
	float r, hh;
	explicit Capsule(const nh_CapsuleCast& c) {
		head(c.origin, c.max_t, c.direction, c.ignore_body);
		qa = q4(c.rotation); r = c.radius; hh = c.half_height;
		ok = ok && finite(r) && finite(hh) && !(r < 0.0f) && !(hh < 0.0f) && (hh == 0.0f || (finite(qa.x) && finite(qa.y) && finite(qa.z) && finite(qa.s)));
		reach = r > 0.0f || hh > 0.0f;
		grow(nh_q_capsule_extent(nh_q_capsule_axis(qa, hh), r));
	}
	nh_QHit hit(float t0, nh_f3 p, nh_quat q, nh_f3 h, bool box) const { return nh_q_all_hit_capsule(o, d, qa, r, hh, max_t, t0, p, q, h, box); }
};

// the hits of one cast, ordered; `out` == nullptr: the count alone
template <class Shape>
uint32_t cast_one(const Rec* rec, uint32_t n, uint32_t nbox, const typename Shape::Record& cast, std::vector<Found>* out) {
	const Shape k(cast);
	if (!k.ok) return 0u;
	uint32_t m = 0u;
	for (uint32_t c = 0u; c < n; ++c) {
		const Rec& e = rec[c];
		if (e.body == k.ignore) continue;
		const bool box = c < nbox;
		const nh_f3 p = rec_pos(e), h = rec_half(e);
		const nh_quat q = rec_rot(e);
		float t0 = 0.0f;
		// the reach rule: the collider's own leaf box must be entered, and the hit is no earlier than that entry
		if (k.reach && !nh_q_leaf_entry3(k.o, k.inv, k.w, p, q, h, box, t0)) continue;
		const nh_QHit s = k.hit(t0, p, q, h, box);
		if (!s.hit) continue;
		if (out) out->push_back(Found{ s.t, s.n, c });
		++m;
	}
	// (float comparison: -0 equals +0; stable: equal t stay in index order)
	if (out) std::stable_sort(out->begin(), out->end(), [](const Found& a, const Found& b) { return a.t < b.t; });
	return m;
}

template <class Shape>
uint64_t castall(const Rec* rec, uint32_t n, uint32_t nbox, const typename Shape::Record* casts, uint32_t count, uint32_t* offsets, nh_RayHit* hits,
                 uint32_t capacity, uint32_t threads) {
	std::vector<uint32_t> counts(count);
	parallel(count, threads, [&](uint32_t i) { counts[i] = cast_one<Shape>(rec, n, nbox, casts[i], nullptr); });
	uint64_t total = 0;
	for (uint32_t i = 0; i < count; ++i) { offsets[i] = (uint32_t)total; total += counts[i]; }
	offsets[count] = (uint32_t)total;
	if (total >= 0xffffffffull) { offsets[count] = 0xffffffffu; return total; }      // the marker: no record at all
	if (!hits || !capacity) return total;
	parallel(count, threads, [&](uint32_t i) {
		if (!(offsets[i + 1] <= capacity) || !counts[i]) return;      // whole segments that fit
		std::vector<Found> found;
		cast_one<Shape>(rec, n, nbox, casts[i], &found);
		for (uint32_t j = 0; j < found.size(); ++j) write_ray_hit(hits[offsets[i] + j], rec, nbox, found[j].c, found[j].t, found[j].n);
	});
	return total;
}

}

extern "C" {

// offsets: count + 1 words, always written; hits: `capacity` records or null (count only), written for the segments that fit and left alone
// elsewhere.  Returns the true total.
uint64_t hs_boxcast_all(const Rec* rec, uint32_t n, uint32_t nbox, const nh_BoxCast* casts, uint32_t count, uint32_t* offsets, nh_RayHit* hits, uint32_t capacity,
                        uint32_t threads) {
	return castall<Box>(rec, n, nbox, casts, count, offsets, hits, capacity, threads);
}

uint64_t hs_capsulecast_all(const Rec* rec, uint32_t n, uint32_t nbox, const nh_CapsuleCast* casts, uint32_t count, uint32_t* offsets, nh_RayHit* hits,
                            uint32_t capacity, uint32_t threads) {
	return castall<Capsule>(rec, n, nbox, casts, count, offsets, hits, capacity, threads);
}

}
