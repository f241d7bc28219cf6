// oracle.h -- what the host oracles of the scene queries (tests/hostoracle/host*.cpp, one library: tests/hostlib.py) have in common: the collider
// record, the thread loop, the rules every answer record encodes, the swept shapes of the casts and the one brute-force closest-hit cast over them.  Built with g++
// -ffp-contract=off, so that nudge_amd/csrc/nh_query.h's arithmetic returns the device's bits.  Shared between oracles only: nothing here walks a tree or
// keeps a list, which is what the oracles judge.
#pragma once
#include <stdint.h>
#include <math.h>
#include <thread>
#include <vector>
#include "../../include/nudge_hip.h"
#include "../../nudge_amd/csrc/nh_query.h"

// 12 words per collider (tests/hostlib.py REC, nh_query_tree.h's nh_QRec): position, bits(body), rotation, half extents | radius (x3), bits(tag)
struct Rec { float p[3]; uint32_t body; float q[4]; float h[3]; uint32_t tag; };
static_assert(sizeof(Rec) == 48, "Rec is hostlib.REC: 12 words");

static inline bool finite(float x) { return (nh_asuint(x) & 0x7f800000u) != 0x7f800000u; }

// f(i) for every i < count, on `threads` threads
template <class F> static void parallel(uint32_t count, uint32_t threads, F f) {
	if (threads < 1) threads = 1;
	std::vector<std::thread> pool;
	for (uint32_t k = 0; k < threads; ++k) pool.emplace_back([=]() { for (uint32_t i = k; i < count; i += threads) f(i); });
	for (auto& t : pool) t.join();
}

static inline nh_f3 v3(const float a[3]) { return nh_make3(a[0], a[1], a[2]); }
static inline nh_quat q4(const float a[4]) { return nh_quat{ a[0], a[1], a[2], a[3] }; }
static inline nh_f3 rec_pos(const Rec& r) { return v3(r.p); }
static inline nh_quat rec_rot(const Rec& r) { return q4(r.q); }
static inline nh_f3 rec_half(const Rec& r) { return v3(r.h); }

// nh_overlap's validity and predicates, capsules included (the header's "Query shapes"); `capsules` false: a capsule query is invalid, as it was
// before nh_overlap knew the shape (tests/test_cpu_overlap.py's invalid queries rely on it)
static inline bool valid(const nh_OverlapQuery& q, bool capsules = true) {
	if (q.shape != NH_SHAPE_SPHERE && q.shape != NH_SHAPE_BOX && !(capsules && q.shape == NH_SHAPE_CAPSULE)) return false;
	if (!finite(q.center[0]) || !finite(q.center[1]) || !finite(q.center[2]) || !finite(q.size[0]) || q.size[0] < 0.0f) return false;
	if (q.shape == NH_SHAPE_SPHERE || (q.shape == NH_SHAPE_CAPSULE && q.size[1] == 0.0f)) return true;
	const int ns = q.shape == NH_SHAPE_BOX ? 3 : 2;
	for (int k = 1; k < ns; ++k) if (!finite(q.size[k]) || q.size[k] < 0.0f) return false;
	for (int k = 0; k < 4; ++k) if (!finite(q.rotation[k])) return false;
	return true;
}

static inline bool touches(const nh_OverlapQuery& q, const Rec& r, bool box) {
	const nh_f3 c = v3(q.center), h = v3(q.size);
	const nh_quat qr = q4(q.rotation);
	const nh_f3 p = rec_pos(r), rh = rec_half(r);
	const nh_quat rq = rec_rot(r);
	if (q.shape == NH_SHAPE_CAPSULE)
		return box ? nh_q_overlap_capsule_box(c, qr, h.x, h.y, p, rq, rh) : nh_q_overlap_capsule_sphere(c, qr, h.x, h.y, p, rh.x);
	const bool sphere = q.shape == NH_SHAPE_SPHERE;
	if (box) return sphere ? nh_q_overlap_sphere_box(c, h.x, p, rq, rh) : nh_q_overlap_box_box(c, qr, h, p, rq, rh);
	return sphere ? nh_q_overlap_sphere_sphere(c, h.x, p, rh.x) : nh_q_overlap_sphere_box(p, rh.x, c, qr, h);
}

// nh_overlap's and nh_penetration's batch by brute force: every valid query (`capsules`: as for valid()) against every collider but those of its
// ignore_body, in index order.
// offsets: count + 1 words, always written (with the 32-bit wrap the device's scan has; offsets[count] = 0xffffffff on overflow).  hits: write(record, query,
// combined index) for every query whose segment ends at or below `capacity` (nothing on overflow); no other byte of `hits` is touched.  Returns the true
// total (64 bits).
template <class H, class W>
static uint64_t overlap_all(const Rec* rec, uint32_t n, uint32_t nbox, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets, H* hits,
                            uint32_t capacity, uint32_t threads, bool capsules, W write) {
	std::vector<uint32_t> cnt(count);
	parallel(count, threads, [&](uint32_t i) {
		uint32_t k = 0;
		if (valid(queries[i], capsules))
			for (uint32_t c = 0; c < n; ++c) if (rec[c].body != queries[i].ignore_body && touches(queries[i], rec[c], c < nbox)) ++k;
		cnt[i] = k;
	});
	uint64_t total = 0;
	uint32_t run = 0;
	for (uint32_t i = 0; i < count; ++i) { offsets[i] = run; run += cnt[i]; total += cnt[i]; }
	offsets[count] = run;
	if (total >= 0xffffffffull) { offsets[count] = 0xffffffffu; return total; }
	if (!hits || !capacity) return total;
	parallel(count, threads, [&](uint32_t i) {
		if (offsets[i + 1] > capacity || !cnt[i]) return;
		uint32_t k = offsets[i];
		for (uint32_t c = 0; c < n; ++c)
			if (rec[c].body != queries[i].ignore_body && touches(queries[i], rec[c], c < nbox)) write(hits[k++], queries[i], c);
	});
	return total;
}

// who was hit: the body, the combined index c split into collider / shape, the tag.  A miss is all ones and NH_SHAPE_NONE
template <class H> static void write_who(H& out, const Rec* rec, uint32_t nbox, uint32_t c) {
	out.body = rec[c].body; out.collider = c < nbox ? c : c - nbox; out.shape = c < nbox ? NH_SHAPE_BOX : NH_SHAPE_SPHERE; out.tag = rec[c].tag;
}
template <class H> static void write_nobody(H& out) { out.body = out.collider = out.tag = 0xffffffffu; out.shape = NH_SHAPE_NONE; }

// nh_RayHit: a hit of collider c (combined index) at t with normal n; a miss holds the cast's own limit, or NaN where the cast was invalid
static inline void write_ray_hit(nh_RayHit& out, const Rec* rec, uint32_t nbox, uint32_t c, float t, nh_f3 n) {
	out.t = t; out.normal[0] = n.x; out.normal[1] = n.y; out.normal[2] = n.z;
	write_who(out, rec, nbox, c);
}
static inline void write_ray_miss(nh_RayHit& out, bool ok, float max_t) {
	out.t = ok ? max_t : nh_asfloat(0x7fc00000u); out.normal[0] = out.normal[1] = out.normal[2] = 0.0f;
	write_nobody(out);
}

// a closest-hit cast's record from what closest_hit (below) left
static inline void write_cast(nh_RayHit& out, const Rec* rec, uint32_t nbox, bool ok, float max_t, float bt, uint32_t bc, nh_f3 bn) {
	if (bc == 0xffffffffu) write_ray_miss(out, ok, max_t);
	else write_ray_hit(out, rec, nbox, bc, bt, bn);
}

// The swept shapes of the casts and the movers (hostcast.cpp, hostcastk.cpp, hostmover.cpp), each rule written once.  Each gives the validity of its own
// fields, the half extent of its bounds for the cast's pad, whether the reach rule applies to it, its closest-hit sweep from o along d against one collider,
// and its all-hits decision on one collider (nh_query.h's nh_q_all_hit*: t0 = the entry into the collider's leaf box, read only under the reach rule).
// SweptRay: nothing but the ray's own predicates
struct SweptRay {
	bool valid() const { return true; }
	nh_f3 extent() const { return nh_make3(0.0f, 0.0f, 0.0f); }
	bool reach() const { return false; }
	nh_QHit sweep(nh_f3 o, nh_f3 d, bool box, nh_f3 p, nh_quat qb, nh_f3 hb) const { return box ? nh_q_ray_box(o, d, p, qb, hb) : nh_q_ray_sphere(o, d, p, hb.x); }
	nh_QHit all_hit(nh_f3 o, nh_f3 d, float max_t, float t0, nh_f3 p, nh_quat qb, nh_f3 hb, bool box) const { return nh_q_all_hit<false>(o, d, 0.0f, max_t, t0, p, qb, hb, box); }
};
// SweptSphere: radius r.  r = 0 is a ray
struct SweptSphere {
	float r;
	bool valid() const { return finite(r) && !(r < 0.0f); }
	nh_f3 extent() const { return nh_make3(r, r, r); }
	bool reach() const { return r > 0.0f; }
	nh_QHit sweep(nh_f3 o, nh_f3 d, bool box, nh_f3 p, nh_quat qb, nh_f3 hb) const { return box ? nh_q_sweep_box(o, d, r, p, qb, hb) : nh_q_sweep_sphere(o, d, r, p, hb.x); }
	nh_QHit all_hit(nh_f3 o, nh_f3 d, float max_t, float t0, nh_f3 p, nh_quat qb, nh_f3 hb, bool box) const { return nh_q_all_hit<true>(o, d, r, max_t, t0, p, qb, hb, box); }
};
// SweptCapsule: rotation q, radius r, half height hh.  hh = 0 is a ball, which does not read its rotation to be valid; r = hh = 0 is a ray
struct SweptCapsule {
	nh_quat q; float r, hh;
	bool valid() const { return finite(r) && finite(hh) && !(r < 0.0f) && !(hh < 0.0f) && (hh == 0.0f || (finite(q.x) && finite(q.y) && finite(q.z) && finite(q.s))); }
	nh_f3 extent() const { return nh_q_capsule_extent(nh_q_capsule_axis(q, hh), r); }
	bool reach() const { return r > 0.0f || hh > 0.0f; }
	nh_QHit sweep(nh_f3 o, nh_f3 d, bool box, nh_f3 p, nh_quat qb, nh_f3 hb) const {
		return box ? nh_q_sweep_capsule_box(o, d, q, r, hh, p, qb, hb) : nh_q_sweep_capsule_sphere(o, d, q, r, hh, p, hb.x);
	}
	nh_QHit all_hit(nh_f3 o, nh_f3 d, float max_t, float t0, nh_f3 p, nh_quat qb, nh_f3 hb, bool box) const { return nh_q_all_hit_capsule(o, d, q, r, hh, max_t, t0, p, qb, hb, box); }
};
// SweptBox: rotation q, half extents h.  h = (0, 0, 0) is a ray, which does not read its rotation at all
struct SweptBox {
	nh_quat q; nh_f3 h;
	bool ray() const { return h.x == 0.0f && h.y == 0.0f && h.z == 0.0f; }
	bool valid() const {
		return finite(h.x) && finite(h.y) && finite(h.z) && !(h.x < 0.0f) && !(h.y < 0.0f) && !(h.z < 0.0f) && (ray() || (finite(q.x) && finite(q.y) && finite(q.z) && finite(q.s)));
	}
	nh_f3 extent() const { return ray() ? nh_make3(0.0f, 0.0f, 0.0f) : nh_q_box_extent(q, h); }
	bool reach() const { return !ray(); }
	nh_QHit sweep(nh_f3 o, nh_f3 d, bool box, nh_f3 p, nh_quat qb, nh_f3 hb) const {
		return box ? nh_q_sweep_box_box(o, d, q, h, p, qb, hb) : nh_q_sweep_box_sphere(o, d, q, h, p, hb.x);
	}
	nh_QHit all_hit(nh_f3 o, nh_f3 d, float max_t, float t0, nh_f3 p, nh_quat qb, nh_f3 hb, bool box) const { return nh_q_all_hit_box(o, d, q, h, max_t, t0, p, qb, hb, box); }
};

// the swept shape of a cast record; all four records start with nh_Ray's fields (origin, max_t, direction, ignore_body)
static inline SweptRay swept(const nh_Ray&) { return SweptRay{}; }
static inline SweptSphere swept(const nh_SphereCast& c) { return SweptSphere{ c.radius }; }
static inline SweptBox swept(const nh_BoxCast& c) { return SweptBox{ q4(c.rotation), v3(c.size) }; }
static inline SweptCapsule swept(const nh_CapsuleCast& c) { return SweptCapsule{ q4(c.rotation), c.radius, c.half_height }; }

// f(the records, typed) for the shape number of the entry points that take one: 0 nh_Ray, 1 nh_SphereCast, 2 nh_BoxCast, 3 nh_CapsuleCast; all ones for any other
template <class F> static uint64_t by_shape(uint32_t shape, const void* casts, F f) {
	switch (shape) {
	case 0: return f(static_cast<const nh_Ray*>(casts));
	case 1: return f(static_cast<const nh_SphereCast*>(casts));
	case 2: return f(static_cast<const nh_BoxCast*>(casts));
	case 3: return f(static_cast<const nh_CapsuleCast*>(casts));
	}
	return ~0ull;
}

static inline bool finite3(nh_f3 a) { return finite(a.x) && finite(a.y) && finite(a.z); }

// the per-axis grow of the node boxes for the shape `a` cast from o: its extent and the cast's pad (nh_q_cast_node3's w; the same on every axis it is
// nh_q_cast_node's, to the bit)
template <class S> static nh_f3 cast_grow(const S& a, nh_f3 o) {
	const nh_f3 e = a.extent();
	const float s = nh_q_cast_pad(o, fmaxf(fmaxf(e.x, e.y), e.z));
	return nh_make3(e.x + s, e.y + s, e.z + s);
}

// The closest hit of the shape `a` cast from o along d up to max_t, by brute force over all colliders with the header's exact rules: invalid casts (which
// look at no collider), ignore_body, ties, the reach rule.  words, mask: colliders whose layer word shares no bit with the mask do not exist for this cast
// (words = NULL: all are seen); only >= 0: that one collider (combined index) alone.  Leaves (bt, bc, bn) as nh_q_cast_one leaves them and returns whether
// the cast was valid.
template <class S>
static bool closest_hit(const Rec* rec, uint32_t n, uint32_t nbox, const S& a, nh_f3 o, nh_f3 d, float max_t, uint32_t ignore_body, const uint32_t* words,
                        uint32_t mask, int64_t only, float& bt, uint32_t& bc, nh_f3& bn) {
	const bool ok = finite3(o) && finite3(d) && a.valid();
	const nh_f3 inv = nh_make3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z), w = cast_grow(a, o);
	const bool reach = a.reach();
	bt = max_t; bc = 0xffffffffu; bn = nh_make3(0.0f, 0.0f, 0.0f);
	const uint32_t c0 = only >= 0 ? (uint32_t)only : 0u, c1 = only >= 0 ? (uint32_t)only + 1u : n;
	for (uint32_t c = ok ? c0 : c1; c < c1; ++c) {
		const Rec& rc = rec[c];
		if (rc.body == ignore_body) continue;
		if (words && !(words[c] & mask)) continue;
		const bool box = c < nbox;
		const nh_f3 p = rec_pos(rc), h = rec_half(rc);
		const nh_quat q = rec_rot(rc);
		nh_QHit hit = a.sweep(o, d, box, p, q, h);
		if (!hit.hit) continue;
		if (reach) {
			// the reach rule: the leaf box must be entered, and the hit is no earlier than that entry
			nh_f3 lo, hi;
			nh_q_leaf_box(p, q, h, box, lo, hi);
			float t0;
			if (!nh_q_cast_node3(lo, hi, o, inv, w, t0)) continue;
			if (t0 > hit.t) hit.t = t0;
		}
		if (nh_q_better(hit.t, c, max_t, bt, bc)) { bt = hit.t; bc = c; bn = hit.n; }
	}
	return ok;
}

// nh_PointHit, likewise: the distance, the normal and the point of h
static inline void write_point_hit(nh_PointHit& out, const Rec* rec, uint32_t nbox, uint32_t c, float distance, const nh_QPoint& h) {
	out.reserved = 0u;
	out.distance = distance;
	out.normal[0] = h.n.x; out.normal[1] = h.n.y; out.normal[2] = h.n.z;
	out.point[0] = h.x.x; out.point[1] = h.x.y; out.point[2] = h.x.z;
	write_who(out, rec, nbox, c);
}
static inline void write_point_miss(nh_PointHit& out, bool ok, float max_d) {
	out.reserved = 0u;
	out.distance = ok ? max_d : nh_asfloat(0x7fc00000u);
	out.normal[0] = out.normal[1] = out.normal[2] = 0.0f; out.point[0] = out.point[1] = out.point[2] = 0.0f;
	write_nobody(out);
}

// one collider against the point p, as nh_closest defines it: the predicate's answer, and as `key` its distance under the reach rule -- at least that
// of the leaf box (rebuilt as the build stores it), where p lies outside it
static inline nh_QPoint rec_point(const Rec& r, bool box, nh_f3 p, float& key) {
	const nh_QPoint h = box ? nh_q_point_box(p, rec_pos(r), rec_rot(r), rec_half(r)) : nh_q_point_sphere(p, rec_pos(r), r.h[0]);
	nh_f3 lo, hi;
	nh_q_leaf_box(rec_pos(r), rec_rot(r), rec_half(r), box, lo, hi);
	key = nh_q_point_key(h.d, nh_q_point_node(lo, hi, p));
	return h;
}

// the single-shape entry points' outputs: (t, normal, hit as 1.0 / 0.0), (normal, depth), (distance, normal, point)
static inline void out5(const nh_QHit& s, float out[5]) { out[0] = s.t; out[1] = s.n.x; out[2] = s.n.y; out[3] = s.n.z; out[4] = s.hit ? 1.0f : 0.0f; }
static inline void out4(const nh_QPen& o, float out[4]) { out[0] = o.n.x; out[1] = o.n.y; out[2] = o.n.z; out[3] = o.depth; }
static inline void out7(const nh_QPoint& r, float out[7]) { out[0] = r.d; out[1] = r.n.x; out[2] = r.n.y; out[3] = r.n.z; out[4] = r.x.x; out[5] = r.x.y; out[6] = r.x.z; }
