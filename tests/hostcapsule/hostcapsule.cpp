// hostcapsule.cpp -- CPU build of the capsule arithmetic of nudge_amd/csrc/nh_query.h, the oracle of the GPU's nh_capsulecast and of nh_overlap's
// capsule queries.  Built with g++ -ffp-contract=off (tests/hostcapsule_util.py), so that every function returns the device's bits; loaded with ctypes.
//   hc_capsulecast  closest hit (or the hit of one collider) by brute force over all colliders, with the header's exact rules -- invalid casts,
//                   hh = 0 as a sphere cast, ignore_body, ties, the reach rule unless r = hh = 0 (the leaf box rebuilt as the build stores it)
//   hc_overlap      offsets and records of a batch of sphere, box and capsule queries by brute force, with nh_overlap's exact semantics (ignore_body,
//                   invalid queries, capacity prefix, the 2^32 - 1 marker)
//   hc_*            the single-collider predicates alone
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

static void cast_one(const Rec* rec, uint32_t n, uint32_t nbox, const nh_CapsuleCast& cc, nh_RayHit& out, int64_t only) {
	const nh_f3 o = nh_make3(cc.origin[0], cc.origin[1], cc.origin[2]), d = nh_make3(cc.direction[0], cc.direction[1], cc.direction[2]);
	const nh_quat qa = { cc.rotation[0], cc.rotation[1], cc.rotation[2], cc.rotation[3] };
	const float r = cc.radius, hh = cc.half_height;
	const bool ok = finite(o.x) && finite(o.y) && finite(o.z) && finite(d.x) && finite(d.y) && finite(d.z) && finite(r) && finite(hh) && !(r < 0.0f) &&
	                !(hh < 0.0f) && (hh == 0.0f || (finite(qa.x) && finite(qa.y) && finite(qa.z) && finite(qa.s)));
	const nh_f3 inv = nh_make3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
	const nh_f3 e = nh_q_capsule_extent(nh_q_capsule_axis(qa, hh), r);
	const float s = nh_q_cast_pad(o, fmaxf(fmaxf(e.x, e.y), e.z));
	const nh_f3 w = nh_make3(e.x + s, e.y + s, e.z + s);
	const bool reach = r > 0.0f || hh > 0.0f;
	float bt = cc.max_t; uint32_t bc = 0xffffffffu; nh_f3 bn = nh_make3(0.0f, 0.0f, 0.0f);
	const uint32_t c0 = only >= 0 ? (uint32_t)only : 0u, c1 = only >= 0 ? (uint32_t)only + 1u : n;
	for (uint32_t c = ok ? c0 : c1; c < c1; ++c) {
		const Rec& rc = rec[c];
		if (rc.body == cc.ignore_body) continue;
		const bool box = c < nbox;
		const nh_f3 p = nh_make3(rc.p[0], rc.p[1], rc.p[2]), h = nh_make3(rc.h[0], rc.h[1], rc.h[2]);
		const nh_quat q = { rc.q[0], rc.q[1], rc.q[2], rc.q[3] };
		nh_QHit hit = box ? nh_q_sweep_capsule_box(o, d, qa, r, hh, p, q, h) : nh_q_sweep_capsule_sphere(o, d, qa, r, hh, p, h.x);
		if (!hit.hit) continue;
		if (reach) {
			// the reach rule: the leaf box must be entered, and the hit is no earlier than that entry
			nh_f3 lo, hi;
			nh_q_leaf_box(p, q, h, box, lo, hi);
			float t0;
			if (!nh_q_cast_node3(lo, hi, o, inv, w, t0)) continue;
			if (t0 > hit.t) hit.t = t0;
		}
		if (nh_q_better(hit.t, c, cc.max_t, bt, bc)) { bt = hit.t; bc = c; bn = hit.n; }
	}
	if (bc == 0xffffffffu) {
		out.t = ok ? cc.max_t : nh_asfloat(0x7fc00000u); out.normal[0] = out.normal[1] = out.normal[2] = 0.0f;
		out.body = out.collider = out.tag = 0xffffffffu; out.shape = NH_SHAPE_NONE;
	} else {
		out.t = bt; out.normal[0] = bn.x; out.normal[1] = bn.y; out.normal[2] = bn.z;
		out.body = rec[bc].body; out.collider = bc < nbox ? bc : bc - nbox; out.shape = bc < nbox ? NH_SHAPE_BOX : NH_SHAPE_SPHERE; out.tag = rec[bc].tag;
	}
}

// nh_overlap's validity and predicates, capsules included (the header's "Query shapes")
static bool valid(const nh_OverlapQuery& q) {
	if (q.shape != NH_SHAPE_SPHERE && q.shape != NH_SHAPE_BOX && q.shape != NH_SHAPE_CAPSULE) return false;
	if (!finite(q.center[0]) || !finite(q.center[1]) || !finite(q.center[2]) || !finite(q.size[0]) || q.size[0] < 0.0f) return false;
	if (q.shape == NH_SHAPE_SPHERE || (q.shape == NH_SHAPE_CAPSULE && q.size[1] == 0.0f)) return true;
	const int ns = q.shape == NH_SHAPE_BOX ? 3 : 2;
	for (int k = 1; k < ns; ++k) if (!finite(q.size[k]) || q.size[k] < 0.0f) return false;
	for (int k = 0; k < 4; ++k) if (!finite(q.rotation[k])) return false;
	return true;
}

static bool touches(const nh_OverlapQuery& q, const Rec& r, bool box) {
	const nh_f3 c = nh_make3(q.center[0], q.center[1], q.center[2]), h = nh_make3(q.size[0], q.size[1], q.size[2]);
	const nh_quat qr = { q.rotation[0], q.rotation[1], q.rotation[2], q.rotation[3] };
	const nh_f3 p = nh_make3(r.p[0], r.p[1], r.p[2]), rh = nh_make3(r.h[0], r.h[1], r.h[2]);
	const nh_quat rq = { r.q[0], r.q[1], r.q[2], r.q[3] };
	if (q.shape == NH_SHAPE_CAPSULE)
		return box ? nh_q_overlap_capsule_box(c, qr, h.x, h.y, p, rq, rh) : nh_q_overlap_capsule_sphere(c, qr, h.x, h.y, p, rh.x);
	const bool sphere = q.shape == NH_SHAPE_SPHERE;
	if (box) return sphere ? nh_q_overlap_sphere_box(c, h.x, p, rq, rh) : nh_q_overlap_box_box(c, qr, h, p, rq, rh);
	return sphere ? nh_q_overlap_sphere_sphere(c, h.x, p, rh.x) : nh_q_overlap_sphere_box(p, rh.x, c, qr, h);
}

static void out5(const nh_QHit& s, float out[5]) { out[0] = s.t; out[1] = s.n.x; out[2] = s.n.y; out[3] = s.n.z; out[4] = s.hit ? 1.0f : 0.0f; }

extern "C" {

// only >= 0: the answer of that one collider (combined index) alone, as the closest-hit rule would give it
void hc_capsulecast(const Rec* rec, uint32_t n, uint32_t nbox, const nh_CapsuleCast* casts, uint32_t count, nh_RayHit* hits, int64_t only, uint32_t threads) {
	parallel(count, threads, [=](uint32_t i) { cast_one(rec, n, nbox, casts[i], hits[i], only); });
}

// offsets: count + 1 words, always written (with the 32-bit wrap the device's scan has; offsets[count] = 0xffffffff on overflow).  hits: the records of
// every query whose segment ends at or below `capacity` (nothing on overflow); no other byte of `hits` is touched.  Returns the true total (64 bits).
uint64_t hc_overlap(const Rec* rec, uint32_t n, uint32_t nbox, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets, nh_OverlapHit* hits,
                    uint32_t capacity, uint32_t threads) {
	std::vector<uint32_t> cnt(count);
	parallel(count, threads, [&](uint32_t i) {
		uint32_t k = 0;
		if (valid(queries[i]))
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
		for (uint32_t c = 0; c < n; ++c) {
			if (rec[c].body == queries[i].ignore_body || !touches(queries[i], rec[c], c < nbox)) continue;
			nh_OverlapHit& o = hits[k++];
			o.body = rec[c].body; o.collider = c < nbox ? c : c - nbox; o.shape = c < nbox ? NH_SHAPE_BOX : NH_SHAPE_SPHERE; o.tag = rec[c].tag;
		}
	});
	return total;
}

// one collider alone, the predicate without the reach rule (the geometry tests): out = t, normal[3], hit (1.0 / 0.0)
void hc_sweep_capsule_box(const float o[3], const float d[3], const float q[4], float r, float hh, const float p[3], const float qb[4], const float hb[3], float out[5]) {
	out5(nh_q_sweep_capsule_box(nh_make3(o[0], o[1], o[2]), nh_make3(d[0], d[1], d[2]), nh_quat{ q[0], q[1], q[2], q[3] }, r, hh,
	                            nh_make3(p[0], p[1], p[2]), nh_quat{ qb[0], qb[1], qb[2], qb[3] }, nh_make3(hb[0], hb[1], hb[2])), out);
}

void hc_sweep_capsule_sphere(const float o[3], const float d[3], const float q[4], float r, float hh, const float c[3], float R, float out[5]) {
	out5(nh_q_sweep_capsule_sphere(nh_make3(o[0], o[1], o[2]), nh_make3(d[0], d[1], d[2]), nh_quat{ q[0], q[1], q[2], q[3] }, r, hh, nh_make3(c[0], c[1], c[2]), R), out);
}

int hc_overlap_capsule_box(const float c[3], const float q[4], float r, float hh, const float p[3], const float qb[4], const float hb[3]) {
	return nh_q_overlap_capsule_box(nh_make3(c[0], c[1], c[2]), nh_quat{ q[0], q[1], q[2], q[3] }, r, hh, nh_make3(p[0], p[1], p[2]), nh_quat{ qb[0], qb[1], qb[2], qb[3] },
	                                nh_make3(hb[0], hb[1], hb[2])) ? 1 : 0;
}

int hc_overlap_capsule_sphere(const float c[3], const float q[4], float r, float hh, const float p[3], float R) {
	return nh_q_overlap_capsule_sphere(nh_make3(c[0], c[1], c[2]), nh_quat{ q[0], q[1], q[2], q[3] }, r, hh, nh_make3(p[0], p[1], p[2]), R) ? 1 : 0;
}

// the capsule's half axis a = rotate(q, (0, hh, 0)) as the predicates compute it
void hc_capsule_axis(const float q[4], float hh, float out[3]) {
	const nh_f3 a = nh_q_capsule_axis(nh_quat{ q[0], q[1], q[2], q[3] }, hh);
	out[0] = a.x; out[1] = a.y; out[2] = a.z;
}

}
