// hostpen.cpp -- CPU build of the penetration arithmetic of nudge_amd/csrc/nh_query.h, the oracle of the GPU's nh_penetration.
// Built with g++ -ffp-contract=off (tests/hostpen_util.py), so that every function returns the device's bits; loaded with ctypes.
//   hp_penetration  offsets and 32-byte records of a batch of sphere, box and capsule queries by brute force over all colliders, with the header's exact
//                   rules: nh_overlap's validity, predicates, ignore_body, order, capacity prefix and 2^32 - 1 marker, and the pair function of each record
//   hp_pen_*        the six pair functions alone: out = normal[3], depth
//   hp_touches      nh_overlap's predicate of one query against one collider
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

static nh_QPen pen(const nh_OverlapQuery& q, const Rec& r, bool box) {
	const nh_f3 c = nh_make3(q.center[0], q.center[1], q.center[2]), h = nh_make3(q.size[0], q.size[1], q.size[2]);
	const nh_quat qr = { q.rotation[0], q.rotation[1], q.rotation[2], q.rotation[3] };
	const nh_f3 p = nh_make3(r.p[0], r.p[1], r.p[2]), rh = nh_make3(r.h[0], r.h[1], r.h[2]);
	const nh_quat rq = { r.q[0], r.q[1], r.q[2], r.q[3] };
	if (q.shape == NH_SHAPE_CAPSULE)
		return box ? nh_q_pen_capsule_box(c, qr, h.x, h.y, p, rq, rh) : nh_q_pen_capsule_sphere(c, qr, h.x, h.y, p, rh.x);
	const bool sphere = q.shape == NH_SHAPE_SPHERE;
	if (box) return sphere ? nh_q_pen_sphere_box(c, h.x, p, rq, rh) : nh_q_pen_box_box(c, qr, h, p, rq, rh);
	return sphere ? nh_q_pen_sphere_sphere(c, h.x, p, rh.x) : nh_q_pen_box_sphere(c, qr, h, p, rh.x);
}

static nh_f3 v3(const float a[3]) { return nh_make3(a[0], a[1], a[2]); }
static nh_quat q4(const float a[4]) { return nh_quat{ a[0], a[1], a[2], a[3] }; }
static void out4(const nh_QPen& o, float out[4]) { out[0] = o.n.x; out[1] = o.n.y; out[2] = o.n.z; out[3] = o.depth; }

extern "C" {

// offsets: count + 1 words, always written (with the 32-bit wrap the device's scan has; offsets[count] = 0xffffffff on overflow).  hits: the records of
// every query whose segment ends at or below `capacity` (nothing on overflow); no other byte of `hits` is touched.  Returns the true total (64 bits).
uint64_t hp_penetration(const Rec* rec, uint32_t n, uint32_t nbox, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets, nh_PenetrationHit* hits,
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
			const nh_QPen o = pen(queries[i], rec[c], c < nbox);
			nh_PenetrationHit& w = hits[k++];
			w.normal[0] = o.n.x; w.normal[1] = o.n.y; w.normal[2] = o.n.z; w.depth = o.depth;
			w.body = rec[c].body; w.collider = c < nbox ? c : c - nbox; w.shape = c < nbox ? NH_SHAPE_BOX : NH_SHAPE_SPHERE; w.tag = rec[c].tag;
		}
	});
	return total;
}

// one query against one collider record: nh_overlap's predicate (validity included), and the pair function
int hp_touches(const nh_OverlapQuery* q, const Rec* r, int box) { return valid(*q) && touches(*q, *r, box != 0) ? 1 : 0; }
void hp_pen(const nh_OverlapQuery* q, const Rec* r, int box, float out[4]) { out4(pen(*q, *r, box != 0), out); }

// the same two over `count` pairs (query i against record i; box[i] != 0: a box collider): ok[i] = the predicate, out[4 i ..] = normal, depth
void hp_pairs(const nh_OverlapQuery* q, const Rec* r, const uint8_t* box, uint32_t count, uint8_t* ok, float* out) {
	for (uint32_t i = 0; i < count; ++i) {
		ok[i] = valid(q[i]) && touches(q[i], r[i], box[i] != 0) ? 1 : 0;
		out4(pen(q[i], r[i], box[i] != 0), out + 4 * i);
	}
}

void hp_pen_sphere_sphere(const float c[3], float r, const float p[3], float R, float out[4]) { out4(nh_q_pen_sphere_sphere(v3(c), r, v3(p), R), out); }
void hp_pen_sphere_box(const float c[3], float r, const float p[3], const float q[4], const float h[3], float out[4]) {
	out4(nh_q_pen_sphere_box(v3(c), r, v3(p), q4(q), v3(h)), out);
}
void hp_pen_box_sphere(const float ca[3], const float qa[4], const float ha[3], const float p[3], float R, float out[4]) {
	out4(nh_q_pen_box_sphere(v3(ca), q4(qa), v3(ha), v3(p), R), out);
}
void hp_pen_capsule_sphere(const float c[3], const float q[4], float r, float hh, const float p[3], float R, float out[4]) {
	out4(nh_q_pen_capsule_sphere(v3(c), q4(q), r, hh, v3(p), R), out);
}
void hp_pen_box_box(const float ca[3], const float qa[4], const float ha[3], const float cb[3], const float qb[4], const float hb[3], float out[4]) {
	out4(nh_q_pen_box_box(v3(ca), q4(qa), v3(ha), v3(cb), q4(qb), v3(hb)), out);
}
void hp_pen_capsule_box(const float c[3], const float q[4], float r, float hh, const float p[3], const float qb[4], const float hb[3], float out[4]) {
	out4(nh_q_pen_capsule_box(v3(c), q4(q), r, hh, v3(p), q4(qb), v3(hb)), out);
}

// nh_q_point_box's signed distance of a point (the exactness test of sphere / box)
float hp_point_box_distance(const float x[3], const float p[3], const float q[4], const float h[3]) { return nh_q_point_box(v3(x), v3(p), q4(q), v3(h)).d; }

}
