// hostoverlap.cpp -- CPU build of the overlap predicates of nudge_amd/csrc/nh_query.h, the oracle of the GPU's nh_overlap.
// Built with g++ -ffp-contract=off (tests/hostoverlap_util.py), so that every predicate returns the device's answer; loaded with ctypes.
//   ho_overlap   offsets and records of a batch of queries by brute force over all colliders, with the header's exact semantics
//                (ignore_body, invalid queries, capacity prefix, the 2^32 - 1 marker), on several threads
//   ho_*         the three predicates alone
#include <stdint.h>
#include <string.h>
#include <thread>
#include <vector>
#include "../../include/nudge_hip.h"
#include "../../nudge_amd/csrc/nh_query.h"

// 12 words per collider (tests/hostquery_util.py REC, nh_query.hip's nh_QRec): position, bits(body), rotation, half extents | radius (x3), bits(tag)
struct Rec { float p[3]; uint32_t body; float q[4]; float h[3]; uint32_t tag; };

static bool finite(float x) { return (nh_asuint(x) & 0x7f800000u) != 0x7f800000u; }

static bool valid(const nh_OverlapQuery& q) {
	if (q.shape != NH_SHAPE_SPHERE && q.shape != NH_SHAPE_BOX) return false;
	if (!finite(q.center[0]) || !finite(q.center[1]) || !finite(q.center[2]) || !finite(q.size[0]) || q.size[0] < 0.0f) return false;
	if (q.shape == NH_SHAPE_SPHERE) return true;
	for (int k = 1; k < 3; ++k) if (!finite(q.size[k]) || q.size[k] < 0.0f) return false;
	for (int k = 0; k < 4; ++k) if (!finite(q.rotation[k])) return false;
	return true;
}

static bool touches(const nh_OverlapQuery& q, const Rec& r, bool box) {
	const nh_f3 c = nh_make3(q.center[0], q.center[1], q.center[2]), h = nh_make3(q.size[0], q.size[1], q.size[2]);
	const nh_quat qr = { q.rotation[0], q.rotation[1], q.rotation[2], q.rotation[3] };
	const nh_f3 p = nh_make3(r.p[0], r.p[1], r.p[2]), rh = nh_make3(r.h[0], r.h[1], r.h[2]);
	const nh_quat rq = { r.q[0], r.q[1], r.q[2], r.q[3] };
	const bool sphere = q.shape == NH_SHAPE_SPHERE;
	if (box) return sphere ? nh_q_overlap_sphere_box(c, h.x, p, rq, rh) : nh_q_overlap_box_box(c, qr, h, p, rq, rh);
	return sphere ? nh_q_overlap_sphere_sphere(c, h.x, p, rh.x) : nh_q_overlap_sphere_box(p, rh.x, c, qr, h);
}

template <class F> static void parallel(uint32_t count, uint32_t threads, F f) {
	if (threads < 1) threads = 1;
	std::vector<std::thread> pool;
	for (uint32_t k = 0; k < threads; ++k) pool.emplace_back([=]() { for (uint32_t i = k; i < count; i += threads) f(i); });
	for (auto& t : pool) t.join();
}

extern "C" {

// offsets: count + 1 words, always written (with the 32-bit wrap the device's scan has; offsets[count] = 0xffffffff on overflow).  hits: the records of
// every query whose segment ends at or below `capacity` (nothing on overflow); no other byte of `hits` is touched.  Returns the true total (64 bits).
uint64_t ho_overlap(const Rec* rec, uint32_t n, uint32_t nbox, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets, nh_OverlapHit* hits,
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

int ho_sphere_sphere(const float c[3], float r, const float p[3], float R) {
	return nh_q_overlap_sphere_sphere(nh_make3(c[0], c[1], c[2]), r, nh_make3(p[0], p[1], p[2]), R) ? 1 : 0;
}

int ho_sphere_box(const float c[3], float r, const float p[3], const float q[4], const float h[3]) {
	const nh_quat qq = { q[0], q[1], q[2], q[3] };
	return nh_q_overlap_sphere_box(nh_make3(c[0], c[1], c[2]), r, nh_make3(p[0], p[1], p[2]), qq, nh_make3(h[0], h[1], h[2])) ? 1 : 0;
}

int ho_box_box(const float ca[3], const float qa[4], const float ha[3], const float cb[3], const float qb[4], const float hb[3]) {
	const nh_quat a = { qa[0], qa[1], qa[2], qa[3] }, b = { qb[0], qb[1], qb[2], qb[3] };
	return nh_q_overlap_box_box(nh_make3(ca[0], ca[1], ca[2]), a, nh_make3(ha[0], ha[1], ha[2]), nh_make3(cb[0], cb[1], cb[2]), b, nh_make3(hb[0], hb[1], hb[2])) ? 1 : 0;
}

}
