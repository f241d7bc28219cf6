// hostboxcast.cpp -- CPU build of the box-cast arithmetic of nudge_amd/csrc/nh_query.h, the oracle of the GPU's nh_boxcast.
// Built with g++ -ffp-contract=off (tests/hostboxcast_util.py), so that every function returns the device's bits; loaded with ctypes.
//   hb_boxcast     closest hit (or the hit of one collider) by brute force over all colliders, with the header's exact rules -- invalid casts,
//                  size 0 as a ray, ignore_body, ties, the reach rule for a nonzero size (the leaf box rebuilt as the build stores it) -- on several threads
//   hb_*           the single-collider predicates alone
#include <stdint.h>
#include <math.h>
#include <thread>
#include <vector>
#include "../../include/nudge_hip.h"
#include "../../nudge_amd/csrc/nh_query.h"

// 12 words per collider (tests/hostquery_util.py REC, nh_query.hip's nh_QRec): position, bits(body), rotation, half extents | radius (x3), bits(tag)
struct Rec { float p[3]; uint32_t body; float q[4]; float h[3]; uint32_t tag; };

static bool finite(float x) { return (nh_asuint(x) & 0x7f800000u) != 0x7f800000u; }

static void cast_one(const Rec* rec, uint32_t n, uint32_t nbox, const nh_BoxCast& bc_, nh_RayHit& out, int64_t only) {
	const nh_f3 o = nh_make3(bc_.origin[0], bc_.origin[1], bc_.origin[2]), d = nh_make3(bc_.direction[0], bc_.direction[1], bc_.direction[2]);
	const nh_f3 ha = nh_make3(bc_.size[0], bc_.size[1], bc_.size[2]);
	const nh_quat qa = { bc_.rotation[0], bc_.rotation[1], bc_.rotation[2], bc_.rotation[3] };
	const bool ray = ha.x == 0.0f && ha.y == 0.0f && ha.z == 0.0f;
	const bool ok = finite(o.x) && finite(o.y) && finite(o.z) && finite(d.x) && finite(d.y) && finite(d.z) && finite(ha.x) && finite(ha.y) && finite(ha.z) &&
	                !(ha.x < 0.0f) && !(ha.y < 0.0f) && !(ha.z < 0.0f) && (ray || (finite(qa.x) && finite(qa.y) && finite(qa.z) && finite(qa.s)));
	const nh_f3 inv = nh_make3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
	const nh_f3 e = ray ? nh_make3(0.0f, 0.0f, 0.0f) : nh_q_box_extent(qa, ha);
	const float s = nh_q_cast_pad(o, fmaxf(fmaxf(e.x, e.y), e.z));
	const nh_f3 w = nh_make3(e.x + s, e.y + s, e.z + s);
	float bt = bc_.max_t; uint32_t bc = 0xffffffffu; nh_f3 bn = nh_make3(0.0f, 0.0f, 0.0f);
	const uint32_t c0 = only >= 0 ? (uint32_t)only : 0u, c1 = only >= 0 ? (uint32_t)only + 1u : n;
	for (uint32_t c = ok ? c0 : c1; c < c1; ++c) {
		const Rec& r = rec[c];
		if (r.body == bc_.ignore_body) continue;
		const bool box = c < nbox;
		const nh_f3 p = nh_make3(r.p[0], r.p[1], r.p[2]), h = nh_make3(r.h[0], r.h[1], r.h[2]);
		const nh_quat q = { r.q[0], r.q[1], r.q[2], r.q[3] };
		nh_QHit hit = box ? nh_q_sweep_box_box(o, d, qa, ha, p, q, h) : nh_q_sweep_box_sphere(o, d, qa, ha, p, h.x);
		if (!hit.hit) continue;
		if (!ray) {
			// the reach rule: the leaf box must be entered, and the hit is no earlier than that entry
			nh_f3 lo, hi;
			nh_q_leaf_box(p, q, h, box, lo, hi);
			float t0;
			if (!nh_q_cast_node3(lo, hi, o, inv, w, t0)) continue;
			if (t0 > hit.t) hit.t = t0;
		}
		if (nh_q_better(hit.t, c, bc_.max_t, bt, bc)) { bt = hit.t; bc = c; bn = hit.n; }
	}
	if (bc == 0xffffffffu) {
		out.t = ok ? bc_.max_t : nh_asfloat(0x7fc00000u); out.normal[0] = out.normal[1] = out.normal[2] = 0.0f;
		out.body = out.collider = out.tag = 0xffffffffu; out.shape = NH_SHAPE_NONE;
	} else {
		out.t = bt; out.normal[0] = bn.x; out.normal[1] = bn.y; out.normal[2] = bn.z;
		out.body = rec[bc].body; out.collider = bc < nbox ? bc : bc - nbox; out.shape = bc < nbox ? NH_SHAPE_BOX : NH_SHAPE_SPHERE; out.tag = rec[bc].tag;
	}
}

extern "C" {

// only >= 0: the answer of that one collider (combined index) alone, as the closest-hit rule would give it
void hb_boxcast(const Rec* rec, uint32_t n, uint32_t nbox, const nh_BoxCast* casts, uint32_t count, nh_RayHit* hits, int64_t only, uint32_t threads) {
	if (threads < 1) threads = 1;
	std::vector<std::thread> pool;
	for (uint32_t k = 0; k < threads; ++k)
		pool.emplace_back([=]() { for (uint32_t i = k; i < count; i += threads) cast_one(rec, n, nbox, casts[i], hits[i], only); });
	for (auto& t : pool) t.join();
}

// one collider alone, the predicate without the reach rule (the geometry tests): out = t, normal[3], hit (1.0 / 0.0)
void hb_sweep_box_box(const float o[3], const float d[3], const float qa[4], const float ha[3], const float p[3], const float qb[4], const float hb[3], float out[5]) {
	const nh_QHit s = nh_q_sweep_box_box(nh_make3(o[0], o[1], o[2]), nh_make3(d[0], d[1], d[2]), nh_quat{ qa[0], qa[1], qa[2], qa[3] }, nh_make3(ha[0], ha[1], ha[2]),
	                                     nh_make3(p[0], p[1], p[2]), nh_quat{ qb[0], qb[1], qb[2], qb[3] }, nh_make3(hb[0], hb[1], hb[2]));
	out[0] = s.t; out[1] = s.n.x; out[2] = s.n.y; out[3] = s.n.z; out[4] = s.hit ? 1.0f : 0.0f;
}

void hb_sweep_box_sphere(const float o[3], const float d[3], const float qa[4], const float ha[3], const float c[3], float R, float out[5]) {
	const nh_QHit s = nh_q_sweep_box_sphere(nh_make3(o[0], o[1], o[2]), nh_make3(d[0], d[1], d[2]), nh_quat{ qa[0], qa[1], qa[2], qa[3] }, nh_make3(ha[0], ha[1], ha[2]),
	                                        nh_make3(c[0], c[1], c[2]), R);
	out[0] = s.t; out[1] = s.n.x; out[2] = s.n.y; out[3] = s.n.z; out[4] = s.hit ? 1.0f : 0.0f;
}

}
