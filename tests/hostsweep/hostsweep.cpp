// hostsweep.cpp -- CPU build of the sphere-cast arithmetic of nudge_amd/csrc/nh_query.h, the oracle of the GPU's nh_spherecast.
// Built with g++ -ffp-contract=off (tests/hostsweep_util.py), so that every function returns the device's bits; loaded with ctypes.
//   hs_spherecast  closest hit (or the hit of one collider) by brute force over all colliders, with the header's exact rules -- invalid casts,
//                  ignore_body, ties, the reach rule for r > 0 (the leaf box rebuilt as the build stores it) -- on several threads
//   hs_*           the single-collider predicates alone
#include <stdint.h>
#include <math.h>
#include <thread>
#include <vector>
#include "../../include/nudge_hip.h"
#include "../../nudge_amd/csrc/nh_query.h"

// 12 words per collider (tests/hostquery_util.py REC, nh_query.hip's nh_QRec): position, bits(body), rotation, half extents | radius (x3), bits(tag)
struct Rec { float p[3]; uint32_t body; float q[4]; float h[3]; uint32_t tag; };

static bool finite(float x) { return (nh_asuint(x) & 0x7f800000u) != 0x7f800000u; }

static void cast_one(const Rec* rec, uint32_t n, uint32_t nbox, const nh_SphereCast& sc, nh_RayHit& out, int64_t only) {
	const nh_f3 o = nh_make3(sc.origin[0], sc.origin[1], sc.origin[2]), d = nh_make3(sc.direction[0], sc.direction[1], sc.direction[2]);
	const float r = sc.radius;
	const bool ok = finite(o.x) && finite(o.y) && finite(o.z) && finite(d.x) && finite(d.y) && finite(d.z) && finite(r) && !(r < 0.0f);
	const nh_f3 inv = nh_make3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
	const float w = r + nh_q_cast_pad(o, r);
	float bt = sc.max_t; uint32_t bc = 0xffffffffu; nh_f3 bn = nh_make3(0.0f, 0.0f, 0.0f);
	const uint32_t c0 = only >= 0 ? (uint32_t)only : 0u, c1 = only >= 0 ? (uint32_t)only + 1u : n;
	for (uint32_t c = ok ? c0 : c1; c < c1; ++c) {
		const Rec& e = rec[c];
		if (e.body == sc.ignore_body) continue;
		const bool box = c < nbox;
		const nh_f3 p = nh_make3(e.p[0], e.p[1], e.p[2]), h = nh_make3(e.h[0], e.h[1], e.h[2]);
		const nh_quat q = { e.q[0], e.q[1], e.q[2], e.q[3] };
		nh_QHit hit = box ? nh_q_sweep_box(o, d, r, p, q, h) : nh_q_sweep_sphere(o, d, r, p, h.x);
		if (!hit.hit) continue;
		if (r > 0.0f) {
			// the reach rule: the leaf box must be entered, and the hit is no earlier than that entry
			nh_f3 lo, hi;
			nh_q_leaf_box(p, q, h, box, lo, hi);
			float t0;
			if (!nh_q_cast_node(lo, hi, o, inv, w, t0)) continue;
			if (t0 > hit.t) hit.t = t0;
		}
		if (nh_q_better(hit.t, c, sc.max_t, bt, bc)) { bt = hit.t; bc = c; bn = hit.n; }
	}
	if (bc == 0xffffffffu) {
		out.t = ok ? sc.max_t : nh_asfloat(0x7fc00000u); out.normal[0] = out.normal[1] = out.normal[2] = 0.0f;
		out.body = out.collider = out.tag = 0xffffffffu; out.shape = NH_SHAPE_NONE;
	} else {
		out.t = bt; out.normal[0] = bn.x; out.normal[1] = bn.y; out.normal[2] = bn.z;
		out.body = rec[bc].body; out.collider = bc < nbox ? bc : bc - nbox; out.shape = bc < nbox ? NH_SHAPE_BOX : NH_SHAPE_SPHERE; out.tag = rec[bc].tag;
	}
}

extern "C" {

// only >= 0: the answer of that one collider (combined index) alone, as the closest-hit rule would give it
void hs_spherecast(const Rec* rec, uint32_t n, uint32_t nbox, const nh_SphereCast* casts, uint32_t count, nh_RayHit* hits, int64_t only, uint32_t threads) {
	if (threads < 1) threads = 1;
	std::vector<std::thread> pool;
	for (uint32_t k = 0; k < threads; ++k)
		pool.emplace_back([=]() { for (uint32_t i = k; i < count; i += threads) cast_one(rec, n, nbox, casts[i], hits[i], only); });
	for (auto& t : pool) t.join();
}

// one collider alone, the predicate without the reach rule (the geometry tests): out = t, normal[3], hit (1.0 / 0.0)
void hs_sweep_box(const float o[3], const float d[3], float r, const float p[3], const float q[4], const float h[3], float out[5]) {
	const nh_quat qq = { q[0], q[1], q[2], q[3] };
	const nh_QHit s = nh_q_sweep_box(nh_make3(o[0], o[1], o[2]), nh_make3(d[0], d[1], d[2]), r, nh_make3(p[0], p[1], p[2]), qq, nh_make3(h[0], h[1], h[2]));
	out[0] = s.t; out[1] = s.n.x; out[2] = s.n.y; out[3] = s.n.z; out[4] = s.hit ? 1.0f : 0.0f;
}

void hs_sweep_sphere(const float o[3], const float d[3], float r, const float c[3], float R, float out[5]) {
	const nh_QHit s = nh_q_sweep_sphere(nh_make3(o[0], o[1], o[2]), nh_make3(d[0], d[1], d[2]), r, nh_make3(c[0], c[1], c[2]), R);
	out[0] = s.t; out[1] = s.n.x; out[2] = s.n.y; out[3] = s.n.z; out[4] = s.hit ? 1.0f : 0.0f;
}

}
