// hostquery.cpp -- CPU build of the scene query's per-item arithmetic (nudge_amd/csrc/nh_query.h), the oracle of the GPU's ray casts.
// Built with g++ -ffp-contract=off (tests/hostquery_util.py), so that every function returns the device's bits; loaded with ctypes.
//   hq_records   the per-collider records k_q_xform writes: world pose, half extents | radius, body, tag
//   hq_raycast   closest hit (or the hit test of one collider) by brute force over all colliders, on several threads
#include <stdint.h>
#include <math.h>
#include <thread>
#include <vector>
#include "../../include/nudge_hip.h"
#include "../../nudge_amd/csrc/nh_query.h"

// 12 words per collider: position, bits(body), rotation, half extents | radius (x3), bits(tag)
struct Rec { float p[3]; uint32_t body; float q[4]; float h[3]; uint32_t tag; };

static bool finite(float x) { return (nh_asuint(x) & 0x7f800000u) != 0x7f800000u; }

static nh_QHit eval(const Rec& r, bool box, nh_f3 o, nh_f3 d) {
	const nh_f3 p = nh_make3(r.p[0], r.p[1], r.p[2]);
	if (box) { const nh_quat q = { r.q[0], r.q[1], r.q[2], r.q[3] }; return nh_q_ray_box(o, d, p, q, nh_make3(r.h[0], r.h[1], r.h[2])); }
	return nh_q_ray_sphere(o, d, p, r.h[0]);
}

static void cast_one(const Rec* rec, uint32_t n, uint32_t nbox, const nh_Ray& ray, nh_RayHit& out, int64_t only) {
	const nh_f3 o = nh_make3(ray.origin[0], ray.origin[1], ray.origin[2]), d = nh_make3(ray.direction[0], ray.direction[1], ray.direction[2]);
	const bool ok = finite(o.x) && finite(o.y) && finite(o.z) && finite(d.x) && finite(d.y) && finite(d.z);
	float bt = ray.max_t; uint32_t bc = 0xffffffffu; nh_f3 bn = nh_make3(0.0f, 0.0f, 0.0f);
	const uint32_t c0 = only >= 0 ? (uint32_t)only : 0u, c1 = only >= 0 ? (uint32_t)only + 1u : n;
	for (uint32_t c = ok ? c0 : c1; c < c1; ++c) {
		if (rec[c].body == ray.ignore_body) continue;
		const nh_QHit h = eval(rec[c], c < nbox, o, d);
		if (h.hit && nh_q_better(h.t, c, ray.max_t, bt, bc)) { bt = h.t; bc = c; bn = h.n; }
	}
	if (bc == 0xffffffffu) {
		out.t = ok ? ray.max_t : nh_asfloat(0x7fc00000u); out.normal[0] = out.normal[1] = out.normal[2] = 0.0f;
		out.body = out.collider = out.tag = 0xffffffffu; out.shape = NH_SHAPE_NONE;
	} else {
		out.t = bt; out.normal[0] = bn.x; out.normal[1] = bn.y; out.normal[2] = bn.z;
		out.body = rec[bc].body; out.collider = bc < nbox ? bc : bc - nbox; out.shape = bc < nbox ? NH_SHAPE_BOX : NH_SHAPE_SPHERE; out.tag = rec[bc].tag;
	}
}

extern "C" {

void hq_records(const nh_Transform* body_xf, uint32_t nbodies, uint32_t nbox, const nh_Transform* box_xf, const nh_BoxCollider* box_data, const uint32_t* box_tags,
                uint32_t nsph, const nh_Transform* sph_xf, const nh_SphereCollider* sph_data, const uint32_t* sph_tags, Rec* out) {
	for (uint32_t c = 0; c < nbox + nsph; ++c) {
		const bool box = c < nbox;
		const nh_Transform& l = box ? box_xf[c] : sph_xf[c - nbox];
		Rec& r = out[c];
		if (l.body < nbodies) {
			const nh_Transform& b = body_xf[l.body];
			const nh_QPose w = nh_q_pose(b.position, b.rotation, l.position, l.rotation);
			r.p[0] = w.p.x; r.p[1] = w.p.y; r.p[2] = w.p.z; r.q[0] = w.q.x; r.q[1] = w.q.y; r.q[2] = w.q.z; r.q[3] = w.q.s;
		} else {
			const float nan = nh_asfloat(0x7fc00000u);
			r.p[0] = r.p[1] = r.p[2] = nan; r.q[0] = r.q[1] = r.q[2] = r.q[3] = nan;
		}
		r.body = l.body;
		if (box) { r.h[0] = box_data[c].size[0]; r.h[1] = box_data[c].size[1]; r.h[2] = box_data[c].size[2]; r.tag = box_tags[c]; }
		else { r.h[0] = r.h[1] = r.h[2] = sph_data[c - nbox].radius; r.tag = sph_tags[c - nbox]; }
	}
}

// only >= 0: the answer of that one collider (combined index) alone, as the closest-hit rule would give it
void hq_raycast(const Rec* rec, uint32_t n, uint32_t nbox, const nh_Ray* rays, uint32_t count, nh_RayHit* hits, int64_t only, uint32_t threads) {
	if (threads < 1) threads = 1;
	std::vector<std::thread> pool;
	for (uint32_t k = 0; k < threads; ++k)
		pool.emplace_back([=]() { for (uint32_t i = k; i < count; i += threads) cast_one(rec, n, nbox, rays[i], hits[i], only); });
	for (auto& t : pool) t.join();
}

// one shape alone (the geometry tests): out = t, normal[3], hit (1.0 / 0.0)
void hq_ray_box(const float o[3], const float d[3], const float p[3], const float q[4], const float h[3], float out[5]) {
	const nh_quat qq = { q[0], q[1], q[2], q[3] };
	const nh_QHit r = nh_q_ray_box(nh_make3(o[0], o[1], o[2]), nh_make3(d[0], d[1], d[2]), nh_make3(p[0], p[1], p[2]), qq, nh_make3(h[0], h[1], h[2]));
	out[0] = r.t; out[1] = r.n.x; out[2] = r.n.y; out[3] = r.n.z; out[4] = r.hit ? 1.0f : 0.0f;
}

void hq_ray_sphere(const float o[3], const float d[3], const float c[3], float radius, float out[5]) {
	const nh_QHit r = nh_q_ray_sphere(nh_make3(o[0], o[1], o[2]), nh_make3(d[0], d[1], d[2]), nh_make3(c[0], c[1], c[2]), radius);
	out[0] = r.t; out[1] = r.n.x; out[2] = r.n.y; out[3] = r.n.z; out[4] = r.hit ? 1.0f : 0.0f;
}

void hq_pose(const float bpos[3], const float brot[4], const float lpos[3], const float lrot[4], float out[7]) {
	const nh_QPose w = nh_q_pose(bpos, brot, lpos, lrot);
	out[0] = w.p.x; out[1] = w.p.y; out[2] = w.p.z; out[3] = w.q.x; out[4] = w.q.y; out[5] = w.q.z; out[6] = w.q.s;
}

}
