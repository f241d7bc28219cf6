// hostquery.cpp -- CPU build of the scene query's per-item arithmetic (nudge_amd/csrc/nh_query.h), the oracle of the GPU's ray casts
// (tests/hostquery_util.py).
//   hq_records   the per-collider records k_q_xform writes: world pose, half extents | radius, body, tag
//   hq_raycast   closest hit (or the hit test of one collider) by brute force over all colliders, on several threads
#include "oracle.h"

static void cast_one(const Rec* rec, uint32_t n, uint32_t nbox, const nh_Ray& ray, nh_RayHit& out, int64_t only) {
	const nh_f3 o = v3(ray.origin), d = v3(ray.direction);
	const bool ok = finite(o.x) && finite(o.y) && finite(o.z) && finite(d.x) && finite(d.y) && finite(d.z);
	float bt = ray.max_t; uint32_t bc = 0xffffffffu; nh_f3 bn = nh_make3(0.0f, 0.0f, 0.0f);
	const uint32_t c0 = only >= 0 ? (uint32_t)only : 0u, c1 = only >= 0 ? (uint32_t)only + 1u : n;
	for (uint32_t c = ok ? c0 : c1; c < c1; ++c) {
		const Rec& r = rec[c];
		if (r.body == ray.ignore_body) continue;
		const nh_QHit h = c < nbox ? nh_q_ray_box(o, d, rec_pos(r), rec_rot(r), rec_half(r)) : nh_q_ray_sphere(o, d, rec_pos(r), r.h[0]);
		if (h.hit && nh_q_better(h.t, c, ray.max_t, bt, bc)) { bt = h.t; bc = c; bn = h.n; }
	}
	if (bc == 0xffffffffu) write_ray_miss(out, ok, ray.max_t);
	else write_ray_hit(out, rec, nbox, bc, bt, bn);
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
	parallel(count, threads, [=](uint32_t i) { cast_one(rec, n, nbox, rays[i], hits[i], only); });
}

// one shape alone (the geometry tests): out = t, normal[3], hit (1.0 / 0.0)
void hq_ray_box(const float o[3], const float d[3], const float p[3], const float q[4], const float h[3], float out[5]) {
	out5(nh_q_ray_box(v3(o), v3(d), v3(p), q4(q), v3(h)), out);
}

void hq_ray_sphere(const float o[3], const float d[3], const float c[3], float radius, float out[5]) { out5(nh_q_ray_sphere(v3(o), v3(d), v3(c), radius), out); }

void hq_pose(const float bpos[3], const float brot[4], const float lpos[3], const float lrot[4], float out[7]) {
	const nh_QPose w = nh_q_pose(bpos, brot, lpos, lrot);
	out[0] = w.p.x; out[1] = w.p.y; out[2] = w.p.z; out[3] = w.q.x; out[4] = w.q.y; out[5] = w.q.z; out[6] = w.q.s;
}

}
