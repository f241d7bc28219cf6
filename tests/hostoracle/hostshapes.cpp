// hostshapes.cpp -- CPU build of the scene query's per-item arithmetic (nudge_amd/csrc/nh_query.h) one item at a time, for the geometry tests
// (tests/hostquery_util.py, tests/hostcast_util.py, tests/hostcapsule_util.py).
//   hq_records   the per-collider records k_q_xform writes: world pose, half extents | radius, body, tag
//   hq_pose      one collider's world pose
//   hq_ray_*, hs_sweep_*, hb_sweep_*, hc_sweep_*   the single-collider cast predicates alone, without the reach rule: out = t, normal[3], hit (1.0 / 0.0)
//   hc_overlap_capsule_*, hc_capsule_axis         the capsule's overlap predicates and its half axis
#include "oracle.h"

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

void hq_pose(const float bpos[3], const float brot[4], const float lpos[3], const float lrot[4], float out[7]) {
	const nh_QPose w = nh_q_pose(bpos, brot, lpos, lrot);
	out[0] = w.p.x; out[1] = w.p.y; out[2] = w.p.z; out[3] = w.q.x; out[4] = w.q.y; out[5] = w.q.z; out[6] = w.q.s;
}

void hq_ray_box(const float o[3], const float d[3], const float p[3], const float q[4], const float h[3], float out[5]) {
	out5(nh_q_ray_box(v3(o), v3(d), v3(p), q4(q), v3(h)), out);
}

void hq_ray_sphere(const float o[3], const float d[3], const float c[3], float radius, float out[5]) { out5(nh_q_ray_sphere(v3(o), v3(d), v3(c), radius), out); }

void hs_sweep_box(const float o[3], const float d[3], float r, const float p[3], const float q[4], const float h[3], float out[5]) {
	out5(nh_q_sweep_box(v3(o), v3(d), r, v3(p), q4(q), v3(h)), out);
}

void hs_sweep_sphere(const float o[3], const float d[3], float r, const float c[3], float R, float out[5]) {
	out5(nh_q_sweep_sphere(v3(o), v3(d), r, v3(c), R), out);
}

void hb_sweep_box_box(const float o[3], const float d[3], const float qa[4], const float ha[3], const float p[3], const float qb[4], const float hb[3], float out[5]) {
	out5(nh_q_sweep_box_box(v3(o), v3(d), q4(qa), v3(ha), v3(p), q4(qb), v3(hb)), out);
}

void hb_sweep_box_sphere(const float o[3], const float d[3], const float qa[4], const float ha[3], const float c[3], float R, float out[5]) {
	out5(nh_q_sweep_box_sphere(v3(o), v3(d), q4(qa), v3(ha), v3(c), R), out);
}

void hc_sweep_capsule_box(const float o[3], const float d[3], const float q[4], float r, float hh, const float p[3], const float qb[4], const float hb[3], float out[5]) {
	out5(nh_q_sweep_capsule_box(v3(o), v3(d), q4(q), r, hh, v3(p), q4(qb), v3(hb)), out);
}

void hc_sweep_capsule_sphere(const float o[3], const float d[3], const float q[4], float r, float hh, const float c[3], float R, float out[5]) {
	out5(nh_q_sweep_capsule_sphere(v3(o), v3(d), q4(q), r, hh, v3(c), R), out);
}

int hc_overlap_capsule_box(const float c[3], const float q[4], float r, float hh, const float p[3], const float qb[4], const float hb[3]) {
	return nh_q_overlap_capsule_box(v3(c), q4(q), r, hh, v3(p), q4(qb), v3(hb)) ? 1 : 0;
}

int hc_overlap_capsule_sphere(const float c[3], const float q[4], float r, float hh, const float p[3], float R) {
	return nh_q_overlap_capsule_sphere(v3(c), q4(q), r, hh, v3(p), R) ? 1 : 0;
}

// the capsule's half axis a = rotate(q, (0, hh, 0)) as the predicates compute it
void hc_capsule_axis(const float q[4], float hh, float out[3]) {
	const nh_f3 a = nh_q_capsule_axis(q4(q), hh);
	out[0] = a.x; out[1] = a.y; out[2] = a.z;
}

}
