// nh_query.h -- per-item arithmetic of the scene query (nh_query_build / nh_raycast, nh_query.hip): a collider's world pose, and a ray
// against one box and against one sphere.
//
// Every function is `NH_HD` so that tests/hostquery builds the SAME arithmetic with g++ -ffp-contract=off and gets the device's bits: the
// brute force over all colliders there is the oracle of the GPU's tree traversal.  Only + - * /, sqrtf (correctly rounded on both sides)
// and sign / absolute-value bit operations are used.
//
// Exact semantics (include/nudge_hip.h, "scene queries"):
//   box     (size = half extents, as in the narrowphase): the ray is brought into the box frame by the inverse rotation, then a slab test.
//           A direction component that is exactly zero makes its slab all or nothing, decided by |o_k| <= h_k (no 0 * inf).  Entry t = the
//           largest slab entry (the first axis on equality); the normal is the entering slab's local axis, signed against the direction,
//           rotated back to world.
//   sphere  a = d.d, m = o - c, b = m.d, disc = b*b - a*(m.m - r*r), t = (-b - sqrtf(disc)) / a, normal = (o + t*d - c) * (1/r).
//   inside  (every box slab contains o, or m.m <= r*r): t = 0, normal = -d / sqrtf(d.d).
//   A hit counts if 0 <= t <= max_t; the closest hit is the smallest t, ties broken by (shape, collider index) ascending -- with the boxes
//   first in the collider numbering that is the order of the combined index c (boxes 0 .. nbox-1, then the spheres).
#ifndef NH_QUERY_H
#define NH_QUERY_H

#include "nh_math.h"

// A collider's world pose: Transform * Transform of the body and the collider's local transform (nudge.cpp:1165-1175), k_xform's arithmetic.
struct nh_QPose { nh_f3 p; nh_quat q; };
NH_HD nh_QPose nh_q_pose(const float bpos[3], const float brot[4], const float lpos[3], const float lrot[4]) {
	const nh_quat bq = { brot[0], brot[1], brot[2], brot[3] };
	const nh_quat lq = { lrot[0], lrot[1], lrot[2], lrot[3] };
	nh_QPose w;
	w.p = nh_rotate(bq, nh_make3(lpos[0], lpos[1], lpos[2])) + nh_make3(bpos[0], bpos[1], bpos[2]);
	w.q = nh_qmul(bq, lq);
	return w;
}

// World AABB half extents of a box: |R| * size (nudge.cpp:3027-3037, k_xform)
NH_HD nh_f3 nh_q_box_extent(nh_quat q, nh_f3 h) {
	const nh_m33 m = nh_matrix(q);
	const nh_f3 c0 = m.c0 * h.x, c1 = m.c1 * h.y, c2 = m.c2 * h.z;
	return nh_make3(nh_abs(c0.x) + nh_abs(c1.x) + nh_abs(c2.x), nh_abs(c0.y) + nh_abs(c1.y) + nh_abs(c2.y), nh_abs(c0.z) + nh_abs(c1.z) + nh_abs(c2.z));
}

struct nh_QHit { float t; nh_f3 n; bool hit; };

NH_HD nh_QHit nh_q_inside(nh_f3 d) {
	const float s = sqrtf(nh_dot(d, d));
	nh_QHit r;
	r.t = 0.0f; r.n = nh_make3(nh_neg(d.x) / s, nh_neg(d.y) / s, nh_neg(d.z) / s); r.hit = true;
	return r;
}

// one slab of the box test: updates the entry / exit and the entering axis; `all` = false when a zero direction component leaves o outside
NH_HD void nh_q_slab(float o, float d, float h, int axis, float& t0, float& t1, int& enter, bool& all) {
	if (d == 0.0f) {
		if (!(nh_abs(o) <= h)) all = false;
		return;
	}
	const float a = (nh_neg(h) - o) / d, b = (h - o) / d;
	const float lo = b < a ? b : a, hi = b < a ? a : b;
	if (lo > t0) { t0 = lo; enter = axis; }
	if (hi < t1) t1 = hi;
}

// Ray (o, d) against the box of world pose (p, q) and half extents h.  hit = false: no intersection in front of or around the origin
// (t < 0 is reported as a miss here; the caller applies max_t).
NH_HD nh_QHit nh_q_ray_box(nh_f3 o, nh_f3 d, nh_f3 p, nh_quat q, nh_f3 h) {
	const nh_quat qi = { nh_neg(q.x), nh_neg(q.y), nh_neg(q.z), q.s };
	const nh_f3 ol = nh_rotate(qi, o - p), dl = nh_rotate(qi, d);
	nh_QHit r; r.t = 0.0f; r.n = nh_make3(0.0f, 0.0f, 0.0f); r.hit = false;
	if (nh_abs(ol.x) <= h.x && nh_abs(ol.y) <= h.y && nh_abs(ol.z) <= h.z) return nh_q_inside(d);
	float t0 = -INFINITY, t1 = INFINITY;
	int enter = -1;
	bool all = true;
	nh_q_slab(ol.x, dl.x, h.x, 0, t0, t1, enter, all);
	nh_q_slab(ol.y, dl.y, h.y, 1, t0, t1, enter, all);
	nh_q_slab(ol.z, dl.z, h.z, 2, t0, t1, enter, all);
	if (!all || enter < 0 || !(t0 <= t1) || !(t0 >= 0.0f)) return r;
	const float dk = enter == 0 ? dl.x : enter == 1 ? dl.y : dl.z;
	const float s = dk > 0.0f ? -1.0f : 1.0f;
	const nh_f3 nl = nh_make3(enter == 0 ? s : 0.0f, enter == 1 ? s : 0.0f, enter == 2 ? s : 0.0f);
	r.t = t0; r.n = nh_rotate(q, nl); r.hit = true;
	return r;
}

// Ray (o, d) against the sphere of centre c and radius rad.
NH_HD nh_QHit nh_q_ray_sphere(nh_f3 o, nh_f3 d, nh_f3 c, float rad) {
	nh_QHit r; r.t = 0.0f; r.n = nh_make3(0.0f, 0.0f, 0.0f); r.hit = false;
	const nh_f3 m = o - c;
	const float mm = nh_dot(m, m), rr = rad * rad;
	if (mm <= rr) return nh_q_inside(d);
	const float a = nh_dot(d, d), b = nh_dot(m, d);
	const float disc = b * b - a * (mm - rr);
	if (!(disc >= 0.0f)) return r;
	const float t = (nh_neg(b) - sqrtf(disc)) / a;
	if (!(t >= 0.0f)) return r;
	const float inv = 1.0f / rad;
	r.t = t; r.n = ((o + t * d) - c) * inv; r.hit = true;
	return r;
}

// Does (t, c) beat the best hit so far (bt, bc)?  bc = 0xffffffff: none yet.  Counting needs 0 <= t <= max_t.
NH_HD bool nh_q_better(float t, uint32_t c, float max_t, float bt, uint32_t bc) {
	if (!(t >= 0.0f && t <= max_t)) return false;
	return bc == 0xffffffffu || t < bt || (t == bt && c < bc);
}

#endif
