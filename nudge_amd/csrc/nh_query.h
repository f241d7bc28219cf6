// nh_query.h -- per-item arithmetic of the scene query (nh_query_build / nh_raycast / nh_overlap, nh_query.hip): a collider's world pose, a ray
// against one box and against one sphere, and the overlap predicates of a query sphere or box against one collider.
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

// ---- overlap (nh_overlap): does a query shape touch a collider?  Closed sets: touching counts ----------------------------------------------
// Each predicate reads "overlap iff every test holds with <=", so a NaN anywhere fails a test and gives NO overlap (the collider of a body that
// does not exist has a NaN pose).  These are geometric queries, not contact generation: nothing is shared with the narrowphase's SAT.

// sphere (c, r) against sphere (p, R): m = c - p, overlap iff m.m <= (r + R)^2
NH_HD bool nh_q_overlap_sphere_sphere(nh_f3 c, float r, nh_f3 p, float R) {
	const nh_f3 m = c - p;
	const float s = r + R;
	return nh_dot(m, m) <= s * s;
}

// sphere (c, r) against the box of world pose (p, q) and half extents h -- a sphere query against a box collider and a box query against a sphere
// collider alike.  The centre is brought into the box frame by the inverse rotation (as nh_q_ray_box does) and clamped to [-h, h]; overlap iff the
// squared distance to the clamped point is <= r^2.  Per axis that distance is |l| - h where positive, 0 inside (l - clamp(l) is +-(|l| - h), the
// same bits squared); a NaN keeps its NaN through `e <= 0 ? 0 : e`.
NH_HD bool nh_q_overlap_sphere_box(nh_f3 c, float r, nh_f3 p, nh_quat q, nh_f3 h) {
	const nh_quat qi = { nh_neg(q.x), nh_neg(q.y), nh_neg(q.z), q.s };
	const nh_f3 l = nh_rotate(qi, c - p);
	const float ex = nh_abs(l.x) - h.x, ey = nh_abs(l.y) - h.y, ez = nh_abs(l.z) - h.z;
	const float dx = ex <= 0.0f ? 0.0f : ex, dy = ey <= 0.0f ? 0.0f : ey, dz = ez <= 0.0f ? 0.0f : ez;
	return dx * dx + dy * dy + dz * dz <= r * r;
}

// Box a (ca, qa, ha) -- the QUERY box -- against box b (cb, qb, hb) -- the collider: the 15 separating axes in a's frame (Gottschalk, Lin & Manocha
// 1996, "OBBTree"; Ericson, Real-Time Collision Detection 4.4.1), R = Ra^T Rb (R_ij = A_i . B_j), t = Ra^T (cb - ca).  The radii use
// E_ij = |R_ij| + 2^-20: when an edge of a is (nearly) parallel to an edge of b, their cross product is (nearly) zero and both sides of its test are
// rounding noise, so without the epsilon a pair of boxes that overlaps could be separated by a degenerate axis.  The epsilon is above the rounding of
// R for unit quaternions (a few ulp of 1) and only ever widens the radii: it can add a touch, never remove one.  What it adds is bounded by three
// more tests, first: the two world AABBs -- c -+ nh_q_box_extent, the very bounds the build (k_q_xform) and the query walk compute before padding --
// must touch.  Exact boxes that overlap have touching AABBs (up to rounding), and a pair the epsilon lets through is at least in the tree's reach:
// the padded node boxes contain these bounds, so the walk can never prune what this predicate accepts.
#define NH_Q_SAT_EPS 9.5367431640625e-07f
NH_HD bool nh_q_overlap_box_box(nh_f3 ca, nh_quat qa, nh_f3 ha, nh_f3 cb, nh_quat qb, nh_f3 hb) {
	const nh_f3 ea = nh_q_box_extent(qa, ha), eb = nh_q_box_extent(qb, hb);
	if (!((cb.x - eb.x) <= (ca.x + ea.x) && (ca.x - ea.x) <= (cb.x + eb.x) && (cb.y - eb.y) <= (ca.y + ea.y) && (ca.y - ea.y) <= (cb.y + eb.y) &&
	      (cb.z - eb.z) <= (ca.z + ea.z) && (ca.z - ea.z) <= (cb.z + eb.z))) return false;
	const nh_m33 A = nh_matrix(qa), B = nh_matrix(qb);
	const nh_f3 d = cb - ca;
	const float t0 = nh_dot(A.c0, d), t1 = nh_dot(A.c1, d), t2 = nh_dot(A.c2, d);
	const float R00 = nh_dot(A.c0, B.c0), R01 = nh_dot(A.c0, B.c1), R02 = nh_dot(A.c0, B.c2);
	const float R10 = nh_dot(A.c1, B.c0), R11 = nh_dot(A.c1, B.c1), R12 = nh_dot(A.c1, B.c2);
	const float R20 = nh_dot(A.c2, B.c0), R21 = nh_dot(A.c2, B.c1), R22 = nh_dot(A.c2, B.c2);
	const float E00 = nh_abs(R00) + NH_Q_SAT_EPS, E01 = nh_abs(R01) + NH_Q_SAT_EPS, E02 = nh_abs(R02) + NH_Q_SAT_EPS;
	const float E10 = nh_abs(R10) + NH_Q_SAT_EPS, E11 = nh_abs(R11) + NH_Q_SAT_EPS, E12 = nh_abs(R12) + NH_Q_SAT_EPS;
	const float E20 = nh_abs(R20) + NH_Q_SAT_EPS, E21 = nh_abs(R21) + NH_Q_SAT_EPS, E22 = nh_abs(R22) + NH_Q_SAT_EPS;
	const float a0 = ha.x, a1 = ha.y, a2 = ha.z, b0 = hb.x, b1 = hb.y, b2 = hb.z;
	// a's face normals A_0 .. A_2
	bool ok = nh_abs(t0) <= a0 + (b0 * E00 + b1 * E01 + b2 * E02);
	ok = ok && nh_abs(t1) <= a1 + (b0 * E10 + b1 * E11 + b2 * E12);
	ok = ok && nh_abs(t2) <= a2 + (b0 * E20 + b1 * E21 + b2 * E22);
	// b's face normals B_0 .. B_2
	ok = ok && nh_abs(t0 * R00 + t1 * R10 + t2 * R20) <= (a0 * E00 + a1 * E10 + a2 * E20) + b0;
	ok = ok && nh_abs(t0 * R01 + t1 * R11 + t2 * R21) <= (a0 * E01 + a1 * E11 + a2 * E21) + b1;
	ok = ok && nh_abs(t0 * R02 + t1 * R12 + t2 * R22) <= (a0 * E02 + a1 * E12 + a2 * E22) + b2;
	// edge x edge: A_i x B_j
	ok = ok && nh_abs(t2 * R10 - t1 * R20) <= (a1 * E20 + a2 * E10) + (b1 * E02 + b2 * E01);
	ok = ok && nh_abs(t2 * R11 - t1 * R21) <= (a1 * E21 + a2 * E11) + (b0 * E02 + b2 * E00);
	ok = ok && nh_abs(t2 * R12 - t1 * R22) <= (a1 * E22 + a2 * E12) + (b0 * E01 + b1 * E00);
	ok = ok && nh_abs(t0 * R20 - t2 * R00) <= (a0 * E20 + a2 * E00) + (b1 * E12 + b2 * E11);
	ok = ok && nh_abs(t0 * R21 - t2 * R01) <= (a0 * E21 + a2 * E01) + (b0 * E12 + b2 * E10);
	ok = ok && nh_abs(t0 * R22 - t2 * R02) <= (a0 * E22 + a2 * E02) + (b0 * E11 + b1 * E10);
	ok = ok && nh_abs(t1 * R00 - t0 * R10) <= (a0 * E10 + a1 * E00) + (b1 * E22 + b2 * E21);
	ok = ok && nh_abs(t1 * R01 - t0 * R11) <= (a0 * E11 + a1 * E01) + (b0 * E22 + b2 * E20);
	ok = ok && nh_abs(t1 * R02 - t0 * R12) <= (a0 * E12 + a1 * E02) + (b0 * E21 + b1 * E20);
	return ok;
}

#endif
