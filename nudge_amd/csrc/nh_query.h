// nh_query.h -- per-item arithmetic of the scene query (nh_query_build / nh_raycast / nh_spherecast / nh_boxcast / nh_capsulecast / nh_overlap /
// nh_closest / nh_distance, nh_query.hip): a collider's world pose, a ray against one box and against one sphere, the overlap predicates of a query sphere, box or
// capsule against one collider, a swept ball, box and capsule against one box and one sphere, the signed distance of a point from one box and one
// sphere, the per-plane test of nh_region, the ray of a (sensor, beam) of nh_sense, the sweep of a collider along its own velocity of nh_sweep, with the walk's node tests they are pruned by.
//
// Every function is `NH_HD` so that tests/hostquery (hostoverlap, hostsweep, hostboxcast, hostcapsule, hostpoint, hostregion) builds the SAME arithmetic with g++ -ffp-contract=off and gets the device's bits: the
// brute force over all colliders there is the oracle of the GPU's tree traversal.  Only + - * /, sqrtf (correctly rounded on both sides)
// and sign / absolute-value bit operations are used (and fminf / fmaxf in the pads and the walk's node test, which agree on both sides).
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

// A collider's world pose and a box's world AABB half extents under the query layer's names: the step's own functions (nh_math.h), so a query sees the very
// colliders the step collides
struct nh_QPose { nh_f3 p; nh_quat q; };
NH_HD nh_QPose nh_q_pose(const float bpos[3], const float brot[4], const float lpos[3], const float lrot[4]) {
	nh_QPose w;
	nh_collider_pose(bpos, brot, lpos, lrot, w.p, w.q);
	return w;
}
NH_HD nh_f3 nh_q_box_extent(nh_quat q, nh_f3 h) { return nh_box_reach(q, h); }

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

// The cut of the box pass (nh_query_build.hip, k_q_boxes_runs / k_q_boxes_top): the leaves, in key order, are cut into runs of NH_Q_RUN.  A Karras node
// covers the contiguous leaf range [first, last] and its own index is one end of it, so a node whose range lies in ONE run has its index, both
// children and their whole subtrees in that run (its workgroup merges it in LDS, slot = index - run start); every other node CROSSES a run boundary
// and belongs to the top phase.  k_q_tree writes the verdict on a node's PARENT next to the parent's index (parents are internal nodes: < 2^30), with
// the side the node hangs on: the left child of a split at g has index g, the right child g + 1, leaf or not.
#define NH_Q_RUN 1024u
#define NH_Q_PARENT_TOP 0x80000000u      // the parent crosses a run boundary (the root's parent word, 0xffffffff, reads as "top" as well)
#define NH_Q_PARENT_RIGHT 0x40000000u    // this node is its parent's right child
#define NH_Q_PARENT_ID 0x3fffffffu
NH_HD bool nh_q_run_crossing(uint32_t first, uint32_t last) { return first / NH_Q_RUN != last / NH_Q_RUN; }
NH_HD uint32_t nh_q_parent_word(uint32_t parent, bool right, bool top) {
	return parent | (right ? NH_Q_PARENT_RIGHT : 0u) | (top ? NH_Q_PARENT_TOP : 0u);
}

// Conservative box of a leaf (k_q_boxes_runs): a relative pad of 2^-18 of its largest coordinate, so that no rounding of the walk's slab tests can cut off a
// collider the exact test hits (the cast side adds the same of its origin, k_q_raycast / k_q_spherecast)
NH_HD float nh_q_pad(nh_f3 mn, nh_f3 mx) {
	const float m = fmaxf(fmaxf(fmaxf(fabsf(mn.x), fabsf(mn.y)), fmaxf(fabsf(mn.z), fabsf(mx.x))), fmaxf(fabsf(mx.y), fabsf(mx.z)));
	return m * 3.814697265625e-06f + 1e-30f;
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
// more tests, first: the two world AABBs -- c -+ nh_q_box_extent, the very bounds the build (k_q_boxes_runs) and the query walk compute before padding --
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

// ---- sphere casts (nh_spherecast): the first t at which the ball of radius r centred at o + t d touches a collider --------------------------------
// The hit is that of the ray against the collider grown by r (its Minkowski sum with the ball): the normal points from the collider to the centre.
// A ball that touches at t = 0 under nh_overlap's predicates hits at t = 0 with the ray's inside normal -d / |d|.  r = 0 is a ray cast, bit for bit.

// First entry t >= 0 of the ray (o, d) into the ball of centre c, radius r; INFINITY when there is none.  The closest-approach form (Hearn & Baker; Haines
// et al., "Precision Improvements for Ray / Sphere Intersection", Ray Tracing Gems 7): disc = r^2 - |m + t_m d|^2 with t_m = -m.d / d.d, so that a grazing
// ray keeps its accuracy when m is much longer than r.  An origin inside the ball (by rounding: callers have ruled out a real start overlap) gives t = 0.
NH_HD float nh_q_ball_entry(nh_f3 o, nh_f3 d, nh_f3 c, float r) {
	const nh_f3 m = o - c;
	const float a = nh_dot(d, d);
	if (!(a > 0.0f)) return INFINITY;
	const float tm = nh_neg(nh_dot(m, d)) / a;
	const nh_f3 l = m + tm * d;
	const float q = r * r - nh_dot(l, l);
	if (!(q >= 0.0f)) return INFINITY;
	const float dt = sqrtf(q / a);
	if (!(tm + dt >= 0.0f)) return INFINITY;
	const float t = tm - dt;
	return t > 0.0f ? t : 0.0f;
}

// First entry t >= 0 of a ray in a box frame into the capsule of radius r around the box edge parallel to axis k through (ci, cj) on the other two axes
// i, j, from -hk to +hk on k: the least of its side (the infinite cylinder's entry, if it lies within [-hk, hk]) and its two end balls (a ray that enters
// the finite cylinder through an end disc is inside that end's ball already).  INFINITY when there is none.
NH_HD float nh_q_capsule_entry(float oi, float oj, float ok, float di, float dj, float dk, float ci, float cj, float hk, float r) {
	float t = INFINITY;
	const float mi = oi - ci, mj = oj - cj;
	const float a = di * di + dj * dj;
	if (a > 0.0f) {
		const float tm = nh_neg(mi * di + mj * dj) / a;
		const float li = mi + tm * di, lj = mj + tm * dj;
		const float q = r * r - (li * li + lj * lj);
		if (q >= 0.0f) {
			const float dt = sqrtf(q / a);
			if (tm + dt >= 0.0f) {
				const float ts = tm - dt > 0.0f ? tm - dt : 0.0f;
				const float xk = ok + ts * dk;
				if (nh_abs(xk) <= hk) t = ts;
			}
		}
	}
	const nh_f3 o3 = nh_make3(oi, oj, ok), d3 = nh_make3(di, dj, dk);
	const float t0 = nh_q_ball_entry(o3, d3, nh_make3(ci, cj, nh_neg(hk)), r), t1 = nh_q_ball_entry(o3, d3, nh_make3(ci, cj, hk), r);
	t = t0 < t ? t0 : t;
	return t1 < t ? t1 : t;
}

// The ball (o + t d, r) against the box of world pose (p, q) and half extents h (Ericson, Real-Time Collision Detection 5.5.7).  In the box frame
// (nh_q_ray_box's): the start overlap by nh_q_overlap_sphere_box; otherwise the ray's entry into the box grown by r on every side (nh_q_slab with h + r,
// from t = 0 on) is classified by the coordinates that lie beyond +-h: none or one -- a face region, and that entry is the hit, the entering slab's axis
// the normal; two -- an edge region, the hit is on that edge's capsule or nowhere; three -- a vertex region, the least hit on its three capsules.  An edge
// or vertex hit's normal is the hit centre minus its closest point on the box (its clamp to [-h, h]), normalised.  r = 0: nh_q_ray_box itself.
NH_HD nh_QHit nh_q_sweep_box(nh_f3 o, nh_f3 d, float r, nh_f3 p, nh_quat q, nh_f3 h) {
	if (r == 0.0f) return nh_q_ray_box(o, d, p, q, h);
	if (nh_q_overlap_sphere_box(o, r, p, q, h)) return nh_q_inside(d);
	nh_QHit res; res.t = 0.0f; res.n = nh_make3(0.0f, 0.0f, 0.0f); res.hit = false;
	const nh_quat qi = { nh_neg(q.x), nh_neg(q.y), nh_neg(q.z), q.s };
	const nh_f3 ol = nh_rotate(qi, o - p), dl = nh_rotate(qi, d);
	float t0 = -INFINITY, t1 = INFINITY;
	int enter = -1;
	bool all = true;
	nh_q_slab(ol.x, dl.x, h.x + r, 0, t0, t1, enter, all);
	nh_q_slab(ol.y, dl.y, h.y + r, 1, t0, t1, enter, all);
	nh_q_slab(ol.z, dl.z, h.z + r, 2, t0, t1, enter, all);
	if (!all || enter < 0 || !(t0 <= t1) || !(t1 >= 0.0f)) return res;
	const float tc = t0 > 0.0f ? t0 : 0.0f;
	const nh_f3 e = ol + tc * dl;
	const float sx = e.x < nh_neg(h.x) ? -1.0f : e.x > h.x ? 1.0f : 0.0f;
	const float sy = e.y < nh_neg(h.y) ? -1.0f : e.y > h.y ? 1.0f : 0.0f;
	const float sz = e.z < nh_neg(h.z) ? -1.0f : e.z > h.z ? 1.0f : 0.0f;
	const int beyond = (sx != 0.0f) + (sy != 0.0f) + (sz != 0.0f);
	if (beyond <= 1) {
		// (an origin inside the grown box in a face region is within r of the box: a start overlap that rounding kept from the test above)
		if (!(t0 > 0.0f)) return nh_q_inside(d);
		const float dk = enter == 0 ? dl.x : enter == 1 ? dl.y : dl.z;
		const float s = dk > 0.0f ? -1.0f : 1.0f;
		res.t = t0; res.n = nh_rotate(q, nh_make3(enter == 0 ? s : 0.0f, enter == 1 ? s : 0.0f, enter == 2 ? s : 0.0f)); res.hit = true;
		return res;
	}
	float t = INFINITY;
	if (sx != 0.0f && sy != 0.0f) t = nh_q_capsule_entry(ol.x, ol.y, ol.z, dl.x, dl.y, dl.z, sx * h.x, sy * h.y, h.z, r);
	if (sx != 0.0f && sz != 0.0f) { const float u = nh_q_capsule_entry(ol.z, ol.x, ol.y, dl.z, dl.x, dl.y, sz * h.z, sx * h.x, h.y, r); t = u < t ? u : t; }
	if (sy != 0.0f && sz != 0.0f) { const float u = nh_q_capsule_entry(ol.y, ol.z, ol.x, dl.y, dl.z, dl.x, sy * h.y, sz * h.z, h.x, r); t = u < t ? u : t; }
	if (!(t < INFINITY)) return res;
	const nh_f3 x = ol + t * dl;
	nh_f3 v = nh_make3(x.x - nh_max(nh_neg(h.x), nh_min(x.x, h.x)), x.y - nh_max(nh_neg(h.y), nh_min(x.y, h.y)), x.z - nh_max(nh_neg(h.z), nh_min(x.z, h.z)));
	float vv = nh_dot(v, v);
	if (!(vv > 0.0f)) { v = nh_make3(sx, sy, sz); vv = nh_dot(v, v); }         // (r below the rounding of the coordinates: the region's direction)
	const float len = sqrtf(vv);
	res.t = t; res.n = nh_rotate(q, nh_make3(v.x / len, v.y / len, v.z / len)); res.hit = true;
	return res;
}

// The ball (o + t d, r) against the sphere collider (c, R): the ray against the sphere of radius R + r -- its start test is nh_q_overlap_sphere_sphere's
// to the bit, and r = 0 is nh_q_ray_sphere itself.
NH_HD nh_QHit nh_q_sweep_sphere(nh_f3 o, nh_f3 d, float r, nh_f3 c, float R) { return nh_q_ray_sphere(o, d, c, R + r); }

// The walk's node test of a cast (k_q_spherecast): the slab test of the ray against the node box grown by w = r + s (s: the cast's pad), with the
// ray cast's operations (k_q_raycast: w = s).  Entered iff t0 <= t1 and t1 >= 0; t0 = the entry.
NH_HD bool nh_q_cast_node(nh_f3 lo, nh_f3 hi, nh_f3 o, nh_f3 inv, float w, float& t0) {
	const float ax = ((lo.x - w) - o.x) * inv.x, bx = ((hi.x + w) - o.x) * inv.x;
	const float ay = ((lo.y - w) - o.y) * inv.y, by = ((hi.y + w) - o.y) * inv.y;
	const float az = ((lo.z - w) - o.z) * inv.z, bz = ((hi.z + w) - o.z) * inv.z;
	t0 = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
	const float t1 = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
	return t0 <= t1 && t1 >= 0.0f;
}

// The box of a leaf as the build stores it (the world AABB and the pad of k_q_boxes_runs): what the host rebuilds to apply the sweep's reach rule.
NH_HD void nh_q_leaf_box(nh_f3 p, nh_quat q, nh_f3 h, bool box, nh_f3& lo, nh_f3& hi) {
	const nh_f3 e = box ? nh_q_box_extent(q, h) : h;
	const nh_f3 mn = p - e, mx = p + e;
	const float pad = nh_q_pad(mn, mx);
	lo = nh_make3(mn.x - pad, mn.y - pad, mn.z - pad);
	hi = nh_make3(mx.x + pad, mx.y + pad, mx.z + pad);
}

// The sweep's pad and the reach rule.  A cast of radius r > 0 hits a collider at t = max(t_pred, t_leaf) where t_pred is the predicate's
// t and t_leaf the entry into the collider's leaf box under nh_q_cast_node -- and not at all when that box is not entered.  Every ancestor box contains
// the leaf box and the node test is monotone in the box, so the walk reaches every collider this rule lets hit at or before the best t so far, whatever
// the rounding of t_pred.  The clamp changes t only where t_pred lies in front of a box padded by 2^-18 of the coordinates around the grown collider.
NH_HD float nh_q_cast_pad(nh_f3 o, float r) { return fmaxf(fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z)), r) * 3.814697265625e-06f; }

// ---- box casts (nh_boxcast): the first t at which the box of pose (o + t d, qa) and half extents ha touches a collider ------------------------------
// The box translates only.  A box that touches at t = 0 under nh_overlap's own predicates (nh_q_overlap_box_box with the cast box as the query,
// nh_q_overlap_sphere_box) hits at t = 0 with the ray's inside normal -d / |d|.  ha = (0, 0, 0) is a ray cast, bit for bit, and qa is not read.

// One separating axis of the translational SAT: the projected centre distance is s - tau u, and the axis holds while |s - tau u| <= rho.  [te, tx] is
// narrowed to that interval at t = base + tau.  A `lead` axis may give the normal: its lower end enters at `axis` when it is the largest lower end of the
// lead axes so far (tn; the first axis on equality), and ue is then its u.  u == 0: all or nothing, |s| <= rho (no 0 * inf).  A NaN fails the axis.
NH_HD void nh_q_sat_axis(float s, float u, float rho, float base, int axis, bool lead, float& te, float& tn, float& tx, int& enter, float& ue, bool& all) {
	if (u == 0.0f) {
		if (!(nh_abs(s) <= rho)) all = false;
		return;
	}
	const float a = base + (s - rho) / u, b = base + (s + rho) / u;
	const float lo = b < a ? b : a, hi = b < a ? a : b;
	if (!(lo <= hi)) all = false;
	if (lo > te) te = lo;
	if (lead && lo > tn) { tn = lo; enter = axis; ue = u; }
	if (hi < tx) tx = hi;
}

// The cast box (o + t d, qa, ha) against the box collider (p, qb, hb): the translational form of nh_q_overlap_box_box's 15 axes -- the same frame (the
// cast box's), the same R = Ra^T Rb and radii with E = |R| + 2^-20 -- where each axis is a t interval, the entry t is the largest lower end, and a hit
// needs every interval to hold with t_enter <= t_exit, t_exit >= 0.  ha = 0: nh_q_ray_box.  A start contact that only this rounding finds
// (t_enter <= 0) also returns the inside rule.
// Near-parallel edges: the six face axes are solved first from the centres, and the edge axes from the centres at the face entry
// tb = max(t_face, 0), where the boxes are within their sizes of each other -- so the rounding of a (nearly) zero cross axis is a few ulp of the
// sizes, which the 2^-20 of its radius covers, and it cannot separate boxes that touch however far the cast started.  Every axis bounds t; but an
// edge pair whose squared cross product |A_i x B_j|^2 (read off R) is below 2^-20 (edges within ~1e-3 rad of parallel) never gives the normal, whose
// direction would be rounding noise.  The normal is the LEAD axis that closes last (faces of the cast box, faces of the collider, then the other
// edge pairs; the first on equality), from the collider to the cast box, normalised, signed against the direction.
NH_HD nh_QHit nh_q_sweep_box_box(nh_f3 o, nh_f3 d, nh_quat qa, nh_f3 ha, nh_f3 p, nh_quat qb, nh_f3 hb) {
	if (ha.x == 0.0f && ha.y == 0.0f && ha.z == 0.0f) return nh_q_ray_box(o, d, p, qb, hb);
	if (nh_q_overlap_box_box(o, qa, ha, p, qb, hb)) return nh_q_inside(d);
	nh_QHit res; res.t = 0.0f; res.n = nh_make3(0.0f, 0.0f, 0.0f); res.hit = false;
	const nh_m33 A = nh_matrix(qa), B = nh_matrix(qb);
	const nh_f3 m = p - o;
	const float t0 = nh_dot(A.c0, m), t1 = nh_dot(A.c1, m), t2 = nh_dot(A.c2, m);
	const float u0 = nh_dot(A.c0, d), u1 = nh_dot(A.c1, d), u2 = nh_dot(A.c2, d);
	const float R00 = nh_dot(A.c0, B.c0), R01 = nh_dot(A.c0, B.c1), R02 = nh_dot(A.c0, B.c2);
	const float R10 = nh_dot(A.c1, B.c0), R11 = nh_dot(A.c1, B.c1), R12 = nh_dot(A.c1, B.c2);
	const float R20 = nh_dot(A.c2, B.c0), R21 = nh_dot(A.c2, B.c1), R22 = nh_dot(A.c2, B.c2);
	const float E00 = nh_abs(R00) + NH_Q_SAT_EPS, E01 = nh_abs(R01) + NH_Q_SAT_EPS, E02 = nh_abs(R02) + NH_Q_SAT_EPS;
	const float E10 = nh_abs(R10) + NH_Q_SAT_EPS, E11 = nh_abs(R11) + NH_Q_SAT_EPS, E12 = nh_abs(R12) + NH_Q_SAT_EPS;
	const float E20 = nh_abs(R20) + NH_Q_SAT_EPS, E21 = nh_abs(R21) + NH_Q_SAT_EPS, E22 = nh_abs(R22) + NH_Q_SAT_EPS;
	const float a0 = ha.x, a1 = ha.y, a2 = ha.z, b0 = hb.x, b1 = hb.y, b2 = hb.z;
	float te = -INFINITY, tn = -INFINITY, tx = INFINITY, ue = 0.0f;
	int enter = -1;
	bool all = true;
	// a's face normals A_0 .. A_2, then b's B_0 .. B_2, from the centres at t = 0
	nh_q_sat_axis(t0, u0, a0 + (b0 * E00 + b1 * E01 + b2 * E02), 0.0f, 0, true, te, tn, tx, enter, ue, all);
	nh_q_sat_axis(t1, u1, a1 + (b0 * E10 + b1 * E11 + b2 * E12), 0.0f, 1, true, te, tn, tx, enter, ue, all);
	nh_q_sat_axis(t2, u2, a2 + (b0 * E20 + b1 * E21 + b2 * E22), 0.0f, 2, true, te, tn, tx, enter, ue, all);
	nh_q_sat_axis(t0 * R00 + t1 * R10 + t2 * R20, u0 * R00 + u1 * R10 + u2 * R20, (a0 * E00 + a1 * E10 + a2 * E20) + b0, 0.0f, 3, true, te, tn, tx, enter, ue, all);
	nh_q_sat_axis(t0 * R01 + t1 * R11 + t2 * R21, u0 * R01 + u1 * R11 + u2 * R21, (a0 * E01 + a1 * E11 + a2 * E21) + b1, 0.0f, 4, true, te, tn, tx, enter, ue, all);
	nh_q_sat_axis(t0 * R02 + t1 * R12 + t2 * R22, u0 * R02 + u1 * R12 + u2 * R22, (a0 * E02 + a1 * E12 + a2 * E22) + b2, 0.0f, 5, true, te, tn, tx, enter, ue, all);
	if (!all || !(te <= tx) || !(tx >= 0.0f)) return res;
	// edge x edge: A_i x B_j, from the centres at the face entry; a near-parallel pair bounds t but does not lead
	const float tb = te > 0.0f ? te : 0.0f;
	const nh_f3 mb = p - (o + tb * d);
	const float v0 = nh_dot(A.c0, mb), v1 = nh_dot(A.c1, mb), v2 = nh_dot(A.c2, mb);
	nh_q_sat_axis(v2 * R10 - v1 * R20, u2 * R10 - u1 * R20, (a1 * E20 + a2 * E10) + (b1 * E02 + b2 * E01), tb, 6, R10 * R10 + R20 * R20 >= NH_Q_SAT_EPS, te, tn, tx, enter, ue, all);
	nh_q_sat_axis(v2 * R11 - v1 * R21, u2 * R11 - u1 * R21, (a1 * E21 + a2 * E11) + (b0 * E02 + b2 * E00), tb, 7, R11 * R11 + R21 * R21 >= NH_Q_SAT_EPS, te, tn, tx, enter, ue, all);
	nh_q_sat_axis(v2 * R12 - v1 * R22, u2 * R12 - u1 * R22, (a1 * E22 + a2 * E12) + (b0 * E01 + b1 * E00), tb, 8, R12 * R12 + R22 * R22 >= NH_Q_SAT_EPS, te, tn, tx, enter, ue, all);
	nh_q_sat_axis(v0 * R20 - v2 * R00, u0 * R20 - u2 * R00, (a0 * E20 + a2 * E00) + (b1 * E12 + b2 * E11), tb, 9, R00 * R00 + R20 * R20 >= NH_Q_SAT_EPS, te, tn, tx, enter, ue, all);
	nh_q_sat_axis(v0 * R21 - v2 * R01, u0 * R21 - u2 * R01, (a0 * E21 + a2 * E01) + (b0 * E12 + b2 * E10), tb, 10, R01 * R01 + R21 * R21 >= NH_Q_SAT_EPS, te, tn, tx, enter, ue, all);
	nh_q_sat_axis(v0 * R22 - v2 * R02, u0 * R22 - u2 * R02, (a0 * E22 + a2 * E02) + (b0 * E11 + b1 * E10), tb, 11, R02 * R02 + R22 * R22 >= NH_Q_SAT_EPS, te, tn, tx, enter, ue, all);
	nh_q_sat_axis(v1 * R00 - v0 * R10, u1 * R00 - u0 * R10, (a0 * E10 + a1 * E00) + (b1 * E22 + b2 * E21), tb, 12, R00 * R00 + R10 * R10 >= NH_Q_SAT_EPS, te, tn, tx, enter, ue, all);
	nh_q_sat_axis(v1 * R01 - v0 * R11, u1 * R01 - u0 * R11, (a0 * E11 + a1 * E01) + (b0 * E22 + b2 * E20), tb, 13, R01 * R01 + R11 * R11 >= NH_Q_SAT_EPS, te, tn, tx, enter, ue, all);
	nh_q_sat_axis(v1 * R02 - v0 * R12, u1 * R02 - u0 * R12, (a0 * E12 + a1 * E02) + (b0 * E21 + b1 * E20), tb, 14, R02 * R02 + R12 * R12 >= NH_Q_SAT_EPS, te, tn, tx, enter, ue, all);
	if (!all || enter < 0 || !(te <= tx) || !(tx >= 0.0f)) return res;
	if (!(te > 0.0f)) return nh_q_inside(d);
	// the entering axis in world space: A_k, B_k or A_i x B_j
	nh_f3 L;
	if (enter < 3) L = enter == 0 ? A.c0 : enter == 1 ? A.c1 : A.c2;
	else if (enter < 6) L = enter == 3 ? B.c0 : enter == 4 ? B.c1 : B.c2;
	else {
		const int i = (enter - 6) / 3, j = (enter - 6) % 3;
		L = nh_cross(i == 0 ? A.c0 : i == 1 ? A.c1 : A.c2, j == 0 ? B.c0 : j == 1 ? B.c1 : B.c2);
	}
	// entering at the lower end: u > 0 puts the collider on the +L side of the cast box, so the normal is -L (which closes with u, whatever closed last)
	const float len = sqrtf(nh_dot(L, L));
	const nh_f3 n = nh_make3(L.x / len, L.y / len, L.z / len);
	res.t = te; res.n = ue > 0.0f ? nh_make3(nh_neg(n.x), nh_neg(n.y), nh_neg(n.z)) : n; res.hit = true;
	return res;
}

// The cast box (o + t d, qa, ha) against the sphere collider (c, R): the ball swept by -d against the box at rest, nh_q_sweep_box(c, -d, R, o, qa, ha),
// with its normal negated (from the sphere to the box).  The start test is nh_q_overlap_sphere_box(c, R, o, qa, ha), nh_overlap's predicate of a box
// query against a sphere collider, answered with nh_q_inside(d) itself; ha = 0: nh_q_ray_sphere.
NH_HD nh_QHit nh_q_sweep_box_sphere(nh_f3 o, nh_f3 d, nh_quat qa, nh_f3 ha, nh_f3 c, float R) {
	if (ha.x == 0.0f && ha.y == 0.0f && ha.z == 0.0f) return nh_q_ray_sphere(o, d, c, R);
	// (nh_q_sweep_box repeats this test first; it is made here so that a start hit is nh_q_inside(d) itself.  The negated nh_q_inside(-d) has the same
	// bits except for a zero direction, whose 0 / 0 NaN would carry the sign of the platform's default NaN flipped -- host and device would differ)
	if (nh_q_overlap_sphere_box(c, R, o, qa, ha)) return nh_q_inside(d);
	nh_QHit h = nh_q_sweep_box(c, nh_make3(nh_neg(d.x), nh_neg(d.y), nh_neg(d.z)), R, o, qa, ha);
	h.n = nh_make3(nh_neg(h.n.x), nh_neg(h.n.y), nh_neg(h.n.z));
	return h;
}

// The walk's node test of a box cast (k_q_boxcast): nh_q_cast_node with the node box grown by w_k on axis k -- w = e + s, e the cast box's world AABB
// half extents (nh_q_box_extent; 0 for a ray), s = nh_q_cast_pad(o, max_k e_k).  At e = 0 it is the ray's test to the bit.
NH_HD bool nh_q_cast_node3(nh_f3 lo, nh_f3 hi, nh_f3 o, nh_f3 inv, nh_f3 w, float& t0) {
	const float ax = ((lo.x - w.x) - o.x) * inv.x, bx = ((hi.x + w.x) - o.x) * inv.x;
	const float ay = ((lo.y - w.y) - o.y) * inv.y, by = ((hi.y + w.y) - o.y) * inv.y;
	const float az = ((lo.z - w.z) - o.z) * inv.z, bz = ((hi.z + w.z) - o.z) * inv.z;
	t0 = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
	const float t1 = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
	return t0 <= t1 && t1 >= 0.0f;
}

// ---- capsules (nh_overlap's NH_SHAPE_CAPSULE, nh_capsulecast) -------------------------------------------------------------------------------
// A capsule of centre c, rotation q, radius r and half height hh is the set of points within r of the segment c -+ a, a = rotate(q, (0, hh, 0)):
// its axis is the local y axis.  hh = 0 is a ball: every capsule function below then IS the sphere function of the same name, to the bit, and does
// not read q.  The capsule's world AABB is c -+ (|a_k| + r) per axis -- what nh_overlap's walk and the guards below compute.

// The half axis a (0 for hh = 0, where q is not read).
NH_HD nh_f3 nh_q_capsule_axis(nh_quat q, float hh) { return hh == 0.0f ? nh_make3(0.0f, 0.0f, 0.0f) : nh_rotate(q, nh_make3(0.0f, hh, 0.0f)); }

// The capsule's world AABB half extents |a_k| + r.
NH_HD nh_f3 nh_q_capsule_extent(nh_f3 a, float r) { return nh_make3(nh_abs(a.x) + r, nh_abs(a.y) + r, nh_abs(a.z) + r); }

// Do the world AABBs c -+ ea and p -+ eb touch?  (nh_q_overlap_box_box's guard)
NH_HD bool nh_q_aabbs_touch(nh_f3 ca, nh_f3 ea, nh_f3 cb, nh_f3 eb) {
	return (cb.x - eb.x) <= (ca.x + ea.x) && (ca.x - ea.x) <= (cb.x + eb.x) && (cb.y - eb.y) <= (ca.y + ea.y) && (ca.y - ea.y) <= (cb.y + eb.y) &&
	       (cb.z - eb.z) <= (ca.z + ea.z) && (ca.z - ea.z) <= (cb.z + eb.z);
}

// Capsule (c, a, r) against the sphere collider (p, R), a != 0: the two world AABBs touch, and the squared distance from p to the segment is at most
// (r + R)^2 -- the segment's closest point is c + u a with u = (p - c).a / a.a clamped to [-1, 1].  The guard only removes what rounding could put
// outside the AABBs, so that the walk, which prunes by those AABBs padded, never prunes a collider this accepts.
NH_HD bool nh_q_overlap_capsule_sphere_a(nh_f3 c, nh_f3 a, float r, nh_f3 p, float R) {
	if (!nh_q_aabbs_touch(c, nh_q_capsule_extent(a, r), p, nh_make3(R, R, R))) return false;
	const float aa = nh_dot(a, a);
	float u = aa > 0.0f ? nh_dot(p - c, a) / aa : 0.0f;
	u = u < -1.0f ? -1.0f : u > 1.0f ? 1.0f : u;
	const nh_f3 m = (c + u * a) - p;
	const float s = r + R;
	return nh_dot(m, m) <= s * s;
}

// Capsule (c, a, r) against the box collider (p, q, h), a != 0: the two world AABBs touch (as in nh_q_overlap_box_box), and the segment comes within
// r of the box -- the ball of radius r swept from c - a along 2a reaches the box by t = 1 (nh_q_sweep_box, whose start test is the ball at c - a),
// or the ball at c + a touches it (nh_q_overlap_sphere_box).  So both end balls that nh_q_overlap_sphere_box accepts are accepted.
NH_HD bool nh_q_overlap_capsule_box_a(nh_f3 c, nh_f3 a, float r, nh_f3 p, nh_quat q, nh_f3 h) {
	if (!nh_q_aabbs_touch(c, nh_q_capsule_extent(a, r), p, nh_q_box_extent(q, h))) return false;
	if (nh_q_overlap_sphere_box(c + a, r, p, q, h)) return true;
	const nh_QHit s = nh_q_sweep_box(c - a, a + a, r, p, q, h);
	return s.hit && s.t <= 1.0f;
}

// nh_overlap's capsule predicates: hh = 0 is the sphere query's predicate itself (and q is not read).
NH_HD bool nh_q_overlap_capsule_sphere(nh_f3 c, nh_quat q, float r, float hh, nh_f3 p, float R) {
	if (hh == 0.0f) return nh_q_overlap_sphere_sphere(c, r, p, R);
	return nh_q_overlap_capsule_sphere_a(c, nh_q_capsule_axis(q, hh), r, p, R);
}
NH_HD bool nh_q_overlap_capsule_box(nh_f3 c, nh_quat q, float r, float hh, nh_f3 p, nh_quat qb, nh_f3 h) {
	if (hh == 0.0f) return nh_q_overlap_sphere_box(c, r, p, qb, h);
	return nh_q_overlap_capsule_box_a(c, nh_q_capsule_axis(q, hh), r, p, qb, h);
}

// ---- capsule casts (nh_capsulecast): the first t at which the capsule (o + t d, q, r, hh) touches a collider ----------------------------------------
// The capsule translates only.  One that touches at t = 0 under nh_overlap's capsule predicates hits at t = 0 with the ray's inside normal -d / |d|,
// and so does a start contact that only the sweep's rounding finds (a candidate at t = 0).  hh = 0 is nh_spherecast's predicate, bit for bit, and q is
// not read.  The normal is a unit vector from the collider towards the capsule.

// The capsule cast against the sphere collider (p, R): in the capsule's frame (the inverse of q), the ray from p along -d into the capsule of radius
// r + R around the segment from -hh to hh on y -- nh_q_capsule_entry with k = y.  The normal points from p to the segment's closest point at the hit
// (-d / |d| where that distance is 0: r = R = 0).
NH_HD nh_QHit nh_q_sweep_capsule_sphere(nh_f3 o, nh_f3 d, nh_quat q, float r, float hh, nh_f3 p, float R) {
	if (hh == 0.0f) return nh_q_sweep_sphere(o, d, r, p, R);
	if (nh_q_overlap_capsule_sphere_a(o, nh_q_capsule_axis(q, hh), r, p, R)) return nh_q_inside(d);
	nh_QHit res; res.t = 0.0f; res.n = nh_make3(0.0f, 0.0f, 0.0f); res.hit = false;
	const nh_quat qi = { nh_neg(q.x), nh_neg(q.y), nh_neg(q.z), q.s };
	const nh_f3 pl = nh_rotate(qi, p - o), dl = nh_rotate(qi, d);
	const nh_f3 ml = nh_make3(nh_neg(dl.x), nh_neg(dl.y), nh_neg(dl.z));
	const float t = nh_q_capsule_entry(pl.x, pl.z, pl.y, ml.x, ml.z, ml.y, 0.0f, 0.0f, hh, r + R);
	if (!(t < INFINITY)) return res;
	if (!(t > 0.0f)) return nh_q_inside(d);
	const nh_f3 y = pl + t * ml;
	const nh_f3 v = nh_make3(nh_neg(y.x), nh_max(nh_neg(hh), nh_min(y.y, hh)) - y.y, nh_neg(y.z));
	const float vv = nh_dot(v, v);
	if (!(vv > 0.0f)) { const nh_QHit in = nh_q_inside(d); res.n = in.n; }
	else { const float len = sqrtf(vv); res.n = nh_rotate(q, nh_make3(v.x / len, v.y / len, v.z / len)); }
	res.t = t; res.hit = true;
	return res;
}

// The capsule cast against the box collider (p, qb, hb), in the box frame (the inverse of qb): o, d and the half axis a (world, nh_q_capsule_axis)
// become ol, dl, al.  First the ray (ol, dl) against the box grown by the capsule's box-frame AABB half extents |al_k| + r: a capsule that never
// enters it never touches the box, and the candidates below are solved from tb = max(its entry, 0), where the capsule is within its size of the box --
// so a cast from far away loses no accuracy in them.  t is the least of:
//   1. the END BALLS c -+ a, swept by nh_q_sweep_box (the -a end first);
//   2. the VERTICES: each of the 8 box vertices as a ray along -d into the infinite cylinder of radius r about the capsule's axis (closest-approach form,
//      as nh_q_ball_entry), counted where the entry's axial coordinate lies within the segment;
//   3. the EDGES: each of the 12 box edges against the segment.  Their distance along the common normal n = al x e (e the edge's unit axis) is linear
//      in t; the entering root at distance r counts when the closest points of the two lines lie within both segments there.  An edge whose
//      |al x e|^2 is below 2^-20 |al|^2 (within ~1e-3 rad of parallel) is skipped: its direction would be rounding noise.
// FACES need no case of their own: the distance from a face's plane to a point of the segment is linear along it, so a segment not parallel to the
// face reaches it first with an end point (its end ball, kind 1), and a parallel one reaches it with every point at once, end points included.  For
// the same reason a near-parallel edge contact is found by an end ball or a vertex of the edge (kinds 1 and 2).  Ties go to the first candidate in
// the order above (end balls, vertices in (x, y, z) sign order from -, edges by axis x, y, z).
// Normals: an end ball's is nh_q_sweep_box's; a vertex's points from the vertex towards the axis (the direction it approached from when r = 0); an
// edge's is -+n / |n|, signed against d.
NH_HD nh_QHit nh_q_sweep_capsule_box(nh_f3 o, nh_f3 d, nh_quat q, float r, float hh, nh_f3 p, nh_quat qb, nh_f3 hb) {
	if (hh == 0.0f) return nh_q_sweep_box(o, d, r, p, qb, hb);
	const nh_f3 a = nh_q_capsule_axis(q, hh);
	if (nh_q_overlap_capsule_box_a(o, a, r, p, qb, hb)) return nh_q_inside(d);
	nh_QHit res; res.t = 0.0f; res.n = nh_make3(0.0f, 0.0f, 0.0f); res.hit = false;
	const nh_quat qi = { nh_neg(qb.x), nh_neg(qb.y), nh_neg(qb.z), qb.s };
	const nh_f3 ol = nh_rotate(qi, o - p), dl = nh_rotate(qi, d), al = nh_rotate(qi, a);
	float te = -INFINITY, tx = INFINITY;
	int enter = -1;
	bool all = true;
	nh_q_slab(ol.x, dl.x, hb.x + (nh_abs(al.x) + r), 0, te, tx, enter, all);
	nh_q_slab(ol.y, dl.y, hb.y + (nh_abs(al.y) + r), 1, te, tx, enter, all);
	nh_q_slab(ol.z, dl.z, hb.z + (nh_abs(al.z) + r), 2, te, tx, enter, all);
	if (!all || !(te <= tx) || !(tx >= 0.0f)) return res;
	const float tb = te > 0.0f ? te : 0.0f;
	const nh_f3 ob = ol + tb * dl;
	// 1. end balls (world frame)
	float t = INFINITY;
	int kind = 0;                        // 1: an end ball (world normal in n), 2: a vertex, 3: an edge (box-frame normal in n)
	nh_f3 n = nh_make3(0.0f, 0.0f, 0.0f);
	{
		const nh_QHit b0 = nh_q_sweep_box(o - a, d, r, p, qb, hb);
		if (b0.hit) { t = b0.t; n = b0.n; kind = 1; }
		const nh_QHit b1 = nh_q_sweep_box(o + a, d, r, p, qb, hb);
		if (b1.hit && b1.t < t) { t = b1.t; n = b1.n; kind = 1; }
	}
	const float A = nh_dot(al, al);
	const float invA = 1.0f / A;
	// 2. vertices: v - tau dl against the cylinder |perp(v - ob - tau dl)| = r, perp = the part orthogonal to al
	const nh_f3 dp = dl - (nh_dot(dl, al) * invA) * al;
	const float aa = nh_dot(dp, dp);
	if (aa > 0.0f) {
		const float inva = 1.0f / aa, rr = r * r;
		for (int v = 0; v < 8; ++v) {
			const nh_f3 m = nh_make3((v & 1) ? hb.x : nh_neg(hb.x), (v & 2) ? hb.y : nh_neg(hb.y), (v & 4) ? hb.z : nh_neg(hb.z)) - ob;
			const nh_f3 mp = m - (nh_dot(m, al) * invA) * al;
			const float tm = nh_dot(mp, dp) * inva;
			const nh_f3 l = mp - tm * dp;
			const float qq = rr - nh_dot(l, l);
			if (!(qq >= 0.0f)) continue;
			const float dt = sqrtf(qq * inva);
			if (!(tm + dt >= 0.0f)) continue;
			const float ts = tm - dt > 0.0f ? tm - dt : 0.0f;
			const float u = nh_dot(m - ts * dl, al) * invA;
			const float tv = tb + ts;
			if (nh_abs(u) <= 1.0f && tv < t) {
				t = tv; kind = 2;
				n = ts * dp - mp;                                          // (from the vertex to the axis)
				if (!(nh_dot(n, n) > 0.0f)) n = nh_make3(nh_neg(dp.x), nh_neg(dp.y), nh_neg(dp.z));
			}
		}
	}
	// 3. edges along axis k, at (-+h_i, -+h_j) on the other two axes i, j
	for (int k = 0; k < 3; ++k) {
		const float ai = k == 0 ? al.y : k == 1 ? al.z : al.x, aj = k == 0 ? al.z : k == 1 ? al.x : al.y, ak = k == 0 ? al.x : k == 1 ? al.y : al.z;
		const float di = k == 0 ? dl.y : k == 1 ? dl.z : dl.x, dj = k == 0 ? dl.z : k == 1 ? dl.x : dl.y, dk = k == 0 ? dl.x : k == 1 ? dl.y : dl.z;
		const float bi = k == 0 ? ob.y : k == 1 ? ob.z : ob.x, bj = k == 0 ? ob.z : k == 1 ? ob.x : ob.y, bk = k == 0 ? ob.x : k == 1 ? ob.y : ob.z;
		const float hi = k == 0 ? hb.y : k == 1 ? hb.z : hb.x, hj = k == 0 ? hb.z : k == 1 ? hb.x : hb.y, hk = k == 0 ? hb.x : k == 1 ? hb.y : hb.z;
		const float D = ai * ai + aj * aj;                                // |al x e_k|^2; the normal is (-aj, ai) on (i, j)
		if (!(D >= NH_Q_SAT_EPS * A)) continue;
		const float f1 = ai * dj - aj * di;
		if (f1 == 0.0f) continue;
		const float L = sqrtf(D), invD = 1.0f / D, inv1 = 1.0f / nh_abs(f1), rL = r * L;
		const float fb = ai * bj - aj * bi;
		for (int e = 0; e < 4; ++e) {
			const float ci = (e & 1) ? hi : nh_neg(hi), cj = (e & 2) ? hj : nh_neg(hj);
			const float f0 = fb - (ai * cj - aj * ci);
			const float sf = f1 < 0.0f ? f0 : nh_neg(f0);                  // the signed distance on the side the segment comes from
			if (!((sf + rL) * inv1 >= 0.0f)) continue;
			const float te0 = (sf - rL) * inv1;
			const float ts = te0 > 0.0f ? te0 : 0.0f;
			const float wi = (bi + ts * di) - ci, wj = (bj + ts * dj) - cj, wk = bk + ts * dk;
			const float u = nh_neg(ai * wi + aj * wj) * invD;
			const float s = wk + u * ak;
			const float tv = tb + ts;
			if (nh_abs(u) <= 1.0f && nh_abs(s) <= hk && tv < t) {
				t = tv; kind = 3;
				const float ni = (f1 > 0.0f ? aj : nh_neg(aj)) / L, nj = (f1 > 0.0f ? nh_neg(ai) : ai) / L;
				n = nh_make3(k == 0 ? 0.0f : k == 1 ? nj : ni, k == 0 ? ni : k == 1 ? 0.0f : nj, k == 0 ? nj : k == 1 ? ni : 0.0f);
			}
		}
	}
	if (kind == 0) return res;
	if (!(t > 0.0f)) return nh_q_inside(d);
	if (kind == 2) { const float len = sqrtf(nh_dot(n, n)); n = nh_make3(n.x / len, n.y / len, n.z / len); }
	res.t = t; res.n = kind == 1 ? n : nh_rotate(qb, n); res.hit = true;
	return res;
}

// ---- closest points (nh_closest): the signed distance of a point from one collider, and the nearest point of its surface ---------------------------
// Negative inside.  Every function returns the distance d, the unit normal n (outwards from the collider, towards p when p is outside) and the surface
// point x; a collider of a NaN pose gives a NaN distance, which no comparison accepts.
struct nh_QPoint { float d; nh_f3 n; nh_f3 x; };

// The sphere (c, R): m = p - c, L = sqrtf(m.m), d = L - R, n = m / L, x = c + n R.  L = 0 (m.m zero, or below the float range when squared): n = +y.
NH_HD nh_QPoint nh_q_point_sphere(nh_f3 p, nh_f3 c, float R) {
	const nh_f3 m = p - c;
	const float L = sqrtf(nh_dot(m, m));
	nh_QPoint r;
	r.d = L - R;
	r.n = L > 0.0f ? nh_make3(m.x / L, m.y / L, m.z / L) : nh_make3(0.0f, 1.0f, 0.0f);
	r.x = c + r.n * R;
	return r;
}

// The box of world pose (c, q) and half extents h.  l = p in the box frame, by nh_q_overlap_sphere_box's inverse rotation.
//   OUTSIDE (some |l_k| > h_k): ql = clamp(l, -h, h), e = l - ql, d = sqrtf(e.e), n = rotate(q, e / d), x = c + rotate(q, ql).  Where e.e is below the
//           float range (d = 0), n is the region's direction (the signs of e) normalised, as nh_q_sweep_box does for its edge normals.
//   INSIDE or on the surface (every |l_k| <= h_k): the face k of least depth h_k - |l_k| (the lowest axis on equality), d = 0 - depth (+0 on the
//           surface, never -0), n = rotate(q, s e_k), x = c + rotate(q, l with l_k = s h_k), s = -1 where l_k < 0 and +1 otherwise (a zero l_k is +).
NH_HD nh_QPoint nh_q_point_box(nh_f3 p, nh_f3 c, nh_quat q, nh_f3 h) {
	const nh_quat qi = { nh_neg(q.x), nh_neg(q.y), nh_neg(q.z), q.s };
	const nh_f3 l = nh_rotate(qi, p - c);
	nh_QPoint r;
	if (nh_abs(l.x) <= h.x && nh_abs(l.y) <= h.y && nh_abs(l.z) <= h.z) {
		const float dx = h.x - nh_abs(l.x), dy = h.y - nh_abs(l.y), dz = h.z - nh_abs(l.z);
		int k = 0;
		float dep = dx;
		if (dy < dep) { k = 1; dep = dy; }
		if (dz < dep) { k = 2; dep = dz; }
		const float lk = k == 0 ? l.x : k == 1 ? l.y : l.z, hk = k == 0 ? h.x : k == 1 ? h.y : h.z;
		const float s = lk < 0.0f ? -1.0f : 1.0f;
		r.d = 0.0f - dep;
		r.n = nh_rotate(q, nh_make3(k == 0 ? s : 0.0f, k == 1 ? s : 0.0f, k == 2 ? s : 0.0f));
		r.x = c + nh_rotate(q, nh_make3(k == 0 ? s * hk : l.x, k == 1 ? s * hk : l.y, k == 2 ? s * hk : l.z));
		return r;
	}
	const nh_f3 ql = nh_make3(nh_max(nh_neg(h.x), nh_min(l.x, h.x)), nh_max(nh_neg(h.y), nh_min(l.y, h.y)), nh_max(nh_neg(h.z), nh_min(l.z, h.z)));
	nh_f3 e = l - ql;
	const float ee = nh_dot(e, e);
	r.d = sqrtf(ee);
	if (ee == 0.0f) {
		// (a point beyond a face by less than the square root of the smallest float: the signs of e give the region)
		e = nh_make3(e.x > 0.0f ? 1.0f : e.x < 0.0f ? -1.0f : 0.0f, e.y > 0.0f ? 1.0f : e.y < 0.0f ? -1.0f : 0.0f, e.z > 0.0f ? 1.0f : e.z < 0.0f ? -1.0f : 0.0f);
		const float len = sqrtf(nh_dot(e, e));
		r.n = nh_rotate(q, nh_make3(e.x / len, e.y / len, e.z / len));
	} else {
		r.n = nh_rotate(q, nh_make3(e.x / r.d, e.y / r.d, e.z / r.d));
	}
	r.x = c + nh_rotate(q, ql);
	return r;
}

// The squared distance from p to the box [lo, hi] as the walk computes it for a node and the reach rule for a leaf: per axis
// fmaxf(fmaxf(lo - p, p - hi), 0), then the sum of the squares in x, y, z order.  0 when p lies in the box (or the box is NaN: a collider of a body
// that does not exist, whose predicate distance is NaN anyway).
NH_HD float nh_q_point_node(nh_f3 lo, nh_f3 hi, nh_f3 p) {
	const float ax = fmaxf(fmaxf(lo.x - p.x, p.x - hi.x), 0.0f);
	const float ay = fmaxf(fmaxf(lo.y - p.y, p.y - hi.y), 0.0f);
	const float az = fmaxf(fmaxf(lo.z - p.z, p.z - hi.z), 0.0f);
	return ax * ax + ay * ay + az * az;
}

// The reach rule of nh_closest: a collider's key is its predicate distance d where its leaf box contains p (d2 = 0), and
// max(d, sqrtf(d2)) otherwise (a NaN d stays NaN).  Every ancestor box contains the leaf box and every operation of nh_q_point_node is monotone in the
// box, so an ancestor's d2 is never larger than the leaf's: a node with d2 > 0 and sqrtf(d2) > the best key so far holds no collider that could win,
// and a node with d2 = 0 is always entered.
NH_HD float nh_q_point_key(float d, float d2) {
	if (!(d2 > 0.0f)) return d;
	const float s = sqrtf(d2);
	return s > d ? s : d;
}

// Does (d, c) beat the best so far (bd, bc)?  bc = 0xffffffff: none yet.  Counting needs d <= max_d; ties go to the lower combined index c.
NH_HD bool nh_q_closer(float d, uint32_t c, float max_d, float bd, uint32_t bc) {
	if (!(d <= max_d)) return false;
	return bc == 0xffffffffu || d < bd || (d == bd && c < bc);
}

// ---- the k nearest (nh_closest_k): a bounded list of (key, combined index) in nh_q_closer's strict order ---------------------------------------------
// The list lives in storage of the caller's with a stride: slot j at base[j * stride] (the kernel's lists lie slot-major in LDS, stride = the workgroup's
// size; a host array has stride 1).  `held` <= k entries are in use, the nearest first.
struct alignas(8) nh_QNear { float key; uint32_t c; };

// Offer the candidate (key, c).  Refused: a key that is not <= max_d (NaN included); with the list full, a candidate that does not beat the last entry;
// a candidate that is already held -- equal key and equal index: the order is strict, so such an entry sits directly in front of the place the candidate
// would take, and a walk may meet a collider again that a seed has proposed.  Otherwise the entries behind its place move back one slot (the last one
// out, where the list is full) and it goes in.  True when the list changed.
NH_HD bool nh_q_nearest_insert(nh_QNear* base, uint32_t stride, uint32_t k, uint32_t* held, float key, uint32_t c, float max_d) {
	if (!(key <= max_d)) return false;
	const uint32_t m = *held;
	uint32_t at = m;                          // the candidate's place: behind every entry it does not beat
	while (at > 0u) {
		const nh_QNear e = base[(at - 1u) * stride];
		if (!nh_q_closer(key, c, max_d, e.key, e.c)) break;
		--at;
	}
	if (at == k) return false;
	if (at > 0u) {
		const nh_QNear e = base[(at - 1u) * stride];
		if (e.key == key && e.c == c) return false;
	}
	for (uint32_t j = m < k ? m : k - 1u; j > at; --j) base[j * stride] = base[(j - 1u) * stride];
	nh_QNear in; in.key = key; in.c = c;
	base[at * stride] = in;
	if (m < k) *held = m + 1u;
	return true;
}

// ---- penetration (nh_penetration): the least translation that frees a query shape from one collider it overlaps ----------------------------------------
// Every function returns the unit normal n, from the collider towards the query shape, and depth >= +0: the query moved by depth * n touches the
// collider, and no shorter translation in any direction does (a ball adds its radius to the depth of what it inflates; the depth of two
// polytopes lies on a face normal of either or on the cross product of an edge pair).  They are called for pairs nh_overlap's predicates accepted; a
// pair that those accept by rounding alone has a distance at or above the radii here, and its depth is clamped to +0 (never negative, never -0).
struct nh_QPen { nh_f3 n; float depth; };

NH_HD float nh_q_pen_clamp(float depth) { return depth > 0.0f ? depth : 0.0f; }

// Sphere query (c, r) / sphere collider (p, R): nh_q_point_sphere(c, p, R) gives d = |c - p| - R and n = (c - p) / |c - p|; depth = r - d.
// Coincident centres: n = +y (nh_q_point_sphere's).
NH_HD nh_QPen nh_q_pen_sphere_sphere(nh_f3 c, float r, nh_f3 p, float R) {
	const nh_QPoint s = nh_q_point_sphere(c, p, R);
	nh_QPen o; o.n = s.n; o.depth = nh_q_pen_clamp(r - s.d);
	return o;
}

// Sphere query (c, r) / box collider (p, q, h): nh_q_point_box(c, p, q, h) gives the signed distance d of the centre and its normal; depth = r - d, so
// a centre inside the box gives r + the depth of its nearest face (the lowest axis on equality, a zero coordinate on the + side) and n = that face's.
NH_HD nh_QPen nh_q_pen_sphere_box(nh_f3 c, float r, nh_f3 p, nh_quat q, nh_f3 h) {
	const nh_QPoint s = nh_q_point_box(c, p, q, h);
	nh_QPen o; o.n = s.n; o.depth = nh_q_pen_clamp(r - s.d);
	return o;
}

// Box query (ca, qa, ha) / sphere collider (p, R): nh_q_point_box(p, ca, qa, ha), the collider's centre against the QUERY box; depth = R - d and n is
// that normal negated (it points from the query box to the sphere).
NH_HD nh_QPen nh_q_pen_box_sphere(nh_f3 ca, nh_quat qa, nh_f3 ha, nh_f3 p, float R) {
	const nh_QPoint s = nh_q_point_box(p, ca, qa, ha);
	nh_QPen o; o.n = nh_make3(nh_neg(s.n.x), nh_neg(s.n.y), nh_neg(s.n.z)); o.depth = nh_q_pen_clamp(R - s.d);
	return o;
}

// A unit vector perpendicular to a: a x e_k / |a x e_k| for the axis k of a's smallest |a_k| (the lowest on equality); +y where that has no length (a = 0).
NH_HD nh_f3 nh_q_perpendicular(nh_f3 a) {
	const float ax = nh_abs(a.x), ay = nh_abs(a.y), az = nh_abs(a.z);
	nh_f3 v;
	if (ax <= ay && ax <= az) v = nh_make3(0.0f, a.z, nh_neg(a.y));
	else if (ay <= az) v = nh_make3(nh_neg(a.z), 0.0f, a.x);
	else v = nh_make3(a.y, nh_neg(a.x), 0.0f);
	const float vv = nh_dot(v, v);
	if (!(vv > 0.0f)) return nh_make3(0.0f, 1.0f, 0.0f);
	const float len = sqrtf(vv);
	return nh_make3(v.x / len, v.y / len, v.z / len);
}

// The segment-to-point step of a capsule (c, a) against the centre p of a sphere collider: m, from p to the segment's closest point c + u a, with
// nh_q_overlap_capsule_sphere_a's own u.  nh_q_pen_capsule_sphere_a and nh_q_dist_capsule_sphere_a ("distance", below) both start from it.
NH_HD nh_f3 nh_q_segment_point(nh_f3 c, nh_f3 a, nh_f3 p) {
	const float aa = nh_dot(a, a);
	float u = aa > 0.0f ? nh_dot(p - c, a) / aa : 0.0f;
	u = u < -1.0f ? -1.0f : u > 1.0f ? 1.0f : u;
	return (c - p) + u * a;                   // ((c + u a) - p without the rounding of c + u a to the grid of the world coordinates)
}

// Capsule (c, a, r), a != 0 / sphere collider (p, R): the segment's closest point c + u a with nh_q_overlap_capsule_sphere_a's own u, m = (c - p) + u a
// (nh_q_segment_point), depth = (r + R) - |m|, n = m / |m|.  |m| = 0 (the segment passes through p): n = nh_q_perpendicular(a), and the depth r + R is
// that of every direction perpendicular to the axis.
NH_HD nh_QPen nh_q_pen_capsule_sphere_a(nh_f3 c, nh_f3 a, float r, nh_f3 p, float R) {
	const nh_f3 m = nh_q_segment_point(c, a, p);
	const float L = sqrtf(nh_dot(m, m));
	nh_QPen o;
	o.n = L > 0.0f ? nh_make3(m.x / L, m.y / L, m.z / L) : nh_q_perpendicular(a);
	o.depth = nh_q_pen_clamp((r + R) - L);
	return o;
}

// One axis of nh_q_pen_box_box: its overlap rho - |s| (>= 0 for a pair nh_q_overlap_box_box accepted: the same expressions) over the axis' length,
// kept when it is below the least so far -- so the first axis wins on equality.
NH_HD void nh_q_pen_axis(float s, float rho, float len, int axis, float& best, float& sb, int& at) {
	const float o = (rho - nh_abs(s)) / len;
	if (o < best) { best = o; sb = s; at = axis; }
}

// Box query a (ca, qa, ha) / box collider b (cb, qb, hb): the 15 axes of nh_q_overlap_box_box with its very expressions -- a's frame, R = Ra^T Rb,
// t = Ra^T (cb - ca), radii with E = |R| + 2^-20 -- so that every overlap rho_k - |s_k| of an accepted pair is >= 0.  A face axis has unit length; the
// overlap of the edge axis A_i x B_j is divided by its length sqrtf(|A_i x B_j|^2), the squared length read off R (the sum of the squares of column j
// without row i).  An edge pair whose squared length is below NH_Q_SAT_EPS gives neither depth nor normal, as in nh_q_sweep_box_box: both its overlap
// and its direction are rounding noise, and (nearly) parallel edges meet along a face axis anyway.  depth = the least normalised overlap, the first
// axis on equality in the order A_0 .. A_2, B_0 .. B_2, A_0 x B_0, A_0 x B_1 .. A_2 x B_2.  n = that axis in world space, normalised, pointing from
// b to a: against the sign of the projected centre distance s_k, and the + side of the axis where s_k is exactly 0.  The 2^-20 of E only ever adds
// to an overlap: at most 6 * 2^-20 of the sizes on a face axis, the same over the length on an edge axis.
NH_HD nh_QPen nh_q_pen_box_box(nh_f3 ca, nh_quat qa, nh_f3 ha, nh_f3 cb, nh_quat qb, nh_f3 hb) {
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
	float best = INFINITY, sb = 0.0f;
	int at = 0;
	// a's face normals A_0 .. A_2, then b's B_0 .. B_2
	nh_q_pen_axis(t0, a0 + (b0 * E00 + b1 * E01 + b2 * E02), 1.0f, 0, best, sb, at);
	nh_q_pen_axis(t1, a1 + (b0 * E10 + b1 * E11 + b2 * E12), 1.0f, 1, best, sb, at);
	nh_q_pen_axis(t2, a2 + (b0 * E20 + b1 * E21 + b2 * E22), 1.0f, 2, best, sb, at);
	nh_q_pen_axis(t0 * R00 + t1 * R10 + t2 * R20, (a0 * E00 + a1 * E10 + a2 * E20) + b0, 1.0f, 3, best, sb, at);
	nh_q_pen_axis(t0 * R01 + t1 * R11 + t2 * R21, (a0 * E01 + a1 * E11 + a2 * E21) + b1, 1.0f, 4, best, sb, at);
	nh_q_pen_axis(t0 * R02 + t1 * R12 + t2 * R22, (a0 * E02 + a1 * E12 + a2 * E22) + b2, 1.0f, 5, best, sb, at);
	// edge x edge: A_i x B_j
	float D;
	D = R10 * R10 + R20 * R20; if (D >= NH_Q_SAT_EPS) nh_q_pen_axis(t2 * R10 - t1 * R20, (a1 * E20 + a2 * E10) + (b1 * E02 + b2 * E01), sqrtf(D), 6, best, sb, at);
	D = R11 * R11 + R21 * R21; if (D >= NH_Q_SAT_EPS) nh_q_pen_axis(t2 * R11 - t1 * R21, (a1 * E21 + a2 * E11) + (b0 * E02 + b2 * E00), sqrtf(D), 7, best, sb, at);
	D = R12 * R12 + R22 * R22; if (D >= NH_Q_SAT_EPS) nh_q_pen_axis(t2 * R12 - t1 * R22, (a1 * E22 + a2 * E12) + (b0 * E01 + b1 * E00), sqrtf(D), 8, best, sb, at);
	D = R00 * R00 + R20 * R20; if (D >= NH_Q_SAT_EPS) nh_q_pen_axis(t0 * R20 - t2 * R00, (a0 * E20 + a2 * E00) + (b1 * E12 + b2 * E11), sqrtf(D), 9, best, sb, at);
	D = R01 * R01 + R21 * R21; if (D >= NH_Q_SAT_EPS) nh_q_pen_axis(t0 * R21 - t2 * R01, (a0 * E21 + a2 * E01) + (b0 * E12 + b2 * E10), sqrtf(D), 10, best, sb, at);
	D = R02 * R02 + R22 * R22; if (D >= NH_Q_SAT_EPS) nh_q_pen_axis(t0 * R22 - t2 * R02, (a0 * E22 + a2 * E02) + (b0 * E11 + b1 * E10), sqrtf(D), 11, best, sb, at);
	D = R00 * R00 + R10 * R10; if (D >= NH_Q_SAT_EPS) nh_q_pen_axis(t1 * R00 - t0 * R10, (a0 * E10 + a1 * E00) + (b1 * E22 + b2 * E21), sqrtf(D), 12, best, sb, at);
	D = R01 * R01 + R11 * R11; if (D >= NH_Q_SAT_EPS) nh_q_pen_axis(t1 * R01 - t0 * R11, (a0 * E11 + a1 * E01) + (b0 * E22 + b2 * E20), sqrtf(D), 13, best, sb, at);
	D = R02 * R02 + R12 * R12; if (D >= NH_Q_SAT_EPS) nh_q_pen_axis(t1 * R02 - t0 * R12, (a0 * E12 + a1 * E02) + (b0 * E21 + b1 * E20), sqrtf(D), 14, best, sb, at);
	// the axis in world space: A_k, B_k or A_i x B_j (nh_q_sweep_box_box's); s > 0 puts b on its + side, so the normal from b to a is the - side
	nh_f3 L;
	if (at < 3) L = at == 0 ? A.c0 : at == 1 ? A.c1 : A.c2;
	else if (at < 6) L = at == 3 ? B.c0 : at == 4 ? B.c1 : B.c2;
	else {
		const int i = (at - 6) / 3, j = (at - 6) % 3;
		L = nh_cross(i == 0 ? A.c0 : i == 1 ? A.c1 : A.c2, j == 0 ? B.c0 : j == 1 ? B.c1 : B.c2);
	}
	const float len = sqrtf(nh_dot(L, L));
	const nh_f3 n = nh_make3(L.x / len, L.y / len, L.z / len);
	nh_QPen o;
	o.n = sb > 0.0f ? nh_make3(nh_neg(n.x), nh_neg(n.y), nh_neg(n.z)) : n;
	o.depth = nh_q_pen_clamp(best);
	return o;
}

// The closest points of the segment o + u a, u in [-1, 1], and the box edge (ci, cj, v), v in [-hk, hk], all on the axes (i, j, k): the closest points of
// two segments (Ericson, Real-Time Collision Detection 5.1.9) with d1 = a, d2 = e_k, m = o - (ci, cj, 0): u = -(a_i m_i + a_j m_j) / (a_i^2 + a_j^2)
// clamped (0 where the two are exactly parallel), v = m_k + u a_k clamped, then u = (a_k v - a.m) / a.a clamped again where v was clamped.  Returns
// the squared distance; w = the segment's point minus the edge's -- where neither parameter was clamped, the component of m along the lines' common
// normal, which that difference is; ve = v, the edge's point on axis k (the box side's closest point is (ci, cj, ve)).
NH_HD float nh_q_segment_edge(float oi, float oj, float ok, float ai, float aj, float ak, float A, float ci, float cj, float hk, float& wi, float& wj, float& wk, float& ve) {
	const float mi = oi - ci, mj = oj - cj;
	const float D = ai * ai + aj * aj;
	const float cm = ai * mi + aj * mj;
	float u = D > 0.0f ? nh_neg(cm) / D : 0.0f;
	u = u < -1.0f ? -1.0f : u > 1.0f ? 1.0f : u;
	float v = ok + u * ak;
	if (nh_abs(v) > hk) {
		v = v < 0.0f ? nh_neg(hk) : hk;
		u = (ak * v - (cm + ak * ok)) / A;
		u = u < -1.0f ? -1.0f : u > 1.0f ? 1.0f : u;
	} else if (D > 0.0f && nh_abs(u) < 1.0f) {
		// both points inside their segments: w lies along the common normal (aj, -ai, 0) of the two lines, at the distance f / sqrtf(D) along it, read
		// off m without the cancellation of m + u a when the two nearly touch
		const float f = (mi * aj - mj * ai) / D;
		wi = f * aj; wj = nh_neg(f * ai); wk = 0.0f; ve = v;
		return wi * wi + wj * wj;
	}
	wi = mi + u * ai; wj = mj + u * aj; wk = (ok + u * ak) - v; ve = v;
	return wi * wi + wj * wj + wk * wk;
}

// The SHALLOW candidates of a segment ol + u al, u in [-1, 1] (A = al.al), against the box [-hb, hb], all in the box frame -- shared by
// nh_q_pen_capsule_box_a and the distance functions below, which enumerate the same candidates in the same order:
//   1. the two END POINTS against the box (the point minus its clamp to [-h, h]), the -a end first;
//   2. the twelve box EDGES against the segment (nh_q_segment_edge): by axis x, y, z, and on each the corners (-, -), (+, -), (-, +), (+, +) on the other
//      two axes.
// Returns the least squared distance, the first candidate on equality (INFINITY where every candidate is NaN); w = the segment's point minus the box's,
// xb = the box's point.  FACES need no case of their own (nh_q_pen_capsule_box_a says why).  Its two halves stand alone for the box / box distance:
// nh_q_vertex_box offers one point (true where it became the least so far), nh_q_segment_edges the twelve edges.
NH_HD bool nh_q_vertex_box(nh_f3 x, nh_f3 hb, float& dd, nh_f3& w, nh_f3& xb) {
	const nh_f3 ql = nh_make3(nh_max(nh_neg(hb.x), nh_min(x.x, hb.x)), nh_max(nh_neg(hb.y), nh_min(x.y, hb.y)), nh_max(nh_neg(hb.z), nh_min(x.z, hb.z)));
	const nh_f3 v = x - ql;
	const float vv = nh_dot(v, v);
	if (!(vv < dd)) return false;
	dd = vv; w = v; xb = ql;
	return true;
}

NH_HD void nh_q_segment_edges(nh_f3 ol, nh_f3 al, float A, nh_f3 hb, float& dd, nh_f3& w, nh_f3& xb) {
	// the edges along axis k, at (-+h_i, -+h_j) on the other two axes i, j
	for (int k = 0; k < 3; ++k) {
		const float ai = k == 0 ? al.y : k == 1 ? al.z : al.x, aj = k == 0 ? al.z : k == 1 ? al.x : al.y, ak = k == 0 ? al.x : k == 1 ? al.y : al.z;
		const float bi = k == 0 ? ol.y : k == 1 ? ol.z : ol.x, bj = k == 0 ? ol.z : k == 1 ? ol.x : ol.y, bk = k == 0 ? ol.x : k == 1 ? ol.y : ol.z;
		const float hi = k == 0 ? hb.y : k == 1 ? hb.z : hb.x, hj = k == 0 ? hb.z : k == 1 ? hb.x : hb.y, hk = k == 0 ? hb.x : k == 1 ? hb.y : hb.z;
		for (int e = 0; e < 4; ++e) {
			const float ci = (e & 1) ? hi : nh_neg(hi), cj = (e & 2) ? hj : nh_neg(hj);
			float wi, wj, wk, ve;
			const float vv = nh_q_segment_edge(bi, bj, bk, ai, aj, ak, A, ci, cj, hk, wi, wj, wk, ve);
			if (vv < dd) {
				dd = vv;
				w = nh_make3(k == 0 ? wk : k == 1 ? wj : wi, k == 0 ? wi : k == 1 ? wk : wj, k == 0 ? wj : k == 1 ? wi : wk);
				xb = nh_make3(k == 0 ? ve : k == 1 ? cj : ci, k == 0 ? ci : k == 1 ? ve : cj, k == 0 ? cj : k == 1 ? ci : ve);
			}
		}
	}
}

NH_HD float nh_q_segment_box(nh_f3 ol, nh_f3 al, float A, nh_f3 hb, nh_f3& w, nh_f3& xb) {
	w = nh_make3(0.0f, 0.0f, 0.0f); xb = nh_make3(0.0f, 0.0f, 0.0f);
	float dd = INFINITY;
	nh_q_vertex_box(ol - al, hb, dd, w, xb);
	nh_q_vertex_box(ol + al, hb, dd, w, xb);
	nh_q_segment_edges(ol, al, A, hb, dd, w, xb);
	return dd;
}

// Capsule (c, a, r), a != 0 / box collider (p, qb, hb), in the box frame (the inverse of qb, as in nh_q_sweep_capsule_box): the centre and the half
// axis become ol and al, and the segment is ol + u al, u in [-1, 1].
//   SHALLOW  the segment misses the box (its parameter range, clipped against the three slabs by nh_q_slab from [-1, 1], is empty): the distance d > 0
//            between segment and box with its pair of closest points is the least of
//              1. the two END POINTS against the box -- nh_q_point_box's outside branch: the point minus its clamp to [-h, h] -- the -a end first;
//              2. the twelve box EDGES against the segment (nh_q_segment_edge), in nh_q_sweep_capsule_box's order: by axis x, y, z, and on each the
//                 corners (-, -), (+, -), (-, +), (+, +) on the other two axes.
//            The first candidate wins on equality.  depth = r - d clamped at +0, n = (segment point - box point) / d turned to world.
//            FACES need no case of their own, as in nh_q_sweep_capsule_box: the distance from a face's plane to a point of the segment is linear along
//            it, so a segment not parallel to the face is nearest to it with an end point (kind 1); a parallel one is equally near with every point,
//            and then either an end point lies over the face (kind 1) or the segment passes above one of the face's edges (kind 2).
//   DEEP     the segment meets the box (or the candidates above found no distance: d = 0 by rounding).  The Minkowski difference of a box and a segment
//            is a zonotope whose face normals are e_k and al x e_k, so the depth of the segment is the least overlap over those six axes:
//              e_k       (h_k + |al_k|) - |ol_k|;
//              al x e_k  the box's radius on it minus the centre's projection, over its length sqrtf(al_i^2 + al_j^2); skipped where its squared
//                        length is below 2^-20 |al|^2, as the cast skips that edge direction -- the face axes bound the depth there.
//            The first axis wins on equality (e_x, e_y, e_z, al x e_x, al x e_y, al x e_z).  depth = r + the least overlap, clamped at +0, and n = that
//            axis on the side of ol (the + side where ol's projection is exactly 0), turned to world.
NH_HD nh_QPen nh_q_pen_capsule_box_a(nh_f3 c, nh_f3 a, float r, nh_f3 p, nh_quat qb, nh_f3 hb) {
	const nh_quat qi = { nh_neg(qb.x), nh_neg(qb.y), nh_neg(qb.z), qb.s };
	const nh_f3 ol = nh_rotate(qi, c - p), al = nh_rotate(qi, a);
	const float A = nh_dot(al, al);
	nh_QPen o;
	float u0 = -1.0f, u1 = 1.0f;
	int enter = -1;
	bool all = true;
	nh_q_slab(ol.x, al.x, hb.x, 0, u0, u1, enter, all);
	nh_q_slab(ol.y, al.y, hb.y, 1, u0, u1, enter, all);
	nh_q_slab(ol.z, al.z, hb.z, 2, u0, u1, enter, all);
	if (!(all && u0 <= u1)) {
		// SHALLOW: the end points, then the edges (nh_q_segment_box)
		nh_f3 w, xb;
		const float dd = nh_q_segment_box(ol, al, A, hb, w, xb);
		if (dd > 0.0f && dd < INFINITY) {
			const float d = sqrtf(dd);
			o.n = nh_rotate(qb, nh_make3(w.x / d, w.y / d, w.z / d));
			o.depth = nh_q_pen_clamp(r - d);
			return o;
		}
	}
	// DEEP: the box's face normals, then al x e_k
	float best = (hb.x + nh_abs(al.x)) - nh_abs(ol.x), sb = ol.x;
	int at = 0;
	{ const float v = (hb.y + nh_abs(al.y)) - nh_abs(ol.y); if (v < best) { best = v; sb = ol.y; at = 1; } }
	{ const float v = (hb.z + nh_abs(al.z)) - nh_abs(ol.z); if (v < best) { best = v; sb = ol.z; at = 2; } }
	float lb = 1.0f;
	for (int k = 0; k < 3; ++k) {
		const float ai = k == 0 ? al.y : k == 1 ? al.z : al.x, aj = k == 0 ? al.z : k == 1 ? al.x : al.y;
		const float bi = k == 0 ? ol.y : k == 1 ? ol.z : ol.x, bj = k == 0 ? ol.z : k == 1 ? ol.x : ol.y;
		const float hi = k == 0 ? hb.y : k == 1 ? hb.z : hb.x, hj = k == 0 ? hb.z : k == 1 ? hb.x : hb.y;
		const float D = ai * ai + aj * aj;                                // |al x e_k|^2; al x e_k = (aj, -ai) on (i, j)
		if (!(D >= NH_Q_SAT_EPS * A)) continue;
		const float L = sqrtf(D);
		const float s = bi * aj - bj * ai;
		const float v = ((hi * nh_abs(aj) + hj * nh_abs(ai)) - nh_abs(s)) / L;
		if (v < best) { best = v; sb = s; at = 3 + k; lb = L; }
	}
	const float sg = sb < 0.0f ? -1.0f : 1.0f;
	nh_f3 nl;
	if (at < 3) nl = nh_make3(at == 0 ? sg : 0.0f, at == 1 ? sg : 0.0f, at == 2 ? sg : 0.0f);
	else {
		const int k = at - 3;
		const float ai = k == 0 ? al.y : k == 1 ? al.z : al.x, aj = k == 0 ? al.z : k == 1 ? al.x : al.y;
		const float ni = sg * aj / lb, nj = nh_neg(sg * ai) / lb;
		nl = nh_make3(k == 0 ? 0.0f : k == 1 ? nj : ni, k == 0 ? ni : k == 1 ? 0.0f : nj, k == 0 ? nj : k == 1 ? ni : 0.0f);
	}
	o.n = nh_rotate(qb, nl);
	o.depth = nh_q_pen_clamp(r + best);
	return o;
}

// nh_penetration's capsule functions: hh = 0 is the sphere query's function itself (and q is not read).
NH_HD nh_QPen nh_q_pen_capsule_sphere(nh_f3 c, nh_quat q, float r, float hh, nh_f3 p, float R) {
	if (hh == 0.0f) return nh_q_pen_sphere_sphere(c, r, p, R);
	return nh_q_pen_capsule_sphere_a(c, nh_q_capsule_axis(q, hh), r, p, R);
}
NH_HD nh_QPen nh_q_pen_capsule_box(nh_f3 c, nh_quat q, float r, float hh, nh_f3 p, nh_quat qb, nh_f3 hb) {
	if (hh == 0.0f) return nh_q_pen_sphere_box(c, r, p, qb, hb);
	return nh_q_pen_capsule_box_a(c, nh_q_capsule_axis(q, hh), r, p, qb, hb);
}

// ---- distance (nh_distance): how far a query shape is from one collider it does not touch, and towards what ---------------------------------------------
// One function per pair, each a fixed, loop-free-in-the-data enumeration (no iteration to a tolerance: the host's brute force runs the same operations and
// gets the same bits).  Each returns an nh_QPoint: d = the separation, n = the unit normal from the collider towards the query shape, x = the witness on the
// collider's surface (the witness on the query shape is x + d n).  THE OVERLAP RECORD is d = +0, n = x = 0: it is returned when nh_overlap's predicate of
// the pair accepts, when the computed separation is <= 0, and when there is no direction (the closest points coincide).  How deep and which way out is
// nh_penetration's answer.  So n is a unit vector iff d > 0.  A collider of a NaN pose gives d = NaN, which no comparison accepts.
NH_HD nh_QPoint nh_q_dist_overlap() {
	nh_QPoint r; r.d = 0.0f; r.n = nh_make3(0.0f, 0.0f, 0.0f); r.x = nh_make3(0.0f, 0.0f, 0.0f);
	return r;
}
NH_HD nh_QPoint nh_q_dist_apart(float sep, nh_f3 n, nh_f3 x) {
	if (sep <= 0.0f) return nh_q_dist_overlap();          // (a NaN goes on as a NaN)
	nh_QPoint r; r.d = sep; r.n = n; r.x = x;
	return r;
}

// Sphere query (c, r) / sphere collider (p, R) and box collider (p, q, h): nh_q_point_sphere / nh_q_point_box of the centre; separation = d - r, its normal
// and its point.  r = 0 is nh_closest's answer wherever that is positive.
NH_HD nh_QPoint nh_q_dist_sphere_sphere(nh_f3 c, float r, nh_f3 p, float R) {
	if (nh_q_overlap_sphere_sphere(c, r, p, R)) return nh_q_dist_overlap();
	const nh_QPoint s = nh_q_point_sphere(c, p, R);
	return nh_q_dist_apart(s.d - r, s.n, s.x);
}
NH_HD nh_QPoint nh_q_dist_sphere_box(nh_f3 c, float r, nh_f3 p, nh_quat q, nh_f3 h) {
	if (nh_q_overlap_sphere_box(c, r, p, q, h)) return nh_q_dist_overlap();
	const nh_QPoint s = nh_q_point_box(c, p, q, h);
	return nh_q_dist_apart(s.d - r, s.n, s.x);
}

// Box query (ca, qa, ha) / sphere collider (p, R): nh_q_point_box of p against the QUERY box; separation = d - R, the normal is that normal negated (it
// points from the query box to the sphere), the point p + R n.
NH_HD nh_QPoint nh_q_dist_box_sphere(nh_f3 ca, nh_quat qa, nh_f3 ha, nh_f3 p, float R) {
	if (nh_q_overlap_sphere_box(p, R, ca, qa, ha)) return nh_q_dist_overlap();
	const nh_QPoint s = nh_q_point_box(p, ca, qa, ha);
	const nh_f3 n = nh_make3(nh_neg(s.n.x), nh_neg(s.n.y), nh_neg(s.n.z));
	return nh_q_dist_apart(s.d - R, n, p + n * R);
}

// Capsule (c, a, r), a != 0 / sphere collider (p, R): m from p to the segment's closest point (nh_q_segment_point, nh_q_pen_capsule_sphere_a's);
// separation = (|m| - R) - r, n = m / |m|, point = p + R n.  |m| = 0 has a separation <= 0: the overlap record.
NH_HD nh_QPoint nh_q_dist_capsule_sphere_a(nh_f3 c, nh_f3 a, float r, nh_f3 p, float R) {
	if (nh_q_overlap_capsule_sphere_a(c, a, r, p, R)) return nh_q_dist_overlap();
	const nh_f3 m = nh_q_segment_point(c, a, p);
	const float L = sqrtf(nh_dot(m, m));
	const nh_f3 n = nh_make3(m.x / L, m.y / L, m.z / L);
	return nh_q_dist_apart((L - R) - r, n, p + n * R);
}

// Capsule (c, a, r), a != 0 / box collider (p, qb, hb): the least of nh_q_pen_capsule_box_a's SHALLOW candidates (nh_q_segment_box: the end points, the -a
// end first, then the twelve edges; the first on equality) in the box frame; separation = d - r, n = w / d turned to world, point = the box side's closest
// point in world.  (A segment that passes through the box has candidates of its own, all wrong; nh_overlap's predicate, asked first, accepts it.)
NH_HD nh_QPoint nh_q_dist_capsule_box_a(nh_f3 c, nh_f3 a, float r, nh_f3 p, nh_quat qb, nh_f3 hb) {
	if (nh_q_overlap_capsule_box_a(c, a, r, p, qb, hb)) return nh_q_dist_overlap();
	const nh_quat qi = { nh_neg(qb.x), nh_neg(qb.y), nh_neg(qb.z), qb.s };
	const nh_f3 ol = nh_rotate(qi, c - p), al = nh_rotate(qi, a);
	nh_f3 w, xb;
	const float dd = nh_q_segment_box(ol, al, nh_dot(al, al), hb, w, xb);
	if (!(dd < INFINITY)) return nh_q_dist_apart(nh_asfloat(0x7fc00000u), w, xb);          // (every candidate NaN: a NaN pose)
	if (!(dd > 0.0f)) return nh_q_dist_overlap();
	const float d = sqrtf(dd);
	return nh_q_dist_apart(d - r, nh_rotate(qb, nh_make3(w.x / d, w.y / d, w.z / d)), p + nh_rotate(qb, xb));
}

// Box query a (ca, qa, ha) / box collider b (cb, qb, hb): the least squared distance over a fixed list of candidates, the first on equality:
//   1. the 8 vertices of a, in b's frame, against b -- the vertex minus its clamp to [-hb, hb] (nh_q_vertex_box).  In b's frame a's centre is
//      o = Rb^T (ca - cb) and its scaled axes a_k = Rb^T (A_k ha_k); vertex v (0 .. 7) is ((o + s0 a_0) + s1 a_1) + s2 a_2 with s_k = +1 where bit k of v
//      is set and -1 otherwise;
//   2. the 8 vertices of b, in a's frame, against a, numbered the same way;
//   3. the 144 edge pairs: each of a's 12 edges as a segment in b's frame -- by axis i = x, y, z, and on each the corners (-, -), (+, -), (-, +), (+, +)
//      on the axes (i + 1) % 3, (i + 2) % 3: centre (o + s1 a_j) + s2 a_k, half axis a_i -- against b's 12 edges in nh_q_segment_edges' order.  An edge of
//      a box with ha_i = 0 is its vertex (group 1) and is skipped.
// This is exact: the closest features of two disjoint convex polytopes always contain a vertex / face or an edge / edge pair at the same distance (a face
// against a face or an edge is nearest at a vertex or at a crossing of edges, as "FACES need no case of their own" argues for the capsule), a vertex
// against the whole box covers vertex / anything, and a segment against an edge covers edge / edge with the clamps at the ends.
// separation = sqrtf of that least, n = (a's point - b's point) / separation and point = b's point, turned to world from the frame the candidate was
// found in.  A box with a zero half extent is valid on either side.
NH_HD nh_QPoint nh_q_dist_box_box(nh_f3 ca, nh_quat qa, nh_f3 ha, nh_f3 cb, nh_quat qb, nh_f3 hb) {
	if (nh_q_overlap_box_box(ca, qa, ha, cb, qb, hb)) return nh_q_dist_overlap();
	const nh_quat qai = { nh_neg(qa.x), nh_neg(qa.y), nh_neg(qa.z), qa.s }, qbi = { nh_neg(qb.x), nh_neg(qb.y), nh_neg(qb.z), qb.s };
	const nh_m33 A = nh_matrix(qa), B = nh_matrix(qb);
	float dd = INFINITY;
	nh_f3 w = nh_make3(0.0f, 0.0f, 0.0f), xb = nh_make3(0.0f, 0.0f, 0.0f);          // a's point minus b's, and b's point, in the frame `in_a` says
	bool in_a = false;
	const nh_f3 o = nh_rotate(qbi, ca - cb);
	const nh_f3 a0 = nh_rotate(qbi, A.c0 * ha.x), a1 = nh_rotate(qbi, A.c1 * ha.y), a2 = nh_rotate(qbi, A.c2 * ha.z);
	// 1. a's vertices against b
	for (int v = 0; v < 8; ++v) {
		const float s0 = (v & 1) ? 1.0f : -1.0f, s1 = (v & 2) ? 1.0f : -1.0f, s2 = (v & 4) ? 1.0f : -1.0f;
		nh_q_vertex_box(((o + s0 * a0) + s1 * a1) + s2 * a2, hb, dd, w, xb);
	}
	// 2. b's vertices against a: the candidate's vector points from a's point to the vertex, so w is its negative and b's point is the vertex itself
	{
		const nh_f3 m = nh_rotate(qai, cb - ca);
		const nh_f3 b0 = nh_rotate(qai, B.c0 * hb.x), b1 = nh_rotate(qai, B.c1 * hb.y), b2 = nh_rotate(qai, B.c2 * hb.z);
		for (int v = 0; v < 8; ++v) {
			const float s0 = (v & 1) ? 1.0f : -1.0f, s1 = (v & 2) ? 1.0f : -1.0f, s2 = (v & 4) ? 1.0f : -1.0f;
			const nh_f3 x = ((m + s0 * b0) + s1 * b1) + s2 * b2;
			nh_f3 e, ql;
			if (nh_q_vertex_box(x, ha, dd, e, ql)) { w = nh_make3(nh_neg(e.x), nh_neg(e.y), nh_neg(e.z)); xb = x; in_a = true; }
		}
	}
	// 3. a's edges against b's edges
	for (int i = 0; i < 3; ++i) {
		const nh_f3 al = i == 0 ? a0 : i == 1 ? a1 : a2, aj = i == 0 ? a1 : i == 1 ? a2 : a0, ak = i == 0 ? a2 : i == 1 ? a0 : a1;
		const float AA = nh_dot(al, al);
		if (!(AA > 0.0f)) continue;
		for (int e = 0; e < 4; ++e) {
			const float s1 = (e & 1) ? 1.0f : -1.0f, s2 = (e & 2) ? 1.0f : -1.0f;
			const float before = dd;
			nh_q_segment_edges((o + s1 * aj) + s2 * ak, al, AA, hb, dd, w, xb);
			if (dd < before) in_a = false;
		}
	}
	if (!(dd < INFINITY)) return nh_q_dist_apart(nh_asfloat(0x7fc00000u), w, xb);          // (every candidate NaN: a NaN pose)
	if (!(dd > 0.0f)) return nh_q_dist_overlap();
	const float d = sqrtf(dd);
	const nh_quat qf = in_a ? qa : qb;
	const nh_f3 cf = in_a ? ca : cb;
	return nh_q_dist_apart(d, nh_rotate(qf, nh_make3(w.x / d, w.y / d, w.z / d)), cf + nh_rotate(qf, xb));
}

// nh_distance's capsule functions: hh = 0 is the sphere query's function itself (and q is not read).
NH_HD nh_QPoint nh_q_dist_capsule_sphere(nh_f3 c, nh_quat q, float r, float hh, nh_f3 p, float R) {
	if (hh == 0.0f) return nh_q_dist_sphere_sphere(c, r, p, R);
	return nh_q_dist_capsule_sphere_a(c, nh_q_capsule_axis(q, hh), r, p, R);
}
NH_HD nh_QPoint nh_q_dist_capsule_box(nh_f3 c, nh_quat q, float r, float hh, nh_f3 p, nh_quat qb, nh_f3 hb) {
	if (hh == 0.0f) return nh_q_dist_sphere_box(c, r, p, qb, hb);
	return nh_q_dist_capsule_box_a(c, nh_q_capsule_axis(q, hh), r, p, qb, hb);
}

// The squared gap between the query's world AABB [qlo, qhi] (centre -+ r, nh_q_box_extent or nh_q_capsule_extent; not padded) and the box [lo, hi] of a
// node or a leaf: nh_q_point_node's operations with an interval in place of the point -- per axis fmaxf(fmaxf(lo - qhi, qlo - hi), 0), then the sum of the
// squares in x, y, z order.  Monotone in the box: a box inside another never has the smaller gap.  With qlo = qhi = p it IS nh_q_point_node(lo, hi, p).
NH_HD float nh_q_dist_node(nh_f3 lo, nh_f3 hi, nh_f3 qlo, nh_f3 qhi) {
	const float ax = fmaxf(fmaxf(lo.x - qhi.x, qlo.x - hi.x), 0.0f);
	const float ay = fmaxf(fmaxf(lo.y - qhi.y, qlo.y - hi.y), 0.0f);
	const float az = fmaxf(fmaxf(lo.z - qhi.z, qlo.z - hi.z), 0.0f);
	return ax * ax + ay * ay + az * az;
}
// The key of a pair under the reach rule: nh_q_point_key(d, g2) with d the pair function's separation (>= +0, or NaN) and g2 =
// nh_q_dist_node of the collider's OWN leaf box (nh_q_leaf_box) -- max(d, sqrtf(g2)).  A function of the pair alone, so the answer does not depend on the
// walk.  It is the `distance` that is written, for an overlap record as well: where nh_overlap's predicate accepts a pair whose boxes rounding has put
// apart (g2 > 0; it cannot happen for box / box and the capsule pairs, whose predicates ask that the unpadded boxes touch, and float subtraction is
// monotone), the overlap record carries that tiny positive distance with its zero normal -- the normal, not the distance, says which kind a record is.

// ---- all-hits casts (nh_raycast_all / nh_spherecast_all / nh_boxcast_all / nh_capsulecast_all): the hit of ONE collider, as the closest-hit walk decides it at a leaf with no best so far --
// The ray's own predicates (SWEEP = false) or the swept ball's with the reach rule for r > 0 (SWEEP = true; t0 = the entry into the collider's leaf box
// under nh_q_cast_node, w = r + nh_q_cast_pad), then 0 <= t <= max_t (nh_q_better against nothing).  The count walk, the list walk and the gather call
// this one function on the same inputs, so all three get the same bits; the host's brute force calls it too.
template <bool SWEEP>
NH_HD nh_QHit nh_q_all_hit(nh_f3 o, nh_f3 d, float r, float max_t, float t0, nh_f3 p, nh_quat q, nh_f3 h, bool box) {
	nh_QHit s;
	if (SWEEP) {
		s = box ? nh_q_sweep_box(o, d, r, p, q, h) : nh_q_sweep_sphere(o, d, r, p, h.x);
		if (r > 0.0f && t0 > s.t) s.t = t0;
	} else {
		s = box ? nh_q_ray_box(o, d, p, q, h) : nh_q_ray_sphere(o, d, p, h.x);
	}
	s.hit = s.hit && nh_q_better(s.t, 0u, max_t, max_t, 0xffffffffu);
	return s;
}

// The entry of a cast into a collider's own leaf box (nh_q_leaf_box: the box the build stores), for the caller that has no walk to take it from: the
// gather and the host.  false: the leaf is not entered, and under the reach rule (r > 0) the collider is not hit.
NH_HD bool nh_q_leaf_entry(nh_f3 o, nh_f3 inv, float w, nh_f3 p, nh_quat q, nh_f3 h, bool box, float& t0) {
	nh_f3 lo, hi;
	nh_q_leaf_box(p, q, h, box, lo, hi);
	return nh_q_cast_node(lo, hi, o, inv, w, t0);
}

// nh_boxcast_all / nh_capsulecast_all: the same decision for the cast box (qa, ha) and the capsule (qa, r, hh) -- nh_QBox::leaf / nh_QCapsule::leaf
// (nh_query.hip) at a leaf with no best hit so far, then 0 <= t <= max_t.  t0 = the entry into the collider's leaf box under nh_q_cast_node3 with the cast's
// per-axis grow (nh_q_leaf_entry3 rebuilds it); it is read exactly where the closest-hit leaf reads it: for a box of nonzero size, and for a capsule
// unless r = hh = 0.  A size-0 box is nh_q_all_hit<false> and a capsule of hh = 0 nh_q_all_hit<true>, bit for bit, through the predicates' own first
// lines.  The count walk, the list walk, the gather and the host's brute force call these on the same inputs.
NH_HD nh_QHit nh_q_all_hit_box(nh_f3 o, nh_f3 d, nh_quat qa, nh_f3 ha, float max_t, float t0, nh_f3 p, nh_quat q, nh_f3 h, bool box) {
	nh_QHit s = box ? nh_q_sweep_box_box(o, d, qa, ha, p, q, h) : nh_q_sweep_box_sphere(o, d, qa, ha, p, h.x);
	const bool ray = ha.x == 0.0f && ha.y == 0.0f && ha.z == 0.0f;
	if (!ray && t0 > s.t) s.t = t0;
	s.hit = s.hit && nh_q_better(s.t, 0u, max_t, max_t, 0xffffffffu);
	return s;
}

NH_HD nh_QHit nh_q_all_hit_capsule(nh_f3 o, nh_f3 d, nh_quat qa, float r, float hh, float max_t, float t0, nh_f3 p, nh_quat q, nh_f3 h, bool box) {
	nh_QHit s = box ? nh_q_sweep_capsule_box(o, d, qa, r, hh, p, q, h) : nh_q_sweep_capsule_sphere(o, d, qa, r, hh, p, h.x);
	if ((r > 0.0f || hh > 0.0f) && t0 > s.t) s.t = t0;
	s.hit = s.hit && nh_q_better(s.t, 0u, max_t, max_t, 0xffffffffu);
	return s;
}

// nh_q_leaf_entry under the per-axis grow w of a box or capsule cast (nh_q_cast_node3).  With the same w on every axis it is nh_q_leaf_entry to the bit.
NH_HD bool nh_q_leaf_entry3(nh_f3 o, nh_f3 inv, nh_f3 w, nh_f3 p, nh_quat q, nh_f3 h, bool box, float& t0) {
	nh_f3 lo, hi;
	nh_q_leaf_box(p, q, h, box, lo, hi);
	return nh_q_cast_node3(lo, hi, o, inv, w, t0);
}

// The all-hits walk's node pad for a RAY (r = 0).  The closest-hit ray walk prunes with boxes padded by 2^-18 of the coordinates, which does not bound the
// rounding of the ray predicates: nh_q_ray_sphere accepts where the computed b*b - a*(m.m - R*R) >= 0, and with |m| = |o - c| the roundings of that
// expression sum to under 32 * 2^-24 * |m|^2 |d|^2 (three rounded products and sums per dot product, the squares, the product with a and the
// differences), so an accepted ray may pass the centre at up to sqrt(R^2 + 2^-19 |m|^2) <= R + 2^-9.5 |m|, and the reported point o + t d lies within that
// distance of the centre as well (its offset along the ray from the closest approach is sqrt(disc) / |d|).  nh_q_ray_box rounds linearly in |m| (a few
// 2^-24 of |m| + |h| in the box frame), far below that.  A closest-hit call loses such a far grazing hit only where it is the closest; the all-hits set
// is every collider the predicate accepts, so its walk grows each node box by 2^-9 of L, an upper bound (the 1-norm) of the distance from the origin to
// the farthest point of the box: L >= |m| for every collider whose leaf box lies inside, L and the grown box are monotone in the box, so no ancestor
// prunes what a leaf would accept.  (Casts of a shape with a size -- r > 0, a box of nonzero size, a capsule unless r = hh = 0 -- need none of this: the reach rule makes their set a
// function of the leaf test.  A box of size 0 and a capsule of r = hh = 0 are rays and take the pad.)
NH_HD float nh_q_all_pad(nh_f3 lo, nh_f3 hi, nh_f3 o) {
	const float fx = fmaxf(fabsf(lo.x - o.x), fabsf(hi.x - o.x)), fy = fmaxf(fabsf(lo.y - o.y), fabsf(hi.y - o.y)), fz = fmaxf(fabsf(lo.z - o.z), fabsf(hi.z - o.z));
	return ((fx + fy) + fz) * 0.001953125f;
}

// The sort key of a hit's t: the bits of t + 0.0f.  t >= 0, so -0 becomes +0 and the bits order as the floats do.
NH_HD uint32_t nh_q_tbits(float t) { return nh_asuint(t + 0.0f); }

// ---- move (nh_move, nh_boxmove): collide-and-slide of a swept capsule or box, the state between two casts -----------------------------------------------------
// These functions ARE the definition of nh_move (include/nudge_hip.h): k_q_move and the host's brute force (tests/hostoracle/hostmover.cpp) both run
//     s = nh_q_move_begin(origin, displacement);
//     while (nh_q_move_go(s)) { hit = the closest-hit capsule cast { s.p, 1.0f, s.v, ignore_body, rotation, radius, half_height };
//                               if (!nh_q_move_advance(s, hit found, hit.t, hit.normal, skin, max_slides)) break; }
// and write s.p, s.flags, s.v, s.slides and the last cast's record.  nh_boxmove (the same file) is the same loop around the closest-hit box cast
// { s.p, 1.0f, s.v, ignore_body, rotation, size }: nothing below sees the shape.  Every product is rounded before the sum it goes into (no fused multiply-add), and every
// dot and cross product is nh_dot / nh_cross of nh_math.h: (x*x + y*y) + z*z, left to right.
// The flag bits are nh_MoveResult.flags' (nh_query.hip asserts that they are the header's NH_MOVE_*).
#define NH_Q_MOVE_HIT 1u
#define NH_Q_MOVE_START_OVERLAP 2u
#define NH_Q_MOVE_SLIDES_OUT 4u
#define NH_Q_MOVE_WEDGED 8u
#define NH_Q_MOVE_MAX_SLIDES 8u
#define NH_Q_MOVE_CREASE_EPS 5.9604644775390625e-08f          // 2^-24: |n_prev x n|^2 below it, the two normals are one plane and there is no crease line
#define NH_Q_MOVE_TINY 9.094947017729282e-13f                  // 2^-40: what is left counts as nothing below this share of |displacement|^2

// p: where the capsule's centre is; v: what is left of the displacement; d0: the displacement asked for; np: the normal of the last hit taken, read only
// where slides > 0 (slides counts exactly the hits taken, so "there is an n_prev" is slides > 0 before the count goes up).
struct nh_QMove { nh_f3 p, v, d0, np; uint32_t slides, flags; };

NH_HD bool nh_q_move_finite(float x) { return (nh_asuint(x) & 0x7f800000u) != 0x7f800000u; }

// The record's validity (header, "Invalid records"); `rotation` is read only where hh > 0
NH_HD bool nh_q_move_valid(nh_f3 o, nh_f3 d, nh_quat q, float r, float hh, float skin, uint32_t max_slides) {
	bool ok = nh_q_move_finite(o.x) && nh_q_move_finite(o.y) && nh_q_move_finite(o.z) && nh_q_move_finite(d.x) && nh_q_move_finite(d.y) && nh_q_move_finite(d.z);
	ok = ok && nh_q_move_finite(r) && nh_q_move_finite(hh) && nh_q_move_finite(skin) && !(r < 0.0f) && !(hh < 0.0f) && !(skin < 0.0f);
	ok = ok && (hh == 0.0f || (nh_q_move_finite(q.x) && nh_q_move_finite(q.y) && nh_q_move_finite(q.z) && nh_q_move_finite(q.s)));
	return ok && max_slides <= NH_Q_MOVE_MAX_SLIDES;
}

// nh_boxmove's record (header, "Invalid records"): the half extents h in place of r and hh; `rotation` is read only where h is not (0, 0, 0)
NH_HD bool nh_q_boxmove_valid(nh_f3 o, nh_f3 d, nh_quat q, nh_f3 h, float skin, uint32_t max_slides) {
	bool ok = nh_q_move_finite(o.x) && nh_q_move_finite(o.y) && nh_q_move_finite(o.z) && nh_q_move_finite(d.x) && nh_q_move_finite(d.y) && nh_q_move_finite(d.z);
	ok = ok && nh_q_move_finite(h.x) && nh_q_move_finite(h.y) && nh_q_move_finite(h.z) && nh_q_move_finite(skin);
	ok = ok && !(h.x < 0.0f) && !(h.y < 0.0f) && !(h.z < 0.0f) && !(skin < 0.0f);
	ok = ok && ((h.x == 0.0f && h.y == 0.0f && h.z == 0.0f) || (nh_q_move_finite(q.x) && nh_q_move_finite(q.y) && nh_q_move_finite(q.z) && nh_q_move_finite(q.s)));
	return ok && max_slides <= NH_Q_MOVE_MAX_SLIDES;
}

NH_HD nh_QMove nh_q_move_begin(nh_f3 origin, nh_f3 displacement) {
	nh_QMove s;
	s.p = origin; s.v = displacement; s.d0 = displacement; s.np = nh_make3(0.0f, 0.0f, 0.0f);
	s.slides = 0u; s.flags = 0u;
	return s;
}

// Rule 1: is there anything left to cast along?  (A v whose square underflows to 0 is nothing; a NaN v -- only an overflow of finite inputs makes one -- goes
// on to a cast that is invalid, hence a miss, hence the end.)
NH_HD bool nh_q_move_go(const nh_QMove& s) { return nh_dot(s.v, s.v) != 0.0f; }

// Rules 3 - 7 behind one cast from s.p along s.v with max_t = 1: `hit` says whether it found a collider, (t, n) are its record's t and normal.  Returns
// whether the move goes on (to rule 1).  Order of operations, per component k where a vector is written:
//   miss        p_k = p_k + v_k; v = +0
//   t == 0      nothing but the flag: p and v keep their bits
//   t > 0       p_k = p_k + (t * v_k), then p_k = p_k + (skin * n_k); u = 1 - t; rem_k = u * v_k
//   deflect     s = rem.n; w = s < 0 ? rem - s*n (w_k = rem_k - (s * n_k)) : rem
//   crease      only where a hit was taken before and w.np < 0: c = np x n, cc = c.c; cc < 2^-24: w = 0; else g = (rem.c) / cc, w_k = c_k * g;
//               then w = 0 if w.np < 0 or w.n < 0
//   never back  w = 0 unless w.d0 > 0          ("unless": a NaN is zeroed too)
//   tiny        w = 0 unless w.w > 2^-40 * (d0.d0)
//   WEDGED      iff one of the four rules above wrote w = 0 and rem has a component that is not (+-)0.  A head-on hit needs no special case: w = rem - s*n is
//               then 0 or rounding dust, w.d0 is not > 0, "never back" fires and the flag is set.  rem = 0 (t = 1: touching exactly at the end) sets none.
//   v = w, np = n; slides > max_slides with v.v > 0: SLIDES_OUT and stop.  With v.v == 0 the move goes on to rule 1, which ends it.
// nh_q_move_advance2 is the one body: `n` is the PUSH normal (the skin push of rule 5), `ns` the SLIDE normal (the deflection, the crease and n_prev of rule
// 6).  nh_move slides along what it hit, ns = n; nh_walk's climb rule ("walk", below) deflects along the horizontal part of a face too steep to stand on.
NH_HD bool nh_q_move_advance2(nh_QMove& s, bool hit, float t, nh_f3 n, nh_f3 ns, float skin, uint32_t max_slides) {
	if (!hit) {
		s.p = s.p + s.v;
		s.v = nh_make3(0.0f, 0.0f, 0.0f);
		return false;
	}
	if (t == 0.0f) { s.flags |= NH_Q_MOVE_START_OVERLAP; return false; }
	const bool prev = s.slides != 0u;
	s.flags |= NH_Q_MOVE_HIT;
	s.slides += 1u;
	s.p = s.p + t * s.v;
	s.p = s.p + skin * n;
	const nh_f3 rem = (1.0f - t) * s.v;
	const float sn = nh_dot(rem, ns);
	nh_f3 w = sn < 0.0f ? rem - sn * ns : rem;
	const nh_f3 zero = nh_make3(0.0f, 0.0f, 0.0f);
	bool zeroed = false;
	if (prev && nh_dot(w, s.np) < 0.0f) {
		const nh_f3 c = nh_cross(s.np, ns);
		const float cc = nh_dot(c, c);
		if (cc < NH_Q_MOVE_CREASE_EPS) { w = zero; zeroed = true; }
		else w = c * (nh_dot(rem, c) / cc);
		if (nh_dot(w, s.np) < 0.0f || nh_dot(w, ns) < 0.0f) { w = zero; zeroed = true; }
	}
	if (!(nh_dot(w, s.d0) > 0.0f)) { w = zero; zeroed = true; }
	if (!(nh_dot(w, w) > NH_Q_MOVE_TINY * nh_dot(s.d0, s.d0))) { w = zero; zeroed = true; }
	if (zeroed && (rem.x != 0.0f || rem.y != 0.0f || rem.z != 0.0f)) s.flags |= NH_Q_MOVE_WEDGED;
	s.v = w; s.np = ns;
	if (s.slides > max_slides && nh_dot(w, w) > 0.0f) { s.flags |= NH_Q_MOVE_SLIDES_OUT; return false; }
	return true;
}

NH_HD bool nh_q_move_advance(nh_QMove& s, bool hit, float t, nh_f3 n, float skin, uint32_t max_slides) { return nh_q_move_advance2(s, hit, t, n, n, skin, max_slides); }

// ---- walk (nh_walk): a grounded character step, the state between two capsule casts ---------------------------------------------------------------------
// These functions ARE the definition of nh_walk (include/nudge_hip.h): k_q_walk and the host's brute force (tests/hostoracle/hostmover.cpp) both run
//     s = nh_q_walk_begin(W);
//     while (nh_q_walk_cast(s, W)) { hit = the closest-hit capsule cast { s.m.p, 1.0f, s.m.v, ignore_body, rotation, radius, half_height };
//                                    nh_q_walk_advance(s, W, hit found, hit.t, hit's collider, hit.normal, the cast was valid); }
// and write s.kp, s.kflags, s.kv, s.kslides, the records of s.klast and nh_q_walk_ground(s), s.step_up, nh_q_walk_drop(s, W) and s.casts.  (nh_boxwalk,
// the same file: the same with the closest-hit box cast { s.m.p, 1.0f, s.m.v, ignore_body, rotation, size }.)  A walk is up to five MOVE LOOPS ("move",
// above: nh_q_move_begin / _go / _advance2 on s.m), one after the other, and the decisions between them; a lane is in one PHASE:
//   A  slide    from origin along displacement, max_slides, under the climb rule.  Its end is KEPT (kp, kv, kslides, kflags, klast).  A taken hit (t > 0) whose
//               normal is steep sets `blocked` (the phase AB).  START_OVERLAP: the walk ends here.  step_height > 0 and blocked: U.  Otherwise C.
//   U  up       from origin along step_height * up (per component), 0 slides.  lift = (p - origin).up.  START_OVERLAP or !(lift > 0): C.  Otherwise F.
//   F  forward  from U's end along displacement, max_slides, under the climb rule.  START_OVERLAP: C.  Otherwise its (v, slides, flags, last) wait in f*, and D.
//   D  down     from F's end along (-lift) * up, 0 slides.  ACCEPT iff its cast hit at t > 0 (NH_Q_MOVE_HIT), the normal is walkable and
//               (p - origin).dh > (kp - origin).dh with dh_k = displacement_k - ((displacement.up) * up_k): then step_up = (p - kp).up, kp = p, (kv, kslides,
//               kflags, klast) = F's, kflags |= STEPPED | GROUNDED, ground = D's cast, and the walk ends.  Otherwise C: A stands.
//   C  probe    only where snap_distance > 0: ONE cast (no move loop, no v.v test) from kp along (-snap_distance) * up.  ground = its record, hit or miss.
//               A steep hit: ON_STEEP.  A walkable hit: GROUNDED, and unless PROBE_ONLY or t == 0: kp = kp + t*v, kp = kp + skin*n (move's rule 5),
//               drop = t * snap_distance, SNAPPED.  (A t == 0 hit has the normal -v / |v| = up: grounded where it stands.)
// A move loop that has nothing to cast along (v.v == 0: a zero displacement, a lift whose square underflows) ends without a cast; nh_q_walk_cast settles such
// loops, at most four in a row, before it answers.  WALKABLE(n): u = n.up, u > 0 and u >= min_ground_up; anything else is STEEP.
// CLIMB RULE, in A and F, off where min_ground_up == 0: at a taken hit that is steep with u >= 0 whose plain deflection w (rem_k = (1 - t) * v_k, s = rem.n,
// w = s < 0 ? rem - s*n : rem -- move's bits) has w.up > 0: the loop's flags |= STEEP, and the slide normal is ns_k = h_k / sqrtf(h.h) with
// h_k = n_k - (u * up_k), unless h.h < 2^-24 (ns = n).  The push stays along n.  STEEP is a flag of its loop: the result carries the kept loop's.
// `casts` counts every cast; A and F make at most max_slides + 1 each, U, D and C one each: 2 * (8 + 1) + 3 = 21.
#define NH_Q_WALK_STEPPED 0x10u
#define NH_Q_WALK_GROUNDED 0x20u
#define NH_Q_WALK_SNAPPED 0x40u
#define NH_Q_WALK_STEEP 0x80u
#define NH_Q_WALK_ON_STEEP 0x100u
#define NH_Q_WALK_PROBE_ONLY 1u
#define NH_Q_WALK_NOBODY 0xffffffffu                            // (nh_query_tree.h's NH_Q_NONE)
#define NH_Q_WALK_MAX_CASTS (2u * (NH_Q_MOVE_MAX_SLIDES + 1u) + 3u)
#define NH_Q_WALK_UP_EPS 0.0009765625f                         // 2^-10: |up.up - 1| above it, `up` is not a unit vector
#define NH_Q_WALK_FLAT_EPS 5.9604644775390625e-08f             // 2^-24: |n - (n.up) up|^2 below it, the face has no horizontal part to slide along
// (AB: A once a steep hit was taken, `blocked`; FOUND: the end behind a cast that wrote the ground record -- D's where the step is accepted, C's)
enum { NH_Q_WALK_A = 0u, NH_Q_WALK_AB = 1u, NH_Q_WALK_U = 2u, NH_Q_WALK_F = 3u, NH_Q_WALK_D = 4u, NH_Q_WALK_C = 5u, NH_Q_WALK_END = 6u, NH_Q_WALK_FOUND = 7u };

// The record's fields the rules read (the capsule itself -- ignore_body, rotation, radius, half_height -- goes into every cast unchanged)
struct nh_QWalkIn { nh_f3 origin, disp, up; float skin, step_height, snap, mgu; uint32_t max_slides, options; };
// One cast's answer as the state keeps it: c = NH_Q_WALK_NOBODY is a miss, whose t is the cast's max_t, 1 -- or the miss record's quiet NaN (0x7fc00000)
// where the cast was invalid
struct nh_QWalkHit { float t; nh_f3 n; uint32_t c; };
// m: the running move loop (its slide budget is the phase's: nh_q_walk_slides); last: its last cast; k*: what is kept; f*: F's end while D runs.  The
// ground record and the drop are written by the cast that ends the walk, so the state keeps the phase FOUND, not a copy: nh_q_walk_ground, _drop.
struct nh_QWalk {
	nh_QMove m; uint32_t phase, casts; float lift;
	nh_QWalkHit last;
	nh_f3 kp, kv; uint32_t kslides, kflags; nh_QWalkHit klast;
	nh_f3 fv; uint32_t fslides, fflags; nh_QWalkHit flast;
	float step_up;
};

// The record's validity (header, "Invalid records"): nh_move's rules (nh_boxmove's for a box) for the first 64 bytes -- `head` -- and the walk's own for the
// 32 bytes behind them, which both shapes share
NH_HD bool nh_q_walk_tail_valid(const nh_QWalkIn& W, bool head) {
	bool ok = head;
	ok = ok && nh_q_move_finite(W.up.x) && nh_q_move_finite(W.up.y) && nh_q_move_finite(W.up.z) && nh_abs(nh_dot(W.up, W.up) - 1.0f) <= NH_Q_WALK_UP_EPS;
	ok = ok && nh_q_move_finite(W.step_height) && !(W.step_height < 0.0f) && nh_q_move_finite(W.snap) && !(W.snap < 0.0f);
	ok = ok && nh_q_move_finite(W.mgu) && W.mgu >= 0.0f && W.mgu <= 1.0f;
	return ok && (W.options & ~NH_Q_WALK_PROBE_ONLY) == 0u;
}

NH_HD bool nh_q_walk_valid(const nh_QWalkIn& W, nh_quat q, float r, float hh) {
	return nh_q_walk_tail_valid(W, nh_q_move_valid(W.origin, W.disp, q, r, hh, W.skin, W.max_slides));
}

NH_HD bool nh_q_boxwalk_valid(const nh_QWalkIn& W, nh_quat q, nh_f3 h) {
	return nh_q_walk_tail_valid(W, nh_q_boxmove_valid(W.origin, W.disp, q, h, W.skin, W.max_slides));
}

NH_HD nh_QWalkHit nh_q_walk_miss() { nh_QWalkHit h; h.t = 1.0f; h.n = nh_make3(0.0f, 0.0f, 0.0f); h.c = NH_Q_WALK_NOBODY; return h; }

NH_HD bool nh_q_walk_walkable(nh_f3 n, const nh_QWalkIn& W) {
	const float u = nh_dot(n, W.up);
	return u > 0.0f && u >= W.mgu;
}

// the next move loop: from p along v
NH_HD void nh_q_walk_start(nh_QWalk& s, uint32_t phase, nh_f3 p, nh_f3 v) {
	s.m = nh_q_move_begin(p, v); s.phase = phase; s.last = nh_q_walk_miss();
}

// the slide budget of the running loop: max_slides in A and F, 0 in U, D (and C, which is one cast)
NH_HD uint32_t nh_q_walk_slides(const nh_QWalk& s, const nh_QWalkIn& W) { return s.phase <= NH_Q_WALK_AB || s.phase == NH_Q_WALK_F ? W.max_slides : 0u; }

NH_HD nh_QWalk nh_q_walk_begin(const nh_QWalkIn& W) {
	nh_QWalk s;
	nh_q_walk_start(s, NH_Q_WALK_A, W.origin, W.disp);
	s.casts = 0u; s.lift = 0.0f;
	s.kp = W.origin; s.kv = W.disp; s.kslides = 0u; s.kflags = 0u; s.klast = s.last;
	s.fv = nh_make3(0.0f, 0.0f, 0.0f); s.fslides = 0u; s.fflags = 0u; s.flast = s.last;
	s.step_up = 0.0f;
	return s;
}

// The ground record and the drop of a walk that has ended
NH_HD nh_QWalkHit nh_q_walk_ground(const nh_QWalk& s) { return s.phase == NH_Q_WALK_FOUND ? s.last : nh_q_walk_miss(); }
NH_HD float nh_q_walk_drop(const nh_QWalk& s, const nh_QWalkIn& W) { return (s.kflags & NH_Q_WALK_SNAPPED) != 0u ? s.last.t * W.snap : 0.0f; }

// C, or the end where there is no probe to make
NH_HD void nh_q_walk_probe(nh_QWalk& s, const nh_QWalkIn& W) {
	if (W.snap > 0.0f) nh_q_walk_start(s, NH_Q_WALK_C, s.kp, (-W.snap) * W.up);
	else s.phase = NH_Q_WALK_END;
}

// The decision behind a move loop that has ended (s.m and s.last hold its end): what the walk does next.  The REPLAY identity calls this between nh_move calls.
NH_HD void nh_q_walk_phase_end(nh_QWalk& s, const nh_QWalkIn& W) {
	const bool overlap = (s.m.flags & NH_Q_MOVE_START_OVERLAP) != 0u;
	if (s.phase <= NH_Q_WALK_AB) {
		s.kp = s.m.p; s.kv = s.m.v; s.kslides = s.m.slides; s.kflags = s.m.flags; s.klast = s.last;
		if (overlap) s.phase = NH_Q_WALK_END;
		else if (W.step_height > 0.0f && s.phase == NH_Q_WALK_AB) nh_q_walk_start(s, NH_Q_WALK_U, W.origin, W.step_height * W.up);
		else nh_q_walk_probe(s, W);
	} else if (s.phase == NH_Q_WALK_U) {
		s.lift = nh_dot(s.m.p - W.origin, W.up);
		if (overlap || !(s.lift > 0.0f)) nh_q_walk_probe(s, W);
		else nh_q_walk_start(s, NH_Q_WALK_F, s.m.p, W.disp);
	} else if (s.phase == NH_Q_WALK_F) {
		if (overlap) nh_q_walk_probe(s, W);
		else {
			s.fv = s.m.v; s.fslides = s.m.slides; s.fflags = s.m.flags; s.flast = s.last;
			nh_q_walk_start(s, NH_Q_WALK_D, s.m.p, (-s.lift) * W.up);
		}
	} else if (s.phase == NH_Q_WALK_D) {
		const nh_f3 dh = W.disp - nh_dot(W.disp, W.up) * W.up;
		const bool landed = (s.m.flags & NH_Q_MOVE_HIT) != 0u && !overlap && nh_q_walk_walkable(s.last.n, W);
		if (landed && nh_dot(s.m.p - W.origin, dh) > nh_dot(s.kp - W.origin, dh)) {
			s.step_up = nh_dot(s.m.p - s.kp, W.up);
			s.kp = s.m.p; s.kv = s.fv; s.kslides = s.fslides; s.klast = s.flast;
			s.kflags = s.fflags | NH_Q_WALK_STEPPED | NH_Q_WALK_GROUNDED;
			s.phase = NH_Q_WALK_FOUND;
		} else nh_q_walk_probe(s, W);
	}
}

// Is there a cast to make?  It is { s.m.p, 1, s.m.v }.  Move loops with nothing to cast along end here (rule 1 of the move).
NH_HD bool nh_q_walk_cast(nh_QWalk& s, const nh_QWalkIn& W) {
	for (uint32_t k = 0u; k < 4u; ++k)
		if (s.phase < NH_Q_WALK_C && !nh_q_move_go(s.m)) nh_q_walk_phase_end(s, W);
	return s.phase < NH_Q_WALK_END;
}

// The slide normal of a taken hit (t > 0) with normal n in the running loop: the climb rule
NH_HD nh_f3 nh_q_walk_slide_normal(nh_QWalk& s, const nh_QWalkIn& W, float t, nh_f3 n) {
	if (W.mgu == 0.0f || !(s.phase <= NH_Q_WALK_AB || s.phase == NH_Q_WALK_F)) return n;
	const float u = nh_dot(n, W.up);
	if (!(u >= 0.0f) || (u > 0.0f && u >= W.mgu)) return n;
	const nh_f3 rem = (1.0f - t) * s.m.v;
	const float sn = nh_dot(rem, n);
	const nh_f3 w = sn < 0.0f ? rem - sn * n : rem;
	if (!(nh_dot(w, W.up) > 0.0f)) return n;
	s.m.flags |= NH_Q_WALK_STEEP;
	const nh_f3 h = n - u * W.up;
	const float hh = nh_dot(h, h);
	if (hh < NH_Q_WALK_FLAT_EPS) return n;
	const float l = sqrtf(hh);
	return nh_make3(h.x / l, h.y / l, h.z / l);
}

// Behind the cast nh_q_walk_cast asked for: (hit, t, c, n) its answer (c: what the caller names the collider by; a miss has t = 1), ok: the
// cast was valid (an invalid cast is a miss)
NH_HD void nh_q_walk_advance(nh_QWalk& s, const nh_QWalkIn& W, bool hit, float t, uint32_t c, nh_f3 n, bool ok) {
	s.casts += 1u;
	s.last.t = ok ? t : nh_asfloat(0x7fc00000u); s.last.n = n; s.last.c = hit ? c : NH_Q_WALK_NOBODY;
	if (s.phase == NH_Q_WALK_C) {
		if (hit) {
			if (nh_q_walk_walkable(n, W)) {
				s.kflags |= NH_Q_WALK_GROUNDED;
				if (!(W.options & NH_Q_WALK_PROBE_ONLY) && t != 0.0f) {
					s.kp = s.kp + t * s.m.v;
					s.kp = s.kp + W.skin * n;
					s.kflags |= NH_Q_WALK_SNAPPED;
				}
			} else s.kflags |= NH_Q_WALK_ON_STEEP;
		}
		s.phase = NH_Q_WALK_FOUND;
		return;
	}
	nh_f3 ns = n;
	if (hit && t != 0.0f) {
		if (s.phase == NH_Q_WALK_A && !nh_q_walk_walkable(n, W)) s.phase = NH_Q_WALK_AB;
		ns = nh_q_walk_slide_normal(s, W, t, n);
	}
	if (!nh_q_move_advance2(s.m, hit, t, n, ns, W.skin, nh_q_walk_slides(s, W))) nh_q_walk_phase_end(s, W);
}

// nh_Touch.phase of a cast asked for in the walk's phase `phase` (nh_walk_touched; the header's NH_TOUCH_*, which nh_query.hip asserts): A and its blocked
// form AB are SLIDE, then U, F, D, C in order.  A move's casts are all SLIDE.
#define NH_Q_TOUCH_SLIDE 0u
#define NH_Q_TOUCH_UP 1u
#define NH_Q_TOUCH_FORWARD 2u
#define NH_Q_TOUCH_DOWN 3u
#define NH_Q_TOUCH_PROBE 4u
NH_HD uint32_t nh_q_walk_touch_phase(uint32_t phase) { return phase <= NH_Q_WALK_AB ? NH_Q_TOUCH_SLIDE : phase - 1u; }

// ---- recover (nh_recover): push a shape out of what it overlaps, the state between two overlap walks -------------------------------------------------
// These functions ARE the definition of nh_recover (include/nudge_hip.h): k_q_recover and the host's brute force (tests/hostoracle/hostrecover.cpp) both run
//     s = nh_q_recover_begin(center);
//     for (;;) { over the set S nh_overlap's predicates accept for the shape at s.p: the pair function's (depth, n) of the collider nh_q_recover_better keeps;
//                if (!nh_q_recover_advance(s, S not empty, depth, n, skin, max_iterations)) break; }
// and write s.p, s.flags, s.p - center, s.iterations and the record of the last pair kept.  Every product is rounded before the sum it goes into (no fused
// multiply-add).  The flag bits are nh_RecoverResult.flags' (nh_query.hip asserts that they are the header's NH_RECOVER_*).
#define NH_Q_RECOVER_PUSHED 1u
#define NH_Q_RECOVER_OVERLAPPING 2u
#define NH_Q_RECOVER_TOUCHING 4u
#define NH_Q_RECOVER_MAX_ITERATIONS 8u

// p: where the shape's centre is; iterations counts exactly the pushes made.
struct nh_QRecover { nh_f3 p; uint32_t iterations, flags; };

// What a recover record adds to the validity of the nh_OverlapQuery it starts with (header, "Invalid records"): a finite skin >= 0 and a push count in range.
NH_HD bool nh_q_recover_valid(float skin, uint32_t max_iterations) {
	return (nh_asuint(skin) & 0x7f800000u) != 0x7f800000u && !(skin < 0.0f) && max_iterations <= NH_Q_RECOVER_MAX_ITERATIONS;
}

NH_HD nh_QRecover nh_q_recover_begin(nh_f3 center) {
	nh_QRecover s;
	s.p = center; s.iterations = 0u; s.flags = 0u;
	return s;
}

// Rule 2's choice among S: the greatest depth, ties to the lowest combined index -- a strict total order on (depth, c), so the collider kept does not
// depend on the order the colliders are met in.  The pair functions return depth >= +0, never -0; a NaN (only non-finite arithmetic on huge finite inputs
// makes one) compares as 0 here, so that the order stays total.  Start with best_c = 0xffffffff, which every index beats at best_depth = 0.
NH_HD bool nh_q_recover_better(float depth, uint32_t c, float best_depth, uint32_t best_c) {
	const float a = nh_q_pen_clamp(depth), b = nh_q_pen_clamp(best_depth);
	return a > b || (a == b && c < best_c);
}

// Rules 1 and 3 - 5 behind one walk with the shape at s.p: `found` says whether S held a collider, (depth, n) are the pair function's for the one kept.
// Returns whether the recover goes on (to the next walk).  Order of operations, per component k:
//   s = depth + skin;  p_k = p_k + (s * n_k)
NH_HD bool nh_q_recover_advance(nh_QRecover& s, bool found, float depth, nh_f3 n, float skin, uint32_t max_iterations) {
	if (!found) return false;
	const float push = depth + skin;
	if (push == 0.0f) { s.flags |= NH_Q_RECOVER_TOUCHING; return false; }
	if (s.iterations == max_iterations) { s.flags |= NH_Q_RECOVER_OVERLAPPING; return false; }
	s.p = s.p + push * n;
	s.iterations += 1u;
	s.flags |= NH_Q_RECOVER_PUSHED;
	return true;
}

// ---- region (nh_region): is a collider inside a convex region, the intersection of up to NH_Q_REGION_MAX_PLANES half-spaces? ------------------------------
// Plane (n, d): a point x is inside iff n.x + d >= 0; n need not be unit length.  The plane KEEPS a collider at world position p iff s + r >= 0.0f with
//   s = nh_dot(n, p) + d
//   r = R * sqrtf(nh_dot(n, n))                                                              for a sphere of radius R
//   r = (h.x * |nh_dot(n, A.c0)| + h.y * |nh_dot(n, A.c1)|) + h.z * |nh_dot(n, A.c2)|        for a box of half extents h, A = nh_matrix(q)
// (r: how far the collider reaches along n, its support distance).  A region keeps a collider iff every one of its planes does: the plane-by-plane frustum
// test.  It never drops a collider that reaches into the region; near an edge or a corner where two planes meet it keeps some that lie outside.  A NaN
// anywhere makes s + r NaN, the >= fails, and the collider is not kept.
#define NH_Q_REGION_MAX_PLANES 8u

NH_HD bool nh_q_region_finite(float x) { return (nh_asuint(x) & 0x7f800000u) != 0x7f800000u; }

// A region's validity: 1 .. 8 planes, every coefficient it reads finite, every n.n finite and > 0.  `planes`: 4 floats per plane.
NH_HD bool nh_q_region_valid(const float* planes, uint32_t plane_count) {
	if (plane_count == 0u || plane_count > NH_Q_REGION_MAX_PLANES) return false;
	bool ok = true;
	for (uint32_t k = 0u; k < plane_count; ++k) {
		const float* pl = planes + 4u * k;
		const float nn = nh_dot(nh_make3(pl[0], pl[1], pl[2]), nh_make3(pl[0], pl[1], pl[2]));
		ok = ok && nh_q_region_finite(pl[0]) && nh_q_region_finite(pl[1]) && nh_q_region_finite(pl[2]) && nh_q_region_finite(pl[3]);
		ok = ok && nh_q_region_finite(nn) && nn > 0.0f;
	}
	return ok;
}

NH_HD bool nh_q_region_keeps_sphere(nh_f3 n, float d, nh_f3 p, float R) {
	const float s = nh_dot(n, p) + d;
	const float r = R * sqrtf(nh_dot(n, n));
	return s + r >= 0.0f;
}

// (A = nh_matrix(q) of the box: the caller computes it once for all planes)
NH_HD bool nh_q_region_keeps_box(nh_f3 n, float d, nh_f3 p, const nh_m33& A, nh_f3 h) {
	const float s = nh_dot(n, p) + d;
	const float r = (h.x * nh_abs(nh_dot(n, A.c0)) + h.y * nh_abs(nh_dot(n, A.c1))) + h.z * nh_abs(nh_dot(n, A.c2));
	return s + r >= 0.0f;
}

// One collider (record: position p, rotation q, half extents h with h.x the radius of a sphere) against the first plane_count planes of a valid region
NH_HD bool nh_q_region_keeps(const float* planes, uint32_t plane_count, nh_f3 p, nh_quat q, nh_f3 h, bool box) {
	bool in = true;
	if (box) {
		const nh_m33 A = nh_matrix(q);
		for (uint32_t k = 0u; k < plane_count; ++k)
			in = in && nh_q_region_keeps_box(nh_make3(planes[4u * k], planes[4u * k + 1u], planes[4u * k + 2u]), planes[4u * k + 3u], p, A, h);
	} else {
		for (uint32_t k = 0u; k < plane_count; ++k)
			in = in && nh_q_region_keeps_sphere(nh_make3(planes[4u * k], planes[4u * k + 1u], planes[4u * k + 2u]), planes[4u * k + 3u], p, h.x);
	}
	return in;
}

// The node test of nh_region's kernel: is the box [lo, hi] SURELY outside the plane (n, d)?  g = the largest value of n.x + d over the box, term by term
// (fmaxf of the two products per axis); the box is outside iff g + m < 0 with the margin
//   m = 2^-18 * (|n.x| * max(|lo.x|, |hi.x|) + |n.y| * max(|lo.y|, |hi.y|) + |n.z| * max(|lo.z|, |hi.z|) + |d|)
// Only a comparison that is TRUE prunes: a NaN box or an overflow prunes nothing.  Conservative against the predicates above: in real
// arithmetic s + r of a collider is at most g of its world AABB, hence of every box that contains it; the roundings of s + r and of g are each below
// 2^-20 of the bracket of m, which is evaluated on a box that contains the collider's coordinates.
NH_HD bool nh_q_region_node_outside(nh_f3 n, float d, nh_f3 lo, nh_f3 hi) {
	const float g = ((fmaxf(n.x * lo.x, n.x * hi.x) + fmaxf(n.y * lo.y, n.y * hi.y)) + fmaxf(n.z * lo.z, n.z * hi.z)) + d;
	const float m = (((fabsf(n.x) * fmaxf(fabsf(lo.x), fabsf(hi.x)) + fabsf(n.y) * fmaxf(fabsf(lo.y), fabsf(hi.y))) + fabsf(n.z) * fmaxf(fabsf(lo.z), fabsf(hi.z))) +
	                 fabsf(d)) * 3.814697265625e-06f;
	return g + m < 0.0f;
}

// ---- events: the per-record functions of nh_overlap_bodies / nh_overlap_events (nh_query.hip, "events"; tests/hostoracle/hostevents.cpp) ------------------
// A list is what a list call of nh_overlap / nh_region wrote: offsets[0 .. count], records of four words (body, collider, shape, tag) and the capacity
// the call was given.  Nothing here reads a record at or beyond `capacity`, whatever the offsets hold.
#define NH_Q_EVENTS_BY_BODY 1u

// Segment i (i < count) is PRESENT iff its records were written: offsets[i+1] <= capacity and no overflow marker -- nh_overlap's written-prefix rule.  A
// non-monotone pair (lists no call wrote) is absent, so a present segment is a range [offsets[i], offsets[i+1]) inside the records.
NH_HD bool nh_q_seg_present(const uint32_t* offsets, uint32_t count, uint32_t capacity, uint32_t i) {
	return offsets[count] != 0xffffffffu && offsets[i + 1u] <= capacity && offsets[i] <= offsets[i + 1u];
}

// The segment of record r: the last i in [0, count] with offsets[i] <= r, so that empty segments are stepped over (offsets[0] = 0 <= r always; offsets
// that do not start at 0 give 0).  `count` itself says that r lies at or behind the total.
NH_HD uint32_t nh_q_seg_of(const uint32_t* offsets, uint32_t count, uint32_t r) {
	uint32_t lo = 0u, hi = count;          // the answer is in [lo, hi]
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo + 1u) / 2u;
		if (offsets[mid] <= r) lo = mid; else hi = mid - 1u;
	}
	return lo;
}

// The segment record r of a list belongs to when that record is one of a present segment; 0xffffffff otherwise (r < capacity is the caller's bound).
NH_HD uint32_t nh_q_seg_of_present(const uint32_t* offsets, uint32_t count, uint32_t capacity, uint32_t r) {
	const uint32_t i = nh_q_seg_of(offsets, count, r);
	if (i >= count || !nh_q_seg_present(offsets, count, capacity, i) || r < offsets[i] || r >= offsets[i + 1u]) return 0xffffffffu;
	return i;
}

// A record's identity as one ordered word: the body (NH_Q_EVENTS_BY_BODY), or (shape, collider) -- with the boxes first that is the combined collider
// index's order, the order nh_overlap writes a segment in; nh_overlap_bodies writes a segment by body.
NH_HD uint64_t nh_q_ident(const uint32_t* rec, uint32_t by_body) { return by_body ? (uint64_t)rec[0] : ((uint64_t)rec[2] << 32) | rec[1]; }

// Is the identity `key` among records [lo, hi) of `hits` (four words a record, sorted by identity)?  A lower-bound search; lo <= hi <= capacity.
NH_HD bool nh_q_ident_find(const uint32_t* hits, uint32_t lo, uint32_t hi, uint64_t key, uint32_t by_body) {
	const uint32_t end = hi;
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2u;
		if (nh_q_ident(hits + 4u * (uint64_t)mid, by_body) < key) lo = mid + 1u; else hi = mid;
	}
	return lo < end && nh_q_ident(hits + 4u * (uint64_t)lo, by_body) == key;          // (every record read lies in [lo, end) of the call)
}

// ---- sensors (nh_sense, nh_sense_rays): the ray of beam j of sensor s ------------------------------------------------------------------------------
// A sensor is a pose and a mount; a beam a sensor-local direction and a range.  The pose is the sensor's own (world frame: no mount), or the sensor's as
// the LOCAL transform of the body it rides on -- nh_collider_pose, the arithmetic that puts a collider on its body.  A mount that does not exist makes the
// pose a quiet NaN, and with it every ray of the sensor: "a ray with a non-finite origin or direction", a miss with t = NaN.
// The ray is (origin = p, max_t = range, direction = rotate(q, beam direction), ignore_body): nh_Ray's eight words, which nh_sense_rays stores and
// nh_sense casts from registers.  Only + - * here: the host oracle (tests/hostoracle/hostsense.cpp) gets the device's bits.
// mounted: the call has bodies and the sensor's body word is not 0xffffffff; exists: false only for a mounted sensor whose body index is out of range.
NH_HD nh_QPose nh_q_sensor_pose(nh_f3 sp, nh_quat sq, bool mounted, bool exists, nh_f3 bp, nh_quat bq) {
	nh_QPose w;
	w.p = sp; w.q = sq;
	if (mounted && exists) nh_collider_pose(bq, bp, sq, sp, w.p, w.q);
	if (mounted && !exists) {                    // (bp, bq are not read)
		const float nan = nh_asfloat(0x7fc00000u);
		w.p = nh_make3(nan, nan, nan); w.q = nh_quat{ nan, nan, nan, nan };
	}
	return w;
}

struct nh_QSensorRay { nh_f3 o; float max_t; nh_f3 d; uint32_t ignore; };
// `exists` as above: the rotation of a NaN quaternion would be a NaN of the platform's making; the contract wants 0x7fc00000 in all six words
NH_HD nh_QSensorRay nh_q_sensor_ray(nh_QPose w, bool exists, nh_f3 beam, float range, uint32_t ignore) {
	nh_QSensorRay r;
	r.o = w.p; r.max_t = range; r.ignore = ignore;
	r.d = exists ? nh_rotate(w.q, beam) : w.p;
	return r;
}

// ---- fast bodies (nh_sweep, nh_sweep_limit): the sweep of a collider along its own velocity --------------------------------------------------------
// A collider at p_c of body b (position p_b, velocity v, angular velocity w) travels d = (v + w x (p_c - p_b)) * time_step in the coming step: two
// products and one subtraction per component of the cross product, one sum, one product -- only + - *, so the host oracle
// (tests/hostoracle/hostsweep.cpp) gets the device's bits.  It is SELECTED iff its body is a dynamic one that exists and |d|^2 > (min_travel * m)^2, m its
// smallest half extent (a sphere: its radius); any NaN makes the comparison false.  The cast is (origin = p_c, max_t = 1, direction = d, ignore_body =
// b, rotation, size = h * core): nh_BoxCast's words for a box, nh_CapsuleCast's with the identity rotation, radius h.x * core and half height 0 for a sphere.
NH_HD nh_f3 nh_q_sweep_travel(nh_f3 pc, nh_f3 pb, nh_f3 v, nh_f3 w, float time_step) {
	const nh_f3 r = nh_make3(pc.x - pb.x, pc.y - pb.y, pc.z - pb.z);
	const nh_f3 u = nh_make3(v.x + (w.y * r.z - w.z * r.y), v.y + (w.z * r.x - w.x * r.z), v.z + (w.x * r.y - w.y * r.x));
	return nh_make3(u.x * time_step, u.y * time_step, u.z * time_step);
}
// (asked BEFORE the body's state is read: a body that does not exist has none)
NH_HD bool nh_q_sweep_body(uint32_t body, uint32_t body_count) { return body > 0u && body < body_count; }
NH_HD bool nh_q_sweep_far(nh_f3 d, nh_f3 h, bool box, float min_travel) {
	const float m = box ? nh_min(nh_min(h.x, h.y), h.z) : h.x;
	const float s = min_travel * m;
	return ((d.x * d.x + d.y * d.y) + d.z * d.z) > s * s;
}
// the swept core: words 12 .. 14 of the cast record (a sphere: radius, half height 0, and the first reserved word 0)
NH_HD nh_f3 nh_q_sweep_core(nh_f3 h, bool box, float core) { return box ? nh_make3(h.x * core, h.y * core, h.z * core) : nh_make3(h.x * core, 0.0f, 0.0f); }
// an entry LIMITS its body iff its hit is a real one behind the start: a core that starts in overlap (t == 0) limits nothing
NH_HD bool nh_q_sweep_limits(uint32_t shape, float t) { return shape != 0xffffffffu /* NH_SHAPE_NONE */ && t > 0.0f; }

#endif
