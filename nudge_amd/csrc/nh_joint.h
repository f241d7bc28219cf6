// nh_joint.h -- per-item logic of the joints (include/nudge_hip.h, "joints"; nh_joints.hip): a joint's validity, the cut points of the
// schedule, the rows of one joint, the warm start and one visit of a row.  Every function is `NH_HD`, as nh_impulse.h's are, so that
// tests/hostoracle/hostjoint.cpp builds the SAME arithmetic with g++ -ffp-contract=off and gets the device's bits; what the oracle judges is everything
// around them -- the levels, the order, who is live, and that a level-parallel replay is the serial loop.
//
// The arithmetic, stated once (the header repeats it for callers).  Only + - * /, sqrtf and compares, and what nh_rotate, nh_cross, nh_dot, nh_world_inertia and
// nh_tangents do (nh_math.h, nh_solver.h); dot products and 3x3 products associate left to right: (x + y) + z.
//   side x of a joint   p_x, q_x = transforms[x]; mi_x = properties[x].mass_inverse; W_x = nh_world_inertia(q_x, inertia_inverse).  Body 0: the transform is read
//                       like any other, mi = 0, W = 0, its velocity counts as zero and its momentum is never read or written.
//   frame               r_x = rotate(q_x, anchor_x);  d = (p_b + r_b) - (p_a + r_a)
//   a row               a linear direction n (angular rows: none), ja and jb (linear: ja = -(r_a x n), jb = r_b x n; angular: ja = -t, jb = t, the sign bit
//                       inverted), wa = W_a ja, wb = W_b jb, k = ((mi_a + mi_b) + ja . wa) + jb . wb (angular: ja . wa + jb . wb), m = k > 0 ? 1 / k : 0,
//                       bias = clamp(beta * C, -max_bias, max_bias) with beta = time_step > 0 ? baumgarte / time_step : 0, bounds [lo, hi].
//   BALL                three rows n = e_x, e_y, e_z, C = d.x, d.y, d.z, unbounded.
//   DISTANCE            one row; len = sqrtf(d . d), n = len > 0 ? d / len : (0, 1, 0).  min == max: C = len - min, unbounded; len > max: C = len - max,
//                       [-inf, 0]; len < min: C = len - min, [0, +inf]; otherwise DEAD: m = 0, bias = 0, bounds [0, 0], accumulated impulse +0.
//   HINGE               BALL's three rows, then two angular ones: a1 = rotate(q_a, axis_a), a2 = rotate(q_b, axis_b), (t1, t2) = nh_tangents(a1),
//                       C_k = (a1 x a2) . t_k, unbounded.
//   one visit           jv = (n . (v_b - v_a) + ja . w_a) + jb . w_b (angular: ja . w_a + jb . w_b); lambda = -(jv + bias) * m; acc' = clamp(acc + lambda, lo, hi);
//                       delta = acc' - acc; v_a -= n * (delta * mi_a); w_a += wa * delta; v_b += n * (delta * mi_b); w_b += wb * delta (angular rows leave v alone).
//   warm start          acc = warm * impulses.row[k] (a dead row: +0), applied like a delta.
//   clamp(x, lo, hi)    x < lo ? lo : (x > hi ? hi : x).
#ifndef NH_JOINT_H
#define NH_JOINT_H

#include "nh_solver.h"
#include "../../include/nudge_hip.h"

#define NH_JOINT_SPAN_MAX (NH_JOINT_ASSEMBLY_MAX + NH_JOINT_BIN - 1u)          // joints of one bin at most: 1279
#define NH_JOINT_ROWS_MAX 5u

// ---- validity and the schedule's cut points ---------------------------------------------------------------------------------------------------------
NH_HD bool nh_j_valid(uint32_t a, uint32_t b, uint32_t type, uint32_t flags, float p0, float p1, uint32_t body_count) {
	if (type != NH_JOINT_BALL && type != NH_JOINT_DISTANCE && type != NH_JOINT_HINGE) return false;
	if (flags != 0u || a == b || a >= body_count || b >= body_count) return false;
	if (type == NH_JOINT_DISTANCE && !(0.0f <= p0 && p0 <= p1)) return false;          // (comparisons: a NaN is invalid)
	return true;
}
NH_HD bool nh_j_valid(const nh_Joint& j, uint32_t body_count) { return nh_j_valid(j.a, j.b, j.type, j.flags, j.p[0], j.p[1], body_count); }

NH_HD uint32_t nh_j_rows(uint32_t type) { return type == NH_JOINT_BALL ? 3u : type == NH_JOINT_DISTANCE ? 1u : type == NH_JOINT_HINGE ? 5u : 0u; }

// the list's cut points: offsets[0 .. assemblies], or (0, count) for a list without offsets
NH_HD uint32_t nh_j_assemblies(const uint32_t* offsets, uint32_t assemblies) { return offsets ? assemblies : 1u; }
NH_HD uint32_t nh_j_offset(const uint32_t* offsets, uint32_t count, uint32_t i) { return offsets ? offsets[i] : (i == 0u ? 0u : count); }

// the first i in [0, A] whose offset is >= x, or A + 1 (offsets ascending)
NH_HD uint32_t nh_j_lower(const uint32_t* offsets, uint32_t A, uint32_t count, uint32_t x) {
	uint32_t lo = 0u, hi = A + 1u;
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2u;
		if (nh_j_offset(offsets, count, mid) < x) lo = mid + 1u; else hi = mid;
	}
	return lo;
}
// where bin w's span starts (bin w + 1's start is its end): the offset of the first assembly that starts at or behind 256 w, at most count
NH_HD uint32_t nh_j_span_begin(const uint32_t* offsets, uint32_t A, uint32_t count, uint32_t w) {
	const uint32_t i = nh_j_lower(offsets, A, count, w * NH_JOINT_BIN);
	const uint32_t o = i <= A ? nh_j_offset(offsets, count, i) : count;
	return o < count ? o : count;
}
// the bin of joint j (j < count, offsets checked): that of the last assembly that starts at or before j
NH_HD uint32_t nh_j_bin_of(const uint32_t* offsets, uint32_t A, uint32_t count, uint32_t j) {
	const uint32_t i = nh_j_lower(offsets, A, count, j + 1u);          // the first assembly that starts behind j
	return nh_j_offset(offsets, count, i ? i - 1u : 0u) / NH_JOINT_BIN;
}
NH_HD uint32_t nh_j_bins(uint32_t count) { return (count + NH_JOINT_BIN - 1u) / NH_JOINT_BIN; }

// ---- the records of the solve (context scratch; 432 B per joint: 27 16-byte words) ---------------------------------------------------------------------
struct nh_JRow { float n[3], m; float ja[3], bias; float jb[3], lo; float wa[3], hi; float wb[3], acc; };          // 80 B
struct nh_JHead { uint32_t a, b, rows /* 0: not live this step */, type; float mi_a, mi_b, pad[2]; };               // 32 B
struct nh_JSolve { nh_JHead head; nh_JRow row[NH_JOINT_ROWS_MAX]; };

struct nh_JSide { nh_f3 p; nh_quat q; nh_inertia W; float mi; };
struct nh_JMom { float v[3], u0, w[3], u1; };          // nh_BodyMomentum's words (u0 / u1: unused0 / unused1, stored back as loaded)

NH_HD nh_JSide nh_j_side(uint32_t body, const nh_Transform& t, const nh_BodyProperties& pr) {
	nh_JSide s;
	s.p = nh_make3(t.position[0], t.position[1], t.position[2]);
	s.q = nh_quat{ t.rotation[0], t.rotation[1], t.rotation[2], t.rotation[3] };
	if (body == 0u) { s.W = nh_inertia{ 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }; s.mi = 0.0f; }
	else { s.W = nh_world_inertia(s.q, pr.inertia_inverse[0], pr.inertia_inverse[1], pr.inertia_inverse[2]); s.mi = pr.mass_inverse; }
	return s;
}

NH_HD nh_f3 nh_j_mul(const nh_inertia& W, nh_f3 t) {
	return nh_make3((W.xx * t.x + W.xy * t.y) + W.xz * t.z, (W.xy * t.x + W.yy * t.y) + W.yz * t.z, (W.xz * t.x + W.yz * t.y) + W.zz * t.z);
}
NH_HD nh_f3 nh_j_neg(nh_f3 a) { return nh_make3(nh_neg(a.x), nh_neg(a.y), nh_neg(a.z)); }
NH_HD float nh_j_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }
NH_HD bool nh_j_linear(uint32_t type, uint32_t k) { return !(type == NH_JOINT_HINGE && k >= 3u); }

struct nh_JFrame { nh_f3 ra, rb, d; };
NH_HD nh_JFrame nh_j_frame(const nh_Joint& j, const nh_JSide& A, const nh_JSide& B) {
	nh_JFrame f;
	f.ra = nh_rotate(A.q, nh_make3(j.anchor_a[0], j.anchor_a[1], j.anchor_a[2]));
	f.rb = nh_rotate(B.q, nh_make3(j.anchor_b[0], j.anchor_b[1], j.anchor_b[2]));
	f.d = (B.p + f.rb) - (A.p + f.ra);
	return f;
}

// Row k of joint j (k < nh_j_rows(j.type)), its accumulated impulse +0.  *dead: the row is a DISTANCE row between its bounds.
NH_HD nh_JRow nh_j_row(const nh_Joint& j, uint32_t k, const nh_JFrame& f, const nh_JSide& A, const nh_JSide& B, const nh_JointParams& pm, bool* dead) {
	nh_f3 n = nh_make3(0.0f, 0.0f, 0.0f), ja, jb;
	float C = 0.0f, lo = nh_asfloat(0xff800000u), hi = nh_asfloat(0x7f800000u);
	*dead = false;
	const bool linear = nh_j_linear(j.type, k);
	if (j.type == NH_JOINT_DISTANCE) {
		const float len = sqrtf(nh_dot(f.d, f.d));
		n = len > 0.0f ? nh_make3(f.d.x / len, f.d.y / len, f.d.z / len) : nh_make3(0.0f, 1.0f, 0.0f);
		const float mn = j.p[0], mx = j.p[1];
		if (mn == mx) C = len - mn;
		else if (len > mx) { C = len - mx; hi = 0.0f; }
		else if (len < mn) { C = len - mn; lo = 0.0f; }
		else { *dead = true; lo = 0.0f; hi = 0.0f; }
	} else if (linear) {
		n = nh_make3(k == 0u ? 1.0f : 0.0f, k == 1u ? 1.0f : 0.0f, k == 2u ? 1.0f : 0.0f);
		C = k == 0u ? f.d.x : (k == 1u ? f.d.y : f.d.z);
	}
	if (linear) {
		ja = nh_j_neg(nh_cross(f.ra, n));
		jb = nh_cross(f.rb, n);
	} else {
		const nh_f3 a1 = nh_rotate(A.q, nh_make3(j.p[0], j.p[1], j.p[2])), a2 = nh_rotate(B.q, nh_make3(j.p[3], j.p[4], j.p[5]));
		nh_f3 t1, t2;
		nh_tangents(a1.x, a1.y, a1.z, t1, t2);
		const nh_f3 t = k == 3u ? t1 : t2;
		C = nh_dot(nh_cross(a1, a2), t);
		ja = nh_j_neg(t);
		jb = t;
	}
	const nh_f3 wa = nh_j_mul(A.W, ja), wb = nh_j_mul(B.W, jb);
	const float kk = linear ? ((A.mi + B.mi) + nh_dot(ja, wa)) + nh_dot(jb, wb) : nh_dot(ja, wa) + nh_dot(jb, wb);
	const float beta = pm.time_step > 0.0f ? pm.baumgarte / pm.time_step : 0.0f;
	nh_JRow r;
	r.n[0] = n.x; r.n[1] = n.y; r.n[2] = n.z;
	r.m = *dead ? 0.0f : (kk > 0.0f ? 1.0f / kk : 0.0f);
	r.ja[0] = ja.x; r.ja[1] = ja.y; r.ja[2] = ja.z;
	r.bias = *dead ? 0.0f : nh_j_clamp(beta * C, nh_neg(pm.max_bias), pm.max_bias);
	r.jb[0] = jb.x; r.jb[1] = jb.y; r.jb[2] = jb.z;
	r.lo = lo;
	r.wa[0] = wa.x; r.wa[1] = wa.y; r.wa[2] = wa.z;
	r.hi = hi;
	r.wb[0] = wb.x; r.wb[1] = wb.y; r.wb[2] = wb.z;
	r.acc = 0.0f;
	return r;
}

// `delta` of row r into the two bodies' momentum (a body 0's words are scratch of the caller's: never loaded, never stored)
NH_HD void nh_j_push(const nh_JRow& r, bool linear, float delta, float mi_a, float mi_b, nh_JMom& ma, nh_JMom& mb) {
	if (linear) {
		const float da = delta * mi_a, db = delta * mi_b;
		ma.v[0] = ma.v[0] - r.n[0] * da; ma.v[1] = ma.v[1] - r.n[1] * da; ma.v[2] = ma.v[2] - r.n[2] * da;
		mb.v[0] = mb.v[0] + r.n[0] * db; mb.v[1] = mb.v[1] + r.n[1] * db; mb.v[2] = mb.v[2] + r.n[2] * db;
	}
	ma.w[0] = ma.w[0] + r.wa[0] * delta; ma.w[1] = ma.w[1] + r.wa[1] * delta; ma.w[2] = ma.w[2] + r.wa[2] * delta;
	mb.w[0] = mb.w[0] + r.wb[0] * delta; mb.w[1] = mb.w[1] + r.wb[1] * delta; mb.w[2] = mb.w[2] + r.wb[2] * delta;
}

// One visit of row r: the new accumulated impulse is left in r.acc.
NH_HD void nh_j_visit(nh_JRow& r, bool linear, float mi_a, float mi_b, nh_JMom& ma, nh_JMom& mb) {
	const nh_f3 ja = nh_make3(r.ja[0], r.ja[1], r.ja[2]), jb = nh_make3(r.jb[0], r.jb[1], r.jb[2]);
	const nh_f3 wa = nh_make3(ma.w[0], ma.w[1], ma.w[2]), wb = nh_make3(mb.w[0], mb.w[1], mb.w[2]);
	float jv;
	if (linear) {
		const nh_f3 dv = nh_make3(mb.v[0] - ma.v[0], mb.v[1] - ma.v[1], mb.v[2] - ma.v[2]);
		jv = (nh_dot(nh_make3(r.n[0], r.n[1], r.n[2]), dv) + nh_dot(ja, wa)) + nh_dot(jb, wb);
	} else jv = nh_dot(ja, wa) + nh_dot(jb, wb);
	const float lambda = nh_neg(jv + r.bias) * r.m;
	const float acc = nh_j_clamp(r.acc + lambda, r.lo, r.hi);
	const float delta = acc - r.acc;
	r.acc = acc;
	nh_j_push(r, linear, delta, mi_a, mi_b, ma, mb);
}

NH_HD nh_JMom nh_j_zero_mom() { nh_JMom m; m.v[0] = m.v[1] = m.v[2] = m.u0 = m.w[0] = m.w[1] = m.w[2] = m.u1 = 0.0f; return m; }

#endif
