// nh_impulse.h -- per-item logic of the body impulses (include/nudge_hip.h, "body impulses"; nh_impulse.hip): a record's validity and its pair (L, T), the
// walk of one RUN of the list, the merge of one body's runs, the change of one momentum record, and the two generators' records.  Every function is
// `NH_HD`, as nh_contact_events.h's are, so that tests/hostoracle/hostimpulse.cpp builds the SAME arithmetic with g++ -ffp-contract=off and gets the
// device's bits; what the oracle judges is everything around them -- flags, scans, the sort, the output rules.
//
// The functions read their arrays through a LOADER (body(i), record(i), position(b), part(r)): the device's issues 16-byte loads, the oracle's reads structs.
//
// The rules (the header states them for callers):
//   valid     0 < body < body_count (body 0 is the static world; NH_IMPULSE_NO_BODY fails the same test).
//   pair      L = impulse; T = (+0, +0, +0) with NH_IMPULSE_AT_CENTRE, else r x L with r = point - position(body): two products and one subtraction
//             per component.
//   run       a maximal stretch of consecutive valid records of one body.  Its six sums start at +0 and take the records left to right in fp32.
//   body sum  starts at +0 and takes the runs' sums in list order.
#ifndef NH_IMPULSE_H
#define NH_IMPULSE_H

#include "nh_solver.h"
#include "../../include/nudge_hip.h"

NH_HD bool nh_bi_valid(uint32_t body, uint32_t body_count) { return body != 0u && body < body_count; }

// bits of one body index in the sort key: those of body_count - 1, at least one -- and the radix sort's end bit for them: whole 8-bit digits
NH_HD uint32_t nh_bi_bits(uint32_t body_count) {
	if (body_count == 0u) return 32u;
	uint32_t b = 1u;
	while (b < 32u && ((body_count - 1u) >> b)) ++b;
	return b;
}
NH_HD int nh_bi_sort_bits(uint32_t bits) { return (int)((bits + 7u) / 8u * 8u); }

// Is record i of the list a run head?  (An invalid neighbour has another body by the validity test itself.)
template <class Load>
NH_HD bool nh_bi_run_head(const Load& ld, uint32_t body_count, uint32_t i) {
	const uint32_t b = ld.body(i);
	return nh_bi_valid(b, body_count) && (i == 0u || ld.body(i - 1u) != b);
}

// a record's pair, added to the six sums
NH_HD void nh_bi_add(const nh_BodyImpulse& r, nh_f3 p, float* lin, float* ang) {
	const float jx = r.impulse[0], jy = r.impulse[1], jz = r.impulse[2];
	float tx = 0.0f, ty = 0.0f, tz = 0.0f;
	if (!(r.flags & NH_IMPULSE_AT_CENTRE)) {
		const float rx = r.point[0] - p.x, ry = r.point[1] - p.y, rz = r.point[2] - p.z;
		tx = ry * jz - rz * jy;
		ty = rz * jx - rx * jz;
		tz = rx * jy - ry * jx;
	}
	lin[0] = lin[0] + jx; lin[1] = lin[1] + jy; lin[2] = lin[2] + jz;
	ang[0] = ang[0] + tx; ang[1] = ang[1] + ty; ang[2] = ang[2] + tz;
}

// The partial sum of the run that STARTS at record i of a list of n (i is a run head).
template <class Load>
NH_HD nh_ImpulseSum nh_bi_run(const Load& ld, uint32_t n, uint32_t i) {
	nh_ImpulseSum s;
	s.body = ld.body(i);
	s.linear[0] = s.linear[1] = s.linear[2] = 0.0f;
	s.angular[0] = s.angular[1] = s.angular[2] = 0.0f;
	const nh_f3 p = ld.position(s.body);
	uint32_t j = i;
	do nh_bi_add(ld.record(j), p, s.linear, s.angular);
	while (++j < n && ld.body(j) == s.body);
	s.count = j - i;
	return s;
}

// The sum of the body whose runs are the sorted positions w, w + 1, ... with the key of w (w is a body head: w == 0 or keys[w - 1] differs); the
// stable sort left them in list order.
template <class Load>
NH_HD nh_ImpulseSum nh_bi_merge(const Load& ld, const uint64_t* keys, const uint32_t* vals, uint32_t runs, uint32_t w) {
	const uint64_t key = keys[w];
	nh_ImpulseSum o = ld.part(vals[w]);
	for (int c = 0; c < 3; ++c) { o.linear[c] = 0.0f + o.linear[c]; o.angular[c] = 0.0f + o.angular[c]; }
	for (uint32_t u = w + 1u; u < runs && keys[u] == key; ++u) {
		const nh_ImpulseSum q = ld.part(vals[u]);
		for (int c = 0; c < 3; ++c) { o.linear[c] = o.linear[c] + q.linear[c]; o.angular[c] = o.angular[c] + q.angular[c]; }
		o.count += q.count;
	}
	return o;
}

// The six velocity words of a body after its sum: v (velocity) and a (angular_velocity) in place.
NH_HD void nh_bi_apply(float* v, float* a, const float rotation[4], const nh_BodyProperties& pr, const nh_ImpulseSum& s) {
	v[0] = v[0] + s.linear[0] * pr.mass_inverse;
	v[1] = v[1] + s.linear[1] * pr.mass_inverse;
	v[2] = v[2] + s.linear[2] * pr.mass_inverse;
	const nh_quat q = { rotation[0], rotation[1], rotation[2], rotation[3] };
	const nh_inertia W = nh_world_inertia(q, pr.inertia_inverse[0], pr.inertia_inverse[1], pr.inertia_inverse[2]);
	const float tx = s.angular[0], ty = s.angular[1], tz = s.angular[2];
	a[0] = a[0] + ((W.xx * tx + W.xy * ty) + W.xz * tz);
	a[1] = a[1] + ((W.xy * tx + W.yy * ty) + W.yz * tz);
	a[2] = a[2] + ((W.xz * tx + W.yz * ty) + W.zz * tz);
}

NH_HD nh_BodyImpulse nh_bi_nobody() {
	nh_BodyImpulse r;
	r.point[0] = r.point[1] = r.point[2] = 0.0f; r.body = NH_IMPULSE_NO_BODY;
	r.impulse[0] = r.impulse[1] = r.impulse[2] = 0.0f; r.flags = 0u;
	return r;
}

// The segment an index r of a list belongs to: the largest i <= count with offsets[i] <= r, at most count - 1 (count > 0).
NH_HD uint32_t nh_bi_segment(const uint32_t* offsets, uint32_t count, uint32_t r) {
	uint32_t lo = 0u, hi = count;          // the answer is in [lo, hi]
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo + 1u) / 2u;
		if (offsets[mid] <= r) lo = mid; else hi = mid - 1u;
	}
	return lo < count ? lo : count - 1u;
}

// nh_blast_impulses' record of one hit body (ld.position(b) is read only for a body that exists)
template <class Load>
NH_HD nh_BodyImpulse nh_bi_blast(const Load& ld, const nh_Blast& b, uint32_t body, uint32_t body_count) {
	nh_BodyImpulse o = nh_bi_nobody();
	if (!nh_bi_valid(body, body_count)) return o;
	const nh_f3 p = ld.position(body);
	const float rx = p.x - b.centre[0], ry = p.y - b.centre[1], rz = p.z - b.centre[2];
	const float d = sqrtf((rx * rx + ry * ry) + rz * rz);
	const float s = b.strength * (1.0f - b.falloff * (d / b.radius));
	if (!(s > 0.0f)) return o;
	const bool apart = d > 0.0f;
	const float dx = apart ? rx / d : 0.0f, dy = apart ? ry / d : 1.0f, dz = apart ? rz / d : 0.0f;
	o.point[0] = p.x; o.point[1] = p.y; o.point[2] = p.z; o.body = body;
	o.impulse[0] = dx * s; o.impulse[1] = dy * s; o.impulse[2] = dz * s; o.flags = NH_IMPULSE_AT_CENTRE;
	return o;
}

// nh_touch_impulses' record of one WRITTEN touch slot (j < min(counts[i], k) is the caller's test: unwritten slots are never read)
NH_HD nh_BodyImpulse nh_bi_touch(const nh_Push& p, const nh_Touch& t) {
	nh_BodyImpulse o = nh_bi_nobody();
	if (t.hit.shape == NH_SHAPE_NONE || t.hit.body == 0u || !(t.hit.t > 0.0f)) return o;
	if (t.phase >= 32u || !((p.phases >> t.phase) & 1u)) return o;
	const float* d = t.direction;
	const float* n = t.hit.normal;
	const float a = nh_neg((d[0] * n[0] + d[1] * n[1]) + d[2] * n[2]);
	if (!(a > 0.0f)) return o;
	const float m = nh_min(p.mass_over_dt * a, p.max_impulse);
	o.point[0] = t.origin[0] + d[0] * t.hit.t; o.point[1] = t.origin[1] + d[1] * t.hit.t; o.point[2] = t.origin[2] + d[2] * t.hit.t;
	o.body = t.hit.body;
	o.impulse[0] = nh_neg(n[0]) * m; o.impulse[1] = nh_neg(n[1]) * m; o.impulse[2] = nh_neg(n[2]) * m;
	o.flags = p.flags;
	return o;
}

#endif
