// tests/hostsim/hostsim.cpp -- CPU-side UNIT-TEST harness (never part of the product, never a fallback).
//
// Compiles the per-item device functions of nudge_amd/csrc/nh_*.h with g++ so that the arithmetic the HIP
// kernels execute can be diffed against the compiled reference (oracle/_ref) on this GPU-less dev box.
// The parallel plumbing of the kernels (sort / scan / compaction / scheduling) is NOT modelled here: this
// harness uses O(n^2) loops and takes the solver order from the oracle.
#include "../../nudge_amd/csrc/nh_math.h"
#include "../../nudge_amd/csrc/nh_narrowphase.h"
#include "../../nudge_amd/csrc/nh_solver.h"
#include <vector>
#include <algorithm>

struct Xf { float p[3]; uint32_t body; float q[4]; };

// The world pose and the exact AABB of every collider (boxes first, then spheres), as k_xform computes them, and the broadphase's pair rule:
// strictly overlapping AABBs (nudge.cpp:3306-3308) of colliders on two different bodies.  Shared by hs_collide and hs_pairs.
struct Boxes {
	std::vector<nh_xform> xf;
	std::vector<float> mn, mx;
	std::vector<uint32_t> tags;
	bool is_pair(uint32_t i, uint32_t j) const {
		const bool ov = mx[3*j] > mn[3*i] && mx[3*i] > mn[3*j] && mx[3*j+1] > mn[3*i+1] && mx[3*i+1] > mn[3*j+1] && mx[3*j+2] > mn[3*i+2] && mx[3*i+2] > mn[3*j+2];
		return ov && xf[i].body != xf[j].body;
	}
};

static Boxes world_boxes(const Xf* body_xf, uint32_t nbox, const Xf* box_xf, const float* box_size /*4 per*/, const uint32_t* box_tags,
                         uint32_t nsph, const Xf* sph_xf, const float* sph_radius, const uint32_t* sph_tags) {
	const uint32_t n = nbox + nsph;
	Boxes w;
	w.xf.resize(n); w.mn.resize(3 * (size_t)n); w.mx.resize(3 * (size_t)n); w.tags.resize(n);
	std::vector<nh_xform>& xf = w.xf;
	std::vector<float>& mn = w.mn; std::vector<float>& mx = w.mx;
	std::vector<uint32_t>& tags = w.tags;
	for (uint32_t i = 0; i < n; ++i) {
		const Xf& l = i < nbox ? box_xf[i] : sph_xf[i - nbox];
		const Xf& b = body_xf[l.body];
		nh_f3 p, reach, lo, hi;
		nh_quat q;
		nh_collider_pose(b.p, b.q, l.p, l.q, p, q);
		xf[i].px = p.x; xf[i].py = p.y; xf[i].pz = p.z; xf[i].body = l.body;
		xf[i].qx = q.x; xf[i].qy = q.y; xf[i].qz = q.z; xf[i].qs = q.s;
		if (i < nbox) {
			const float* s = box_size + 4 * i;
			reach = nh_box_reach(q, nh_make3(s[0], s[1], s[2]));
			tags[i] = box_tags[i];
		} else {
			reach.x = reach.y = reach.z = sph_radius[i - nbox];
			tags[i] = sph_tags[i - nbox];
		}
		nh_aabb_of(p, reach, lo, hi);
		mn[3*i+0] = lo.x; mn[3*i+1] = lo.y; mn[3*i+2] = lo.z;
		mx[3*i+0] = hi.x; mx[3*i+1] = hi.y; mx[3*i+2] = hi.z;
	}
	return w;
}

extern "C" {

// The broadphase's result by brute force: the collider index pairs (i < j) whose exact AABBs overlap strictly and whose bodies differ, in (i, j) order.
// Returns their number; the first `cap` are written to out_pairs (2 per).  `out_aabb` (6 per collider: min xyz, max xyz), when given, receives the AABBs.
long long hs_pairs(const Xf* body_xf, uint32_t nbox, const Xf* box_xf, const float* box_size /*4 per*/, uint32_t nsph, const Xf* sph_xf, const float* sph_radius,
                   uint64_t cap, uint32_t* out_pairs, float* out_aabb) {
	const uint32_t n = nbox + nsph;
	std::vector<uint32_t> no_tags(n, 0u);
	const Boxes w = world_boxes(body_xf, nbox, box_xf, box_size, no_tags.data(), nsph, sph_xf, sph_radius, no_tags.data());
	if (out_aabb) for (uint32_t i = 0; i < n; ++i) { memcpy(out_aabb + 6*(size_t)i, &w.mn[3*(size_t)i], 12); memcpy(out_aabb + 6*(size_t)i + 3, &w.mx[3*(size_t)i], 12); }
	uint64_t found = 0;
	for (uint32_t i = 0; i < n; ++i) for (uint32_t j = i + 1; j < n; ++j) {
		if (!w.is_pair(i, j)) continue;
		if (found < cap) { out_pairs[2*found] = i; out_pairs[2*found+1] = j; }
		++found;
	}
	return (long long)found;
}

// World transforms + AABBs + morton keys for all colliders (boxes first, then spheres).
// Returns number of contacts; outputs sorted by (key, feature).
int hs_collide(const Xf* body_xf, uint32_t nbox, const Xf* box_xf, const float* box_size /*4 per*/, const uint32_t* box_tags,
               uint32_t nsph, const Xf* sph_xf, const float* sph_radius, const uint32_t* sph_tags,
               uint32_t cap, float* out_contacts /*8 per*/, uint32_t* out_bodies /*2 per*/, uint64_t* out_keys, uint32_t* out_features) {
	uint32_t n = nbox + nsph;
	const Boxes w = world_boxes(body_xf, nbox, box_xf, box_size, box_tags, nsph, sph_xf, sph_radius, sph_tags);
	const std::vector<nh_xform>& xf = w.xf;
	const std::vector<float>& mn = w.mn;
	const std::vector<uint32_t>& tags = w.tags;
	// morton keys
	nh_f3 smin = nh_make3(mn[0], mn[1], mn[2]), smax = smin;
	for (uint32_t i = 1; i < n; ++i) {
		smin.x = nh_min(smin.x, mn[3*i]); smin.y = nh_min(smin.y, mn[3*i+1]); smin.z = nh_min(smin.z, mn[3*i+2]);
		smax.x = nh_max(smax.x, mn[3*i]); smax.y = nh_max(smax.y, mn[3*i+1]); smax.z = nh_max(smax.z, mn[3*i+2]);
	}
	float scale = nh_morton_scale(smin, smax);
	nh_f3 smin_s = nh_make3(smin.x * scale, smin.y * scale, smin.z * scale);
	std::vector<uint64_t> mk(n);
	for (uint32_t i = 0; i < n; ++i) mk[i] = nh_morton_of(nh_make3(mn[3*i], mn[3*i+1], mn[3*i+2]), scale, smin_s);

	struct Rec { uint64_t key; uint32_t feature; uint32_t seq; float c[8]; uint32_t ba, bb; };
	std::vector<Rec> recs;
	uint32_t seq = 0;
	for (uint32_t i = 0; i < n; ++i) for (uint32_t j = i + 1; j < n; ++j) {
		if (!w.is_pair(i, j)) continue;
		// the pair's "a" = later in morton order (ties: the lower index comes first), then the pair by shape: what the kernels call
		const bool i_first = nh_a_is_first(mk[i], mk[j], i, j);
		const uint32_t a = i_first ? j : i, b = i_first ? i : j;
		const bool a_sph = a >= nbox, b_sph = b >= nbox;
		const float none[3] = { 0.0f, 0.0f, 0.0f };
		nh_contact_out out[16];
		nh_bb_result r;
		r.kind = 0; r.mask = 0;
		uint64_t key = 0; uint32_t ba = 0, bb = 0;
		int cnt = nh_pair_contacts(xf[a], xf[b], a_sph ? none : box_size + 4*a, b_sph ? none : box_size + 4*b, a_sph ? sph_radius[a - nbox] : 0.0f, b_sph ? sph_radius[b - nbox] : 0.0f,
		                           tags[a], tags[b], a_sph, b_sph, r, out[0], key, ba, bb);
		if (r.kind) nh_bb_contacts(r, out);
		for (int k = 0; k < cnt; ++k) {
			Rec rc; rc.key = key; rc.feature = out[k].feature; rc.seq = seq++;
			rc.c[0] = out[k].px; rc.c[1] = out[k].py; rc.c[2] = out[k].pz; rc.c[3] = out[k].penetration;
			rc.c[4] = out[k].nx; rc.c[5] = out[k].ny; rc.c[6] = out[k].nz; rc.c[7] = out[k].friction;
			rc.ba = ba; rc.bb = bb;
			recs.push_back(rc);
		}
	}
	// reference tag order: (b_tag, a_tag, feature)
	std::stable_sort(recs.begin(), recs.end(), [](const Rec& x, const Rec& y) {
		uint64_t kx = (x.key >> 32) << 32 | (x.key & 0xffffffffu), ky = (y.key >> 32) << 32 | (y.key & 0xffffffffu);
		if (kx != ky) return kx < ky;
		return x.feature < y.feature;
	});
	uint32_t m = (uint32_t)std::min<size_t>(recs.size(), cap);
	for (uint32_t i = 0; i < m; ++i) {
		memcpy(out_contacts + 8*i, recs[i].c, 32);
		out_bodies[2*i] = recs[i].ba; out_bodies[2*i+1] = recs[i].bb;
		out_keys[i] = recs[i].key; out_features[i] = recs[i].feature;
	}
	return (int)recs.size();
}

// setup + warm start + `iterations` x apply + export, with contacts visited in the given order
// (order[i] = contact index; duplicates -- the reference's padding lanes -- are skipped).
void hs_solve(uint32_t nbodies, const Xf* body_xf, const float* props /*4 per: inertia_inverse xyz, mass_inverse*/, float* momentum /*8 per*/,
              uint32_t ncontacts, const float* contacts /*8 per*/, const uint32_t* bodies /*2 per*/, const float* cached /*4 per*/,
              uint32_t norder, const uint32_t* order, uint32_t iterations, float* out_impulses /*4 per*/) {
	std::vector<nh_row> rows(ncontacts);
	std::vector<nh_state> st(ncontacts);
	std::vector<uint32_t> seq;
	std::vector<uint8_t> seen(ncontacts, 0);
	for (uint32_t i = 0; i < norder; ++i) { uint32_t c = order[i]; if (!seen[c]) { seen[c] = 1; seq.push_back(c); } }
	for (uint32_t i = 0; i < nbodies; ++i) momentum[8*i+3] = props[4*i+3];
	auto load = [&](uint32_t b) { nh_vel v; memcpy(&v, momentum + 8*b, 32); return v; };
	auto store = [&](uint32_t b, const nh_vel& v) { memcpy(momentum + 8*b, &v, 32); };
	for (uint32_t c : seq) {
		uint32_t a = bodies[2*c], b = bodies[2*c+1];
		nh_quat qa = { body_xf[a].q[0], body_xf[a].q[1], body_xf[a].q[2], body_xf[a].q[3] };
		nh_quat qb = { body_xf[b].q[0], body_xf[b].q[1], body_xf[b].q[2], body_xf[b].q[3] };
		nh_inertia IA = nh_world_inertia(qa, props[4*a], props[4*a+1], props[4*a+2]);
		nh_inertia IB = nh_world_inertia(qb, props[4*b], props[4*b+1], props[4*b+2]);
		nh_contact_in ci; memcpy(&ci, contacts + 8*c, 32);
		nh_build_row(ci, nh_make3(body_xf[a].p[0], body_xf[a].p[1], body_xf[a].p[2]), nh_make3(body_xf[b].p[0], body_xf[b].p[1], body_xf[b].p[2]),
		             IA, IB, props[4*a+3], props[4*b+3], rows[c]);
		nh_vel va = load(a), vb = load(b);
		nh_warm_start(rows[c], cached[4*c], cached[4*c+1], cached[4*c+2], va, vb, st[c]);
		store(a, va); store(b, vb);
	}
	for (uint32_t it = 0; it < iterations; ++it)
		for (uint32_t c : seq) {
			uint32_t a = bodies[2*c], b = bodies[2*c+1];
			nh_vel va = load(a), vb = load(b);
			nh_apply_one(rows[c], st[c], va, vb);
			store(a, va); store(b, vb);
		}
	for (uint32_t c = 0; c < ncontacts; ++c) {
		if (!seen[c]) continue;
		nh_export_impulse(rows[c], st[c], out_impulses[4*c], out_impulses[4*c+1], out_impulses[4*c+2]);
	}
}

// Same solve, but contacts against body 0 go through the ONE-BODY forms (nh_row1 / nh_apply_one1 ...) the fused GPU kernel uses
// when body 0 is inert.  Returns the number of contacts that took that path (0 if body 0 is not inert).
int hs_solve_one_body(uint32_t nbodies, const Xf* body_xf, const float* props, float* momentum,
                      uint32_t ncontacts, const float* contacts, const uint32_t* bodies, const float* cached,
                      uint32_t norder, const uint32_t* order, uint32_t iterations, float* out_impulses) {
	if (!nh_is_inert(momentum, momentum + 4, props, props[3])) return 0;
	std::vector<nh_row> rows(ncontacts);
	std::vector<nh_row1> rows1(ncontacts);
	std::vector<nh_state> st(ncontacts);
	std::vector<uint32_t> seq;
	std::vector<uint8_t> seen(ncontacts, 0);
	for (uint32_t i = 0; i < norder; ++i) { uint32_t c = order[i]; if (!seen[c]) { seen[c] = 1; seq.push_back(c); } }
	for (uint32_t i = 0; i < nbodies; ++i) momentum[8*i+3] = props[4*i+3];
	auto load = [&](uint32_t b) { nh_vel v; memcpy(&v, momentum + 8*b, 32); return v; };
	auto store = [&](uint32_t b, const nh_vel& v) { memcpy(momentum + 8*b, &v, 32); };
	auto one = [&](uint32_t c) { return (bodies[2*c] == 0) != (bodies[2*c+1] == 0); };
	int taken = 0;
	for (uint32_t c : seq) {
		uint32_t a = bodies[2*c], b = bodies[2*c+1];
		nh_contact_in ci; memcpy(&ci, contacts + 8*c, 32);
		if (one(c)) {
			uint32_t d = a ? a : b;
			nh_quat qd = { body_xf[d].q[0], body_xf[d].q[1], body_xf[d].q[2], body_xf[d].q[3] };
			nh_inertia ID = nh_world_inertia(qd, props[4*d], props[4*d+1], props[4*d+2]);
			nh_build_row1(ci, nh_make3(body_xf[d].p[0], body_xf[d].p[1], body_xf[d].p[2]), ID, props[4*d+3], a != 0, rows1[c]);
			nh_vel vd = load(d);
			nh_warm_start1(rows1[c], cached[4*c], cached[4*c+1], cached[4*c+2], vd, a != 0, st[c]);
			store(d, vd);
			++taken;
			continue;
		}
		nh_quat qa = { body_xf[a].q[0], body_xf[a].q[1], body_xf[a].q[2], body_xf[a].q[3] };
		nh_quat qb = { body_xf[b].q[0], body_xf[b].q[1], body_xf[b].q[2], body_xf[b].q[3] };
		nh_inertia IA = nh_world_inertia(qa, props[4*a], props[4*a+1], props[4*a+2]);
		nh_inertia IB = nh_world_inertia(qb, props[4*b], props[4*b+1], props[4*b+2]);
		nh_build_row(ci, nh_make3(body_xf[a].p[0], body_xf[a].p[1], body_xf[a].p[2]), nh_make3(body_xf[b].p[0], body_xf[b].p[1], body_xf[b].p[2]),
		             IA, IB, props[4*a+3], props[4*b+3], rows[c]);
		nh_vel va = load(a), vb = load(b);
		nh_warm_start(rows[c], cached[4*c], cached[4*c+1], cached[4*c+2], va, vb, st[c]);
		store(a, va); store(b, vb);
	}
	for (uint32_t it = 0; it < iterations; ++it)
		for (uint32_t c : seq) {
			uint32_t a = bodies[2*c], b = bodies[2*c+1];
			if (one(c)) {
				uint32_t d = a ? a : b;
				nh_vel vd = load(d);
				nh_apply_one1(rows1[c], st[c], vd, a != 0);
				store(d, vd);
				continue;
			}
			nh_vel va = load(a), vb = load(b);
			nh_apply_one(rows[c], st[c], va, vb);
			store(a, va); store(b, vb);
		}
	for (uint32_t c = 0; c < ncontacts; ++c) {
		if (!seen[c]) continue;
		if (one(c)) nh_export_impulse1(rows1[c], st[c], out_impulses[4*c], out_impulses[4*c+1], out_impulses[4*c+2]);
		else nh_export_impulse(rows[c], st[c], out_impulses[4*c], out_impulses[4*c+1], out_impulses[4*c+2]);
	}
	// the general path zeroes unused1 of every body it touches, body 0 included (nudge.cpp:4823, 4849)
	return taken;
}

// Same solve with RADIAL rows (nh_rowr, nh_solver.h) wherever a contact qualifies (both lever arms parallel to the normal, isotropic
// inertia, or the inert static world): what the colour-scheduled GPU sweeps of the default solver order run.  Returns how many did.
int hs_solve_radial(uint32_t nbodies, const Xf* body_xf, const float* props, float* momentum,
                    uint32_t ncontacts, const float* contacts, const uint32_t* bodies, const float* cached,
                    uint32_t norder, const uint32_t* order, uint32_t iterations, float* out_impulses) {
	const bool inert0 = nh_is_inert(momentum, momentum + 4, props, props[3]);
	std::vector<nh_row> rows(ncontacts);
	std::vector<nh_rowr> rowsr(ncontacts);
	std::vector<uint8_t> radial(ncontacts, 0);
	std::vector<nh_state> st(ncontacts);
	std::vector<uint32_t> seq;
	std::vector<uint8_t> seen(ncontacts, 0);
	for (uint32_t i = 0; i < norder; ++i) { uint32_t c = order[i]; if (!seen[c]) { seen[c] = 1; seq.push_back(c); } }
	for (uint32_t i = 0; i < nbodies; ++i) momentum[8*i+3] = props[4*i+3];
	auto load = [&](uint32_t b) { nh_vel v; memcpy(&v, momentum + 8*b, 32); return v; };
	auto store = [&](uint32_t b, const nh_vel& v) { memcpy(momentum + 8*b, &v, 32); };
	int taken = 0;
	for (uint32_t c : seq) {
		uint32_t a = bodies[2*c], b = bodies[2*c+1];
		nh_contact_in ci; memcpy(&ci, contacts + 8*c, 32);
		nh_f3 pa = nh_make3(body_xf[a].p[0], body_xf[a].p[1], body_xf[a].p[2]), pb = nh_make3(body_xf[b].p[0], body_xf[b].p[1], body_xf[b].p[2]);
		const bool ia = inert0 && a == 0, ib = inert0 && b == 0;
		radial[c] = nh_side_is_radial(ci.px - pa.x, ci.py - pa.y, ci.pz - pa.z, ci.nx, ci.ny, ci.nz, props[4*a], props[4*a+1], props[4*a+2], ia) &&
		            nh_side_is_radial(ci.px - pb.x, ci.py - pb.y, ci.pz - pb.z, ci.nx, ci.ny, ci.nz, props[4*b], props[4*b+1], props[4*b+2], ib);
		nh_vel va = load(a), vb = load(b);
		if (radial[c]) {
			nh_build_rowr(ci, pa, pb, props[4*a], props[4*b], props[4*a+3], props[4*b+3], ia, ib, rowsr[c]);
			nh_warm_start_r(rowsr[c], cached[4*c], cached[4*c+1], cached[4*c+2], va, vb, st[c]);
			++taken;
		} else {
			nh_quat qa = { body_xf[a].q[0], body_xf[a].q[1], body_xf[a].q[2], body_xf[a].q[3] };
			nh_quat qb = { body_xf[b].q[0], body_xf[b].q[1], body_xf[b].q[2], body_xf[b].q[3] };
			nh_build_row(ci, pa, pb, nh_world_inertia(qa, props[4*a], props[4*a+1], props[4*a+2]), nh_world_inertia(qb, props[4*b], props[4*b+1], props[4*b+2]),
			             props[4*a+3], props[4*b+3], rows[c]);
			nh_warm_start(rows[c], cached[4*c], cached[4*c+1], cached[4*c+2], va, vb, st[c]);
		}
		store(a, va); store(b, vb);
	}
	for (uint32_t it = 0; it < iterations; ++it)
		for (uint32_t c : seq) {
			uint32_t a = bodies[2*c], b = bodies[2*c+1];
			nh_vel va = load(a), vb = load(b);
			if (radial[c]) nh_apply_radial(rowsr[c], st[c], va, vb); else nh_apply_one(rows[c], st[c], va, vb);
			store(a, va); store(b, vb);
		}
	for (uint32_t c = 0; c < ncontacts; ++c) {
		if (!seen[c]) continue;
		if (radial[c]) nh_export_impulse_r(rowsr[c], st[c], out_impulses[4*c], out_impulses[4*c+1], out_impulses[4*c+2]);
		else nh_export_impulse(rows[c], st[c], out_impulses[4*c], out_impulses[4*c+1], out_impulses[4*c+2]);
	}
	return taken;
}

void hs_advance(uint32_t nactive, const uint32_t* active, Xf* body_xf, const float* momentum, uint8_t* idle, float dt) {
	for (uint32_t n = 0; n < nactive; ++n) {
		uint32_t i = active[n];
		idle[i] = nh_advance_body(body_xf[i].p, body_xf[i].q, momentum + 8*i, momentum + 8*i + 4, idle[i], dt);
	}
}

void hs_gravity(uint32_t nactive, const uint32_t* active, float* momentum, float dt, float g, float rate) {
	float damping = 1.0f - dt * rate;
	float dv = g * dt;
	for (uint32_t n = 0; n < nactive; ++n) {
		uint32_t i = active[n];
		nh_gravity_damping(momentum + 8*i, momentum + 8*i + 4, 0.0f * dt, dv, 0.0f * dt, damping);
	}
}

}
