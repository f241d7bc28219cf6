// hostsweep.cpp -- CPU build of the fast-body calls of include/nudge_hip.h (nh_sweep, nh_sweep_limit), the oracle of the GPU's kernels
// (tests/hostsweep_util.py).
//   hs_sweep        selection, records and hits: nudge_amd/csrc/nh_query.h's nh_q_sweep_travel / _far / _core -- the arithmetic the device runs -- over
//                   every collider in index order; the hit of each selected one by oracle.h's closest_hit over SweptBox / SweptSphere -- the brute force
//                   nh_boxcast's and nh_spherecast's oracle is -- under layer words and a mask per COLLIDER; the all-or-none capacity rule
//   hs_sweep_limit  the factor of every entry's body -- the least t over the body's entries with a real hit and t > 0 -- and the momentum array with the
//                   velocity of every limited body scaled once
// The body transforms and momentum are plain arrays of nh_Transform / nh_BodyMomentum.
#include "oracle.h"

namespace {

struct Cast { nh_BoxCast record; bool selected; };

Cast cast_of(const Rec& r, bool box, const nh_Transform* transforms, const nh_BodyMomentum* momentum, uint32_t nbodies, float time_step, float min_travel, float core) {
	Cast k;
	k.selected = nh_q_sweep_body(r.body, nbodies);
	nh_f3 d = nh_make3(0.0f, 0.0f, 0.0f);
	if (k.selected) {
		d = nh_q_sweep_travel(rec_pos(r), v3(transforms[r.body].position), v3(momentum[r.body].velocity), v3(momentum[r.body].angular_velocity), time_step);
		k.selected = nh_q_sweep_far(d, rec_half(r), box, min_travel);
	}
	const nh_f3 s = nh_q_sweep_core(rec_half(r), box, core);
	nh_BoxCast& c = k.record;
	c.origin[0] = r.p[0]; c.origin[1] = r.p[1]; c.origin[2] = r.p[2]; c.max_t = 1.0f;
	c.direction[0] = d.x; c.direction[1] = d.y; c.direction[2] = d.z; c.ignore_body = r.body;
	for (int j = 0; j < 4; ++j) c.rotation[j] = box ? r.q[j] : (j == 3 ? 1.0f : 0.0f);
	c.size[0] = s.x; c.size[1] = s.y; c.size[2] = s.z; c.reserved = 0u;
	return k;
}

}

extern "C" {

// filter == 0: no mask is read.  Otherwise collider c, as a query, sees collider k iff (words[k] & m) != 0, m = masks[c] (masks null: `mask`); words
// null: all ones.  counts: two words, always written.  colliders / casts / hits: `capacity` records or null, written iff the total fits.
void hs_sweep(const Rec* rec, uint32_t n, uint32_t nbox, const nh_Transform* transforms, const nh_BodyMomentum* momentum, uint32_t nbodies,
              float time_step, float min_travel, float core, uint32_t filter, const uint32_t* words, const uint32_t* masks, uint32_t mask,
              uint32_t* counts, uint32_t* colliders, nh_BoxCast* casts, nh_RayHit* hits, uint32_t capacity, uint32_t threads) {
	std::vector<uint32_t> ones;
	if (filter && !words) { ones.assign(n, 0xffffffffu); words = ones.data(); }
	if (!filter) words = nullptr;
	std::vector<uint32_t> list;
	counts[0] = counts[1] = 0u;
	for (uint32_t c = 0; c < n; ++c)
		if (cast_of(rec[c], c < nbox, transforms, momentum, nbodies, time_step, min_travel, core).selected) { list.push_back(c); ++counts[c < nbox ? 0 : 1]; }
	if (list.size() > capacity) return;
	const uint32_t* entries = list.data();
	parallel((uint32_t)list.size(), threads, [=](uint32_t i) {
		const uint32_t c = entries[i];
		const bool box = c < nbox;
		const nh_BoxCast k = cast_of(rec[c], box, transforms, momentum, nbodies, time_step, min_travel, core).record;
		if (colliders) colliders[i] = c;
		if (casts) casts[i] = k;
		if (!hits) return;
		float bt; uint32_t bc; nh_f3 bn;
		const uint32_t m = masks ? masks[c] : mask;
		const bool ok = box ? closest_hit(rec, n, nbox, SweptBox{ q4(k.rotation), v3(k.size) }, v3(k.origin), v3(k.direction), k.max_t, k.ignore_body, words, m, -1, bt, bc, bn)
		                    : closest_hit(rec, n, nbox, SweptSphere{ k.size[0] }, v3(k.origin), v3(k.direction), k.max_t, k.ignore_body, words, m, -1, bt, bc, bn);
		write_cast(hits[i], rec, nbox, ok, k.max_t, bt, bc, bn);
	});
}

// momentum: nbodies records, changed in place.  factors: `capacity` floats or null; the first counts[0] + counts[1] are written.
void hs_sweep_limit(const Rec* rec, uint32_t n, const uint32_t* counts, const uint32_t* colliders, const nh_RayHit* hits, uint32_t capacity,
                    nh_BodyMomentum* momentum, uint32_t nbodies, float* factors) {
	const uint64_t total = (uint64_t)counts[0] + counts[1];
	if (total > capacity) return;
	std::vector<float> f(nbodies, 1.0f);
	auto body_of = [&](uint32_t i) { const uint32_t c = colliders[i]; return c < n && rec[c].body < nbodies ? rec[c].body : 0xffffffffu; };
	for (uint32_t i = 0; i < total; ++i) {
		const uint32_t b = body_of(i);
		if (b != 0xffffffffu && nh_q_sweep_limits(hits[i].shape, hits[i].t) && hits[i].t < f[b]) f[b] = hits[i].t;
	}
	std::vector<bool> done(nbodies, false);
	for (uint32_t i = 0; i < total; ++i) {
		const uint32_t b = body_of(i);
		if (factors) factors[i] = b != 0xffffffffu ? f[b] : 1.0f;
		if (b == 0xffffffffu || done[b] || !(f[b] < 1.0f)) continue;
		done[b] = true;
		for (int k = 0; k < 3; ++k) momentum[b].velocity[k] *= f[b];
	}
}

}
