// nh_contact_events.h -- per-item logic of the contact events (include/nudge_hip.h, "contact events"; nh_contact_events.hip): a contact's unordered body
// pair and its sort key, the walk of one RUN of the contact list, the merge of one pair's runs, the search of a pair list, the search of the contact
// cache.  Every function is `NH_HD`, as nh_query.h's are, so that tests/hostoracle/hostcontacts.cpp builds the SAME arithmetic with g++ -ffp-contract=off
// and gets the device's bits; what the oracle judges is everything around them -- flags, scans, the sort, the compaction, the output rules.
//
// The functions read their arrays through a LOADER (contact(i), pair(i), impulse(i), part(r)): the device's issues 16-byte loads, the oracle's reads structs.
//
// The rules (the header states them for callers):
//   pair      lo = min(a, b), hi = max(a, b); a contact is FLIPPED when its a is not lo, and then contributes its impulse and its normal with the sign
//             bit inverted (nh_neg: exact, NaNs included).
//   run       a maximal stretch of consecutive contacts with the same (lo, hi).  Its four sums start at +0 and take the contacts left to right in fp32;
//             a contact's normal impulse is (ix * nx + iy * ny) + iz * nz, of the unflipped or the flipped vectors alike.
//   pair sum  starts at +0 and takes the runs' sums in list order.  (A run's sum is never -0, so a pair of one run has its run's bits.)
//   deepest   over the pair's contacts in list order: start with the first, replace iff penetration > best.  A NaN never replaces; a NaN that comes
//             first is never replaced.  By runs: a run's candidate is its first contact, replaced iff penetration > best or best is a NaN and the
//             contact's is none -- the run's lowest-index maximum over its numbers, or its first contact where it has none -- and NH_CP_NAN_FIRST in
//             the partial record's `deepest` says that the run's FIRST contact is a NaN.  The pair takes its first run's candidate, or with that flag
//             the first contact itself, and replaces iff a later run's candidate is greater.  Same answer as the flat rule: a number first is
//             replaced by exactly the greater numbers, in index order, and a NaN first by nothing.
#ifndef NH_CONTACT_EVENTS_H
#define NH_CONTACT_EVENTS_H

#include "nh_math.h"
#include "../../include/nudge_hip.h"

#define NH_CP_NAN_FIRST 0x80000000u          // in a PARTIAL record's `deepest` (contact indices are below 2^31: the capacity rule)
#define NH_CP_NONE 0xFFFFFFFFu

NH_HD bool nh_cp_isnan(float x) { return (nh_asuint(x) & 0x7fffffffu) > 0x7f800000u; }

// bits of one body index in the sort key: those of body_count - 1, at least one; body_count = 0: unknown, all 32
NH_HD uint32_t nh_cp_bits(uint32_t body_count) {
	if (body_count == 0u) return 32u;
	uint32_t b = 1u;
	while (b < 32u && ((body_count - 1u) >> b)) ++b;
	return b;
}
// ... and the radix sort's end bit for two of them: whole 8-bit digits
NH_HD int nh_cp_sort_bits(uint32_t bits) { return (int)((2u * bits + 7u) / 8u * 8u); }

// the identity of a contact's pair, lo << 32 | hi, and the sort key lo << bits | hi (ascending key = ascending (lo, hi) while every index is below 2^bits)
NH_HD uint64_t nh_cp_pair(nh_BodyPair p) { return p.a <= p.b ? ((uint64_t)p.a << 32) | p.b : ((uint64_t)p.b << 32) | p.a; }
NH_HD bool nh_cp_flipped(nh_BodyPair p) { return p.a > p.b; }
NH_HD uint64_t nh_cp_key(uint64_t pair, uint32_t bits) { return bits >= 32u ? pair : ((pair >> 32) << bits) | (uint64_t)(uint32_t)pair; }

NH_HD void nh_cp_set_deepest(nh_ContactPair& r, const nh_Contact& c, bool flip, uint32_t index) {
	r.position[0] = c.position[0]; r.position[1] = c.position[1]; r.position[2] = c.position[2];
	r.penetration = c.penetration;
	r.normal[0] = flip ? nh_neg(c.normal[0]) : c.normal[0];
	r.normal[1] = flip ? nh_neg(c.normal[1]) : c.normal[1];
	r.normal[2] = flip ? nh_neg(c.normal[2]) : c.normal[2];
	r.deepest = index;
}

// The partial record of the run that STARTS at contact i of a list of n (i is a run head: i == 0 or pair(i - 1) differs).
template <class Load>
NH_HD nh_ContactPair nh_cp_run(const Load& ld, uint32_t n, uint32_t i) {
	nh_BodyPair p = ld.pair(i);
	const uint64_t id = nh_cp_pair(p);
	nh_ContactPair r;
	r.lo = (uint32_t)(id >> 32); r.hi = (uint32_t)id; r.first = i;
	float sx = 0.0f, sy = 0.0f, sz = 0.0f, sn = 0.0f;
	bool nan_first = false;
	uint32_t j = i;
	for (;;) {
		const nh_Contact c = ld.contact(j);
		const nh_f3 v = ld.impulse(j);
		const bool flip = nh_cp_flipped(p);
		const float d = (v.x * c.normal[0] + v.y * c.normal[1]) + v.z * c.normal[2];
		sx = sx + (flip ? nh_neg(v.x) : v.x);
		sy = sy + (flip ? nh_neg(v.y) : v.y);
		sz = sz + (flip ? nh_neg(v.z) : v.z);
		sn = sn + d;
		if (j == i) { nan_first = nh_cp_isnan(c.penetration); nh_cp_set_deepest(r, c, flip, j); }
		else if (c.penetration > r.penetration || (nh_cp_isnan(r.penetration) && !nh_cp_isnan(c.penetration))) nh_cp_set_deepest(r, c, flip, j);
		if (++j >= n) break;
		p = ld.pair(j);
		if (nh_cp_pair(p) != id) break;
	}
	r.count = j - i;
	r.impulse[0] = sx; r.impulse[1] = sy; r.impulse[2] = sz; r.normal_impulse = sn;
	if (nan_first) r.deepest |= NH_CP_NAN_FIRST;
	return r;
}

// The record of the pair whose runs are the sorted positions w, w + 1, ... with the key of w (w is a pair head: w == 0 or keys[w - 1] differs); the
// stable sort left them in list order.
template <class Load>
NH_HD nh_ContactPair nh_cp_merge(const Load& ld, const uint64_t* keys, const uint32_t* vals, uint32_t runs, uint32_t w) {
	const uint64_t key = keys[w];
	nh_ContactPair o = ld.part(vals[w]);
	if (o.deepest & NH_CP_NAN_FIRST) {          // the pair's first contact is a NaN: it stays, whatever its run's candidate is
		const uint32_t i = o.first;
		nh_cp_set_deepest(o, ld.contact(i), nh_cp_flipped(ld.pair(i)), i);
	}
	float sx = 0.0f + o.impulse[0], sy = 0.0f + o.impulse[1], sz = 0.0f + o.impulse[2], sn = 0.0f + o.normal_impulse;
	for (uint32_t u = w + 1u; u < runs && keys[u] == key; ++u) {
		const nh_ContactPair q = ld.part(vals[u]);
		sx = sx + q.impulse[0]; sy = sy + q.impulse[1]; sz = sz + q.impulse[2]; sn = sn + q.normal_impulse;
		o.count += q.count;
		if (q.penetration > o.penetration) {
			o.position[0] = q.position[0]; o.position[1] = q.position[1]; o.position[2] = q.position[2];
			o.penetration = q.penetration;
			o.normal[0] = q.normal[0]; o.normal[1] = q.normal[1]; o.normal[2] = q.normal[2];
			o.deepest = q.deepest & ~NH_CP_NAN_FIRST;
		}
	}
	o.impulse[0] = sx; o.impulse[1] = sy; o.impulse[2] = sz; o.normal_impulse = sn;
	return o;
}

// Is (lo, hi) a key of the first n records of a pair list (unique ascending keys)?
NH_HD bool nh_cp_find(const nh_ContactPair* pairs, uint32_t n, uint32_t lo, uint32_t hi) {
	uint32_t a = 0u, b = n;
	while (a < b) {
		const uint32_t mid = a + ((b - a) >> 1);
		const uint32_t ml = pairs[mid].lo, mh = pairs[mid].hi;
		if (ml < lo || (ml == lo && mh < hi)) a = mid + 1u; else b = mid;
	}
	return a < n && pairs[a].lo == lo && pairs[a].hi == hi;
}

// The cache entry of contact i with (tag, feature), or NH_CP_NONE: k_cache_lookup's search (nh_cache.hip) -- the entry at the contact's own index
// first, where a cache that is last step's contact list has it, then the lower bound in (tag, feature) order over the m entries.
NH_HD uint32_t nh_cp_cache_find(const uint64_t* ctags, const uint32_t* cfeatures, uint32_t m, uint32_t i, uint64_t t, uint32_t f) {
	if (i < m && ctags[i] == t && cfeatures[i] == f) return i;
	uint32_t a = 0u, b = m;
	while (a < b) {
		const uint32_t mid = a + ((b - a) >> 1);
		const uint64_t mt = ctags[mid];
		if (mt < t || (mt == t && cfeatures[mid] < f)) a = mid + 1u; else b = mid;
	}
	return (a < m && ctags[a] == t && cfeatures[a] == f) ? a : NH_CP_NONE;
}

#endif
