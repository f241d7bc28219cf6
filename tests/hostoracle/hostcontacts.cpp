// hostcontacts.cpp -- CPU build of the per-item functions of nh_contact_pairs / nh_contact_events / nh_step_contact_pairs
// (nudge_amd/csrc/nh_contact_events.h), the oracle of the GPU's flag-scan-sort-merge pipeline (tests/hostcontacts_util.py, whose numpy oracle computes
// the same with explicit loops over np.float32 scalars).
//   hc_contact_pairs       serial: the runs in list order by nh_cp_run, a std::stable_sort of the runs by (lo, hi) -- whatever body_count says about
//                          the key width --, one nh_cp_merge per group, the header's output rule
//   hc_contact_events      the two differences by nh_cp_find, serial copies
//   hc_step_contact_pairs  each contact's impulse by nh_cp_cache_find, then hc_contact_pairs
#include <algorithm>
#include "oracle.h"
#include "../../nudge_amd/csrc/nh_contact_events.h"

namespace {

struct Load {
	const nh_Contact* data; const nh_BodyPair* bodies; const nh_CachedContactImpulse* impulses; const nh_ContactPair* parts;
	nh_Contact contact(uint32_t j) const { return data[j]; }
	nh_BodyPair pair(uint32_t j) const { return bodies[j]; }
	nh_f3 impulse(uint32_t j) const { return impulses ? nh_make3(impulses[j].impulse[0], impulses[j].impulse[1], impulses[j].impulse[2]) : nh_make3(0.0f, 0.0f, 0.0f); }
	nh_ContactPair part(uint32_t r) const { nh_ContactPair p = parts[r]; return p; }
};

// *count = the true number; the records iff they all fit
void emit(const std::vector<nh_ContactPair>& records, uint32_t* count, nh_ContactPair* out, uint32_t capacity) {
	*count = (uint32_t)records.size();
	if (!out || records.size() > capacity) return;
	for (size_t k = 0; k < records.size(); ++k) out[k] = records[k];
}

void difference(const nh_ContactPair* mine, uint32_t n, const nh_ContactPair* other, uint32_t m, bool all, std::vector<nh_ContactPair>& out) {
	for (uint32_t r = 0u; r < n; ++r)
		if (all || !nh_cp_find(other, m, mine[r].lo, mine[r].hi)) out.push_back(mine[r]);
}

}

extern "C" {

void hc_contact_pairs(const nh_Contact* data, const nh_BodyPair* bodies, const nh_CachedContactImpulse* impulses, uint32_t n, uint32_t* count,
                      nh_ContactPair* out, uint32_t capacity) {
	std::vector<nh_ContactPair> parts;
	Load ld{ data, bodies, impulses, nullptr };
	for (uint32_t i = 0u; i < n;) {
		parts.push_back(nh_cp_run(ld, n, i));
		i += parts.back().count;
	}
	const uint32_t runs = (uint32_t)parts.size();
	std::vector<uint32_t> vals(runs);
	for (uint32_t r = 0u; r < runs; ++r) vals[r] = r;
	auto id = [&](uint32_t r) { return ((uint64_t)parts[r].lo << 32) | parts[r].hi; };
	std::stable_sort(vals.begin(), vals.end(), [&](uint32_t a, uint32_t b) { return id(a) < id(b); });
	std::vector<uint64_t> keys(runs);
	for (uint32_t w = 0u; w < runs; ++w) keys[w] = id(vals[w]);
	ld.parts = parts.data();
	std::vector<nh_ContactPair> records;
	for (uint32_t w = 0u; w < runs; ++w)
		if (w == 0u || keys[w] != keys[w - 1u]) records.push_back(nh_cp_merge(ld, keys.data(), vals.data(), runs, w));
	emit(records, count, out, capacity);
}

void hc_step_contact_pairs(const nh_Contact* data, const nh_BodyPair* bodies, const uint64_t* tags, const uint32_t* features, uint32_t n,
                           const uint64_t* ctags, const uint32_t* cfeatures, const nh_CachedContactImpulse* cdata, uint32_t m, uint32_t* count,
                           nh_ContactPair* out, uint32_t capacity) {
	std::vector<nh_CachedContactImpulse> impulses(n ? n : 1u);
	for (uint32_t i = 0u; i < n; ++i) {
		const uint32_t at = nh_cp_cache_find(ctags, cfeatures, m, i, tags[i], features[i]);
		impulses[i] = at == NH_CP_NONE ? nh_CachedContactImpulse{ { 0.0f, 0.0f, 0.0f }, 0.0f } : cdata[at];
	}
	hc_contact_pairs(data, bodies, impulses.data(), n, count, out, capacity);
}

// (prev_count / cur_count: the lists' device words; has_prev 0: the first frame)
void hc_contact_events(uint32_t has_prev, const nh_ContactPair* prev, uint32_t prev_count, uint32_t prev_capacity, const nh_ContactPair* cur,
                       uint32_t cur_count, uint32_t cur_capacity, uint32_t* began_count, nh_ContactPair* began, uint32_t began_capacity,
                       uint32_t* ended_count, nh_ContactPair* ended, uint32_t ended_capacity) {
	std::vector<nh_ContactPair> b, e;
	const bool present = cur_count <= cur_capacity && (!has_prev || prev_count <= prev_capacity);
	if (present) {
		difference(cur, cur_count, prev, has_prev ? prev_count : 0u, !has_prev, b);
		if (has_prev) difference(prev, prev_count, cur, cur_count, false, e);
	}
	emit(b, began_count, began, began_capacity);
	emit(e, ended_count, ended, ended_capacity);
}

uint32_t hc_bits(uint32_t body_count) { return nh_cp_bits(body_count); }

}
