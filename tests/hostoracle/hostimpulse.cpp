// hostimpulse.cpp -- CPU build of the per-item functions of nh_impulse_sums / nh_body_impulses / nh_blast_impulses / nh_touch_impulses
// (nudge_amd/csrc/nh_impulse.h), the oracle of the GPU's flag-scan-sort-merge pipeline (tests/hostimpulse_util.py, whose numpy oracle computes the same
// with explicit loops over np.float32 scalars).
//   hi_impulse_sums    serial: the runs in list order by nh_bi_run, a std::stable_sort of the runs by body -- whatever the body count says about the key
//                      width --, one nh_bi_merge per group, the header's output rule
//   hi_body_impulses   the same sums, then nh_bi_apply on copies of the momentum and idle arrays
//   hi_blast_impulses  per record of the list nh_bi_segment and nh_bi_blast
//   hi_touch_impulses  per slot nh_bi_touch, or the NO_BODY record for a slot at or behind counts[i]
#include <algorithm>
#include <string.h>
#include "oracle.h"
#include "../../nudge_amd/csrc/nh_impulse.h"

namespace {

struct Load {
	const nh_BodyImpulse* records; const nh_Transform* transforms; const nh_ImpulseSum* parts;
	uint32_t body(uint32_t i) const { return records[i].body; }
	nh_BodyImpulse record(uint32_t i) const { return records[i]; }
	nh_f3 position(uint32_t b) const { return v3(transforms[b].position); }
	nh_ImpulseSum part(uint32_t r) const { return parts[r]; }
};

// the sums of the first n records, ascending by body
std::vector<nh_ImpulseSum> sums_of(const nh_Transform* transforms, uint32_t body_count, const nh_BodyImpulse* records, uint32_t n) {
	std::vector<nh_ImpulseSum> parts;
	Load ld{ records, transforms, nullptr };
	for (uint32_t i = 0u; i < n;) {
		if (!nh_bi_run_head(ld, body_count, i)) { ++i; continue; }
		parts.push_back(nh_bi_run(ld, n, i));
		i += parts.back().count;
	}
	const uint32_t runs = (uint32_t)parts.size();
	std::vector<uint32_t> vals(runs);
	for (uint32_t r = 0u; r < runs; ++r) vals[r] = r;
	std::stable_sort(vals.begin(), vals.end(), [&](uint32_t a, uint32_t b) { return parts[a].body < parts[b].body; });
	std::vector<uint64_t> keys(runs);
	for (uint32_t w = 0u; w < runs; ++w) keys[w] = parts[vals[w]].body;
	ld.parts = parts.data();
	std::vector<nh_ImpulseSum> out;
	for (uint32_t w = 0u; w < runs; ++w)
		if (w == 0u || keys[w] != keys[w - 1u]) out.push_back(nh_bi_merge(ld, keys.data(), vals.data(), runs, w));
	return out;
}

uint32_t clamped(uint32_t count, uint32_t capacity) { return count < capacity ? count : capacity; }

}

extern "C" {

// (count: the list's device word, clamped to capacity here)  *out_count = the true number; the records iff they all fit
void hi_impulse_sums(const nh_Transform* transforms, uint32_t body_count, const nh_BodyImpulse* records, uint32_t count, uint32_t capacity,
                     uint32_t* out_count, nh_ImpulseSum* out, uint32_t out_capacity) {
	const std::vector<nh_ImpulseSum> sums = sums_of(transforms, body_count, records, clamped(count, capacity));
	*out_count = (uint32_t)sums.size();
	if (!out || sums.size() > out_capacity) return;
	for (size_t k = 0; k < sums.size(); ++k) out[k] = sums[k];
}

// momentum and idle are changed IN PLACE (the caller passes copies); the momentum words are moved as bytes, so unused0 / unused1 keep their bits
void hi_body_impulses(const nh_Transform* transforms, const nh_BodyProperties* properties, nh_BodyMomentum* momentum, uint8_t* idle, uint32_t body_count,
                      const nh_BodyImpulse* records, uint32_t count, uint32_t capacity, uint32_t wake) {
	for (const nh_ImpulseSum& s : sums_of(transforms, body_count, records, clamped(count, capacity))) {
		float m[8];
		memcpy(m, momentum + s.body, sizeof(m));
		nh_bi_apply(m, m + 4, transforms[s.body].rotation, properties[s.body], s);
		memcpy(momentum + s.body, m, sizeof(m));
		if (wake) idle[s.body] = 0u;
	}
}

void hi_blast_impulses(const nh_Transform* transforms, uint32_t body_count, const nh_Blast* blasts, uint32_t count, const uint32_t* offsets,
                       const nh_OverlapHit* hits, uint32_t capacity, nh_BodyImpulse* out) {
	if (count == 0u) return;
	Load ld{ nullptr, transforms, nullptr };
	const uint32_t n = clamped(offsets[count], capacity);
	for (uint32_t j = 0u; j < n; ++j) out[j] = nh_bi_blast(ld, blasts[nh_bi_segment(offsets, count, j)], hits[j].body, body_count);
}

void hi_touch_impulses(const nh_Push* pushes, uint32_t count, uint32_t k, const uint32_t* counts, const nh_Touch* touches, nh_BodyImpulse* out) {
	for (uint32_t i = 0u; i < count; ++i)
		for (uint32_t j = 0u; j < k; ++j) {
			const size_t w = (size_t)i * k + j;
			out[w] = j < clamped(counts[i], k) ? nh_bi_touch(pushes[i], touches[w]) : nh_bi_nobody();
		}
}

uint32_t hi_key_bytes(uint32_t body_count) { return (uint32_t)nh_bi_sort_bits(nh_bi_bits(body_count)) / 8u; }

}
