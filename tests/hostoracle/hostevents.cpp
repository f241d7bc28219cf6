// hostevents.cpp -- CPU build of the per-record functions of nh_overlap_bodies / nh_overlap_events (nudge_amd/csrc/nh_query.h, "events"), the oracle of
// the GPU's record-parallel set difference (tests/hostevents_util.py, whose numpy oracle computes the same per volume with sets).
//   he_events    flags as the device's lanes set them -- a record's segment by nh_q_seg_of_present, its identity in the other list's segment by
//                nh_q_ident_find -- then a serial scan and copy under nh_overlap's offsets and capacity rules
//   he_bodies    per present segment a stable sort by body; the first record of each run
//   he_seg_of / he_seg_present / he_ident_find    the functions alone
#include <algorithm>
#include "oracle.h"

namespace {

struct List { const uint32_t* offsets; const uint32_t* hits; uint32_t capacity; };

// The output of one list under nh_overlap's rules: `counts` per volume -> offsets; record k of volume i is hits[src(i, k)], written iff the volume's
// segment ends at or below `capacity`.
template <class Src> void emit(uint32_t count, const std::vector<uint32_t>& counts, const List& from, Src src, uint32_t* offsets, uint32_t* hits, uint32_t capacity) {
	uint32_t at = 0u;
	for (uint32_t i = 0u; i < count; ++i) {
		offsets[i] = at;
		const uint32_t end = at + counts[i];
		if (hits && end <= capacity)
			for (uint32_t k = 0u; k < counts[i]; ++k)
				for (int w = 0; w < 4; ++w) hits[4u * (size_t)(at + k) + w] = from.hits[4u * (size_t)src(i, k) + w];
		at = end;
	}
	offsets[count] = at;
}

// Per volume the records of `mine` whose identity is not in `other`'s segment (other == nullptr: every record of a present segment)
void difference(uint32_t count, const List& mine, const List* other, uint32_t by_body, uint32_t* offsets, uint32_t* hits, uint32_t capacity) {
	std::vector<uint32_t> counts(count, 0u);
	std::vector<std::vector<uint32_t>> kept(count);
	for (uint32_t r = 0u; r < mine.capacity; ++r) {
		const uint32_t i = nh_q_seg_of_present(mine.offsets, count, mine.capacity, r);
		if (i == 0xffffffffu) continue;
		if (other) {
			if (!nh_q_seg_present(other->offsets, count, other->capacity, i)) continue;
			if (nh_q_ident_find(other->hits, other->offsets[i], other->offsets[i + 1u], nh_q_ident(mine.hits + 4u * (size_t)r, by_body), by_body)) continue;
		}
		kept[i].push_back(r);
		++counts[i];
	}
	emit(count, counts, mine, [&](uint32_t i, uint32_t k) { return kept[i][k]; }, offsets, hits, capacity);
}

}

extern "C" {

void he_events(uint32_t count, const uint32_t* prev_offsets, const uint32_t* prev_hits, uint32_t prev_capacity, const uint32_t* cur_offsets,
               const uint32_t* cur_hits, uint32_t cur_capacity, uint32_t by_body, uint32_t* entered_offsets, uint32_t* entered_hits, uint32_t entered_capacity,
               uint32_t* left_offsets, uint32_t* left_hits, uint32_t left_capacity) {
	const List cur{ cur_offsets, cur_hits, cur_capacity }, prev{ prev_offsets, prev_hits, prev_capacity };
	difference(count, cur, prev_offsets ? &prev : nullptr, by_body, entered_offsets, entered_hits, entered_capacity);
	if (prev_offsets) difference(count, prev, &cur, by_body, left_offsets, left_hits, left_capacity);
	else for (uint32_t i = 0u; i <= count; ++i) left_offsets[i] = 0u;
}

void he_bodies(uint32_t count, const uint32_t* in_offsets, const uint32_t* in_hits, uint32_t in_capacity, uint32_t* out_offsets, uint32_t* out_hits,
               uint32_t out_capacity) {
	const List in{ in_offsets, in_hits, in_capacity };
	std::vector<uint32_t> counts(count, 0u);
	std::vector<std::vector<uint32_t>> kept(count);
	for (uint32_t i = 0u; i < count; ++i) {
		if (!nh_q_seg_present(in_offsets, count, in_capacity, i)) continue;
		std::vector<uint32_t> order;
		for (uint32_t r = in_offsets[i]; r < in_offsets[i + 1u]; ++r) order.push_back(r);
		std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return in_hits[4u * (size_t)a] < in_hits[4u * (size_t)b]; });
		for (size_t k = 0; k < order.size(); ++k)
			if (k == 0 || in_hits[4u * (size_t)order[k]] != in_hits[4u * (size_t)order[k - 1]]) kept[i].push_back(order[k]);
		counts[i] = (uint32_t)kept[i].size();
	}
	emit(count, counts, in, [&](uint32_t i, uint32_t k) { return kept[i][k]; }, out_offsets, out_hits, out_capacity);
}

uint32_t he_seg_of(const uint32_t* offsets, uint32_t count, uint32_t r) { return nh_q_seg_of(offsets, count, r); }

int he_seg_present(const uint32_t* offsets, uint32_t count, uint32_t capacity, uint32_t i) { return nh_q_seg_present(offsets, count, capacity, i) ? 1 : 0; }

int he_ident_find(const uint32_t* hits, uint32_t lo, uint32_t hi, const uint32_t* record, uint32_t by_body) {
	return nh_q_ident_find(hits, lo, hi, nh_q_ident(record, by_body), by_body) ? 1 : 0;
}

}
