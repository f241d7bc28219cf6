// hostregion.cpp -- CPU build of the region predicates of nudge_amd/csrc/nh_query.h, the oracle of the GPU's nh_region (tests/hostregion_util.py).
//   hq_region        offsets and records of a batch of regions by brute force over all colliders, with the header's exact semantics (validity, ignore_body,
//                    the capacity prefix, the 2^32 - 1 marker, the true total), on several threads.  No tree, no entry nodes, no node test: those are what
//                    it judges
//   hq_region_keeps  one plane against `count` colliders (plane k against collider k): the per-plane predicates alone
//   hq_region_valid  a region's validity
//   hq_region_node_outside  the kernel's node test of one box against one plane (for the conservativeness test)
#include "oracle.h"

static_assert(sizeof(nh_Region) == 144, "nh_Region is 144 bytes");

static inline bool inside(const nh_Region& g, const Rec& r, bool box) {
	return nh_q_region_keeps(&g.planes[0][0], g.plane_count, rec_pos(r), rec_rot(r), rec_half(r), box);
}

extern "C" {

uint64_t hq_region(const Rec* rec, uint32_t n, uint32_t nbox, const nh_Region* regions, uint32_t count, uint32_t* offsets, nh_OverlapHit* hits,
                   uint32_t capacity, uint32_t threads) {
	std::vector<uint32_t> cnt(count);
	parallel(count, threads, [&](uint32_t i) {
		const nh_Region& g = regions[i];
		uint32_t k = 0;
		if (nh_q_region_valid(&g.planes[0][0], g.plane_count))
			for (uint32_t c = 0; c < n; ++c) if (rec[c].body != g.ignore_body && inside(g, rec[c], c < nbox)) ++k;
		cnt[i] = k;
	});
	uint64_t total = 0;
	uint32_t run = 0;
	for (uint32_t i = 0; i < count; ++i) { offsets[i] = run; run += cnt[i]; total += cnt[i]; }
	offsets[count] = run;
	if (total >= 0xffffffffull) { offsets[count] = 0xffffffffu; return total; }
	if (!hits || !capacity) return total;
	parallel(count, threads, [&](uint32_t i) {
		if (offsets[i + 1] > capacity || !cnt[i]) return;
		const nh_Region& g = regions[i];
		uint32_t k = offsets[i];
		for (uint32_t c = 0; c < n; ++c) if (rec[c].body != g.ignore_body && inside(g, rec[c], c < nbox)) write_who(hits[k++], rec, nbox, c);
	});
	return total;
}

// out[k] = does plane k (4 floats) keep collider k (position, rotation, half extents | radius in h[0])?
void hq_region_keeps(uint32_t count, const float* planes, const float* p, const float* q, const float* h, int box, uint8_t* out) {
	for (uint32_t k = 0; k < count; ++k) {
		const nh_f3 n = v3(planes + 4 * k);
		const float d = planes[4 * k + 3];
		out[k] = box ? nh_q_region_keeps_box(n, d, v3(p + 3 * k), nh_matrix(q4(q + 4 * k)), v3(h + 3 * k)) : nh_q_region_keeps_sphere(n, d, v3(p + 3 * k), h[3 * k]);
	}
}

int hq_region_valid(const nh_Region* g) { return nh_q_region_valid(&g->planes[0][0], g->plane_count) ? 1 : 0; }

int hq_region_node_outside(const float plane[4], const float lo[3], const float hi[3]) {
	return nh_q_region_node_outside(v3(plane), plane[3], v3(lo), v3(hi)) ? 1 : 0;
}

// the leaf box of a collider as the build stores it (nh_q_leaf_box: the world AABB padded by nh_q_pad)
void hq_region_leaf_box(const float p[3], const float q[4], const float h[3], int box, float lo[3], float hi[3]) {
	nh_f3 l, u;
	nh_q_leaf_box(v3(p), q4(q), v3(h), box != 0, l, u);
	lo[0] = l.x; lo[1] = l.y; lo[2] = l.z; hi[0] = u.x; hi[1] = u.y; hi[2] = u.z;
}

}
