// hostboxcast.cpp -- CPU build of the box-cast arithmetic of nudge_amd/csrc/nh_query.h, the oracle of the GPU's nh_boxcast (tests/hostboxcast_util.py).
//   hb_boxcast     closest hit (or the hit of one collider) by brute force over all colliders (oracle.h's closest_hit of a SweptBox), with the header's exact
//                  rules -- invalid casts, size 0 as a ray, ignore_body, ties, the reach rule for a nonzero size (the leaf box rebuilt as the build stores
//                  it) -- on several threads
//   hb_*           the single-collider predicates alone
#include "oracle.h"

extern "C" {

// only >= 0: the answer of that one collider (combined index) alone, as the closest-hit rule would give it
void hb_boxcast(const Rec* rec, uint32_t n, uint32_t nbox, const nh_BoxCast* casts, uint32_t count, nh_RayHit* hits, int64_t only, uint32_t threads) {
	parallel(count, threads, [=](uint32_t i) {
		const nh_BoxCast& cc = casts[i];
		float bt; uint32_t bc; nh_f3 bn;
		const bool ok = closest_hit(rec, n, nbox, SweptBox{ q4(cc.rotation), v3(cc.size) }, v3(cc.origin), v3(cc.direction), cc.max_t, cc.ignore_body, nullptr, 0u, only, bt, bc, bn);
		write_cast(hits[i], rec, nbox, ok, cc.max_t, bt, bc, bn);
	});
}

// one collider alone, the predicate without the reach rule (the geometry tests): out = t, normal[3], hit (1.0 / 0.0)
void hb_sweep_box_box(const float o[3], const float d[3], const float qa[4], const float ha[3], const float p[3], const float qb[4], const float hb[3], float out[5]) {
	out5(nh_q_sweep_box_box(v3(o), v3(d), q4(qa), v3(ha), v3(p), q4(qb), v3(hb)), out);
}

void hb_sweep_box_sphere(const float o[3], const float d[3], const float qa[4], const float ha[3], const float c[3], float R, float out[5]) {
	out5(nh_q_sweep_box_sphere(v3(o), v3(d), q4(qa), v3(ha), v3(c), R), out);
}

}
