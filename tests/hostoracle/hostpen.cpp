// hostpen.cpp -- CPU build of the penetration arithmetic of nudge_amd/csrc/nh_query.h, the oracle of the GPU's nh_penetration (tests/hostpen_util.py).
//   hp_penetration  offsets and 32-byte records of a batch of sphere, box and capsule queries by brute force over all colliders, with the header's exact
//                   rules: nh_overlap's validity, predicates, ignore_body, order, capacity prefix and 2^32 - 1 marker (oracle.h's overlap_all), and the
//                   pair function of each record
//   hp_pen_*        the six pair functions alone: out = normal[3], depth
//   hp_touches      nh_overlap's predicate of one query against one collider
#include "oracle.h"

static nh_QPen pen(const nh_OverlapQuery& q, const Rec& r, bool box) {
	const nh_f3 c = v3(q.center), h = v3(q.size);
	const nh_quat qr = q4(q.rotation);
	const nh_f3 p = rec_pos(r), rh = rec_half(r);
	const nh_quat rq = rec_rot(r);
	if (q.shape == NH_SHAPE_CAPSULE)
		return box ? nh_q_pen_capsule_box(c, qr, h.x, h.y, p, rq, rh) : nh_q_pen_capsule_sphere(c, qr, h.x, h.y, p, rh.x);
	const bool sphere = q.shape == NH_SHAPE_SPHERE;
	if (box) return sphere ? nh_q_pen_sphere_box(c, h.x, p, rq, rh) : nh_q_pen_box_box(c, qr, h, p, rq, rh);
	return sphere ? nh_q_pen_sphere_sphere(c, h.x, p, rh.x) : nh_q_pen_box_sphere(c, qr, h, p, rh.x);
}

extern "C" {

uint64_t hp_penetration(const Rec* rec, uint32_t n, uint32_t nbox, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets, nh_PenetrationHit* hits,
                        uint32_t capacity, uint32_t threads) {
	return overlap_all(rec, n, nbox, queries, count, offsets, hits, capacity, threads, true, [=](nh_PenetrationHit& w, const nh_OverlapQuery& q, uint32_t c) {
		const nh_QPen o = pen(q, rec[c], c < nbox);
		w.normal[0] = o.n.x; w.normal[1] = o.n.y; w.normal[2] = o.n.z; w.depth = o.depth;
		write_who(w, rec, nbox, c);
	});
}

// one query against one collider record: nh_overlap's predicate (validity included), and the pair function
int hp_touches(const nh_OverlapQuery* q, const Rec* r, int box) { return valid(*q) && touches(*q, *r, box != 0) ? 1 : 0; }
void hp_pen(const nh_OverlapQuery* q, const Rec* r, int box, float out[4]) { out4(pen(*q, *r, box != 0), out); }

// the same two over `count` pairs (query i against record i; box[i] != 0: a box collider): ok[i] = the predicate, out[4 i ..] = normal, depth
void hp_pairs(const nh_OverlapQuery* q, const Rec* r, const uint8_t* box, uint32_t count, uint8_t* ok, float* out) {
	for (uint32_t i = 0; i < count; ++i) {
		ok[i] = valid(q[i]) && touches(q[i], r[i], box[i] != 0) ? 1 : 0;
		out4(pen(q[i], r[i], box[i] != 0), out + 4 * i);
	}
}

void hp_pen_sphere_sphere(const float c[3], float r, const float p[3], float R, float out[4]) { out4(nh_q_pen_sphere_sphere(v3(c), r, v3(p), R), out); }
void hp_pen_sphere_box(const float c[3], float r, const float p[3], const float q[4], const float h[3], float out[4]) {
	out4(nh_q_pen_sphere_box(v3(c), r, v3(p), q4(q), v3(h)), out);
}
void hp_pen_box_sphere(const float ca[3], const float qa[4], const float ha[3], const float p[3], float R, float out[4]) {
	out4(nh_q_pen_box_sphere(v3(ca), q4(qa), v3(ha), v3(p), R), out);
}
void hp_pen_capsule_sphere(const float c[3], const float q[4], float r, float hh, const float p[3], float R, float out[4]) {
	out4(nh_q_pen_capsule_sphere(v3(c), q4(q), r, hh, v3(p), R), out);
}
void hp_pen_box_box(const float ca[3], const float qa[4], const float ha[3], const float cb[3], const float qb[4], const float hb[3], float out[4]) {
	out4(nh_q_pen_box_box(v3(ca), q4(qa), v3(ha), v3(cb), q4(qb), v3(hb)), out);
}
void hp_pen_capsule_box(const float c[3], const float q[4], float r, float hh, const float p[3], const float qb[4], const float hb[3], float out[4]) {
	out4(nh_q_pen_capsule_box(v3(c), q4(q), r, hh, v3(p), q4(qb), v3(hb)), out);
}

// nh_q_point_box's signed distance of a point (the exactness test of sphere / box)
float hp_point_box_distance(const float x[3], const float p[3], const float q[4], const float h[3]) { return nh_q_point_box(v3(x), v3(p), q4(q), v3(h)).d; }

}
