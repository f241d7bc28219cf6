
// nh_query.hip -- scene queries against the tree of the last nh_query_build or nh_query_refit (nh_query_build.hip, nh_query_tree.h): nh_raycast (batched
// closest-hit / any-hit ray casts), nh_spherecast, nh_boxcast and nh_capsulecast (the same for swept balls, oriented boxes and capsules), their all-hits
// (_all) and first-k (_k) forms, nh_closest / nh_closest_k / nh_distance (the nearest colliders to a point or a shape) and nh_overlap / nh_penetration (the
// colliders touching each of a batch of spheres, boxes or capsules, as variable-length segments) and nh_move (collide-and-slide: the capsule cast in a loop) and nh_recover
// (shapes pushed out of what they overlap: the overlap walk in a loop, the penetration functions at its leaves).
// nh_sweep / nh_sweep_limit ("fast bodies": the colliders that travel far, swept along their own velocity through the closest-hit casts' body, and their bodies stopped at the hit).
// nh_region (the colliders inside each of a batch of convex regions, through nh_overlap's chain) does not walk: it sweeps the leaves below the tree's entry nodes.
// nh_overlap_wide / nh_penetration_wide (nh_overlap's and nh_penetration's bytes for large volumes) sweep the same way, with nh_overlap's predicates.
// include/nudge_hip.h, "scene queries".
// Layer masks (include/nudge_hip.h, "layer masks"): every query call walks under the mask(s) nh_query_filter set, in the FILTER = true instantiation of its kernel.
// Traversal is stackless: a node that is missed or a leaf that is done continues at its ESCAPE link (the next node in pre-order after its subtree),
// a hit internal node at its left child.  A private stack array would go to scratch memory.
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <utility>
#include "nh_query_tree.h"

// ---- what the walks share -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool nh_q_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool nh_q_finite(nh_f3 v) { return nh_q_finite(v.x) && nh_q_finite(v.y) && nh_q_finite(v.z); }
__device__ __forceinline__ bool nh_q_finite(nh_quat q) { return nh_q_finite(q.x) && nh_q_finite(q.y) && nh_q_finite(q.z) && nh_q_finite(q.s); }

// A collider's record as the predicates of nh_query.h take it: position, rotation, half extents (h.x: the radius of a sphere)
struct nh_QShape { nh_f3 p; nh_quat q; nh_f3 h; };
__device__ __forceinline__ nh_QShape nh_q_unpack(const nh_QRec& r) {
	return { nh_make3(r.a.x, r.a.y, r.a.z), nh_quat{ r.b.x, r.b.y, r.b.z, r.b.w }, nh_make3(r.c.x, r.c.y, r.c.z) };
}

// Who collider c (combined index) is: (body, index among its shape, shape, tag) -- nh_OverlapHit's four words, and the second 16 bytes of nh_RayHit
// and nh_PenetrationHit
__device__ __forceinline__ uint4 nh_q_identity(uint32_t c, uint32_t nbox, const nh_QRec& r) {
	return make_uint4(__float_as_uint(r.a.w), c < nbox ? c : c - nbox, c < nbox ? NH_SHAPE_BOX : NH_SHAPE_SPHERE, __float_as_uint(r.c.w));
}

// A volume record (nh_OverlapQuery; nh_DistanceQuery starts as one): the one decode nh_overlap, nh_penetration and nh_distance read it through -- the second
// promises the first's set and the third its validity.  A capsule of half height 0 is a sphere query: the same functions, its rotation not read.  `ok`: a
// known shape, every field it reads finite, no size negative.  a: the half axis of a capsule (else 0); e: the half extent of the world AABB, not padded.
struct nh_QVolume {
	nh_f3 c, h, a, e;
	nh_quat q;
	uint32_t ignore;
	bool capsule, sphere, ok;
	__device__ __forceinline__ void read(const float4* __restrict__ qp) {
		const float4 q0 = qp[0], q1 = qp[1], q2 = qp[2];
		c = nh_make3(q0.x, q0.y, q0.z); h = nh_make3(q2.x, q2.y, q2.z);
		q = { q1.x, q1.y, q1.z, q1.w };
		const uint32_t shape = __float_as_uint(q0.w);
		ignore = __float_as_uint(q2.w);
		capsule = shape == NH_SHAPE_CAPSULE && h.y != 0.0f;
		sphere = !capsule && (shape == NH_SHAPE_SPHERE || shape == NH_SHAPE_CAPSULE);
		ok = (sphere || capsule || shape == NH_SHAPE_BOX) && nh_q_finite(c) && nh_q_finite(h.x) && !(h.x < 0.0f);
		if (!sphere) ok = ok && nh_q_finite(h.y) && !(h.y < 0.0f) && nh_q_finite(q);
		if (!sphere && !capsule) ok = ok && nh_q_finite(h.z) && !(h.z < 0.0f);
		a = capsule ? nh_q_capsule_axis(q, h.y) : nh_make3(0.0f, 0.0f, 0.0f);
		e = sphere ? nh_make3(h.x, h.x, h.x) : capsule ? nh_q_capsule_extent(a, h.x) : nh_q_box_extent(q, h);
	}
};

// A list call's segment of records (nh_overlap, nh_penetration, the all-hits casts): the count pass (LIST = false) counts what query i finds into
// offsets[i]; behind the scan the list pass (LIST = true) finds the same again and writes record k of query i at offsets[i] + k.  Key and value are
// the caller's own.
template <bool LIST>
struct nh_QSegment {
	uint32_t base = 0u, end = 0u, k = 0u;
	// before the loop over the queries; `first`: the chain's first launch resets the words the scan and k_q_overlap_fix go on from.  The written prefix.
	__device__ static __forceinline__ uint32_t begin(bool first, uint32_t* offsets, uint32_t count, nh_QCtl* ctl) {
		if (!LIST && first && blockIdx.x == 0 && threadIdx.x == 0) { offsets[count] = 0u; ctl->ov_wrap = 0u; ctl->ov_written = 0u; }   // (k_q_overlap_fix sets both)
		return LIST ? ctl->ov_written : 0u;
	}
	// false: query i has nothing to list -- its segment is empty, or not in the written prefix
	__device__ __forceinline__ bool open(const uint32_t* offsets, uint32_t i, uint32_t written) {
		if (!LIST) return true;
		base = offsets[i]; end = offsets[i + 1u];
		return base < end && end <= written;
	}
	__device__ __forceinline__ uint32_t at() const { return base + k; }
	// one more found (LIST: written at at()); true ends the walk: the count pass found exactly end - base, so the segment is full and nothing else can follow
	__device__ __forceinline__ bool add() {
		if (LIST && base + k + 1u == end) return true;
		++k;
		return false;
	}
};

// The stackless walk (the head of this file) from `node`: enter(lo, hi, x) says whether a node's box is entered and may leave a number x for the leaf
// (the casts' entry t0, the point query's squared distance); leaf(c, record, x) sees every entered leaf whose body is not `ignore` and returns true
// to end the walk (any-hit; a list segment that is full).
//
// FILTER (header, "layer masks"): a node whose word of layer bits shares none with the query's mask m holds nothing the query may see -- the word is the
// OR over its leaves -- and is left by its escape link before the box test; a leaf's word is its collider's.  words = NULL: no layers are set, every word
// is all ones.  The FILTER = false walk reads neither.
struct nh_QFilter {
	const uint32_t* words;       // by node id (nh_QueryState::node_layers), or NULL
	const uint32_t* masks;       // per query, or NULL: every query uses `mask`
	uint32_t mask;
	__device__ __forceinline__ uint32_t of(uint32_t i) const { return masks ? masks[i] : mask; }
	__device__ __forceinline__ bool sees(uint32_t node, uint32_t m) const { return ((words ? words[node] : 0xffffffffu) & m) != 0u; }
};

template <bool FILTER, class Enter, class Leaf>
__device__ __forceinline__ void nh_q_walk(const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec, uint32_t node, uint32_t ignore,
                                          const nh_QFilter& F, uint32_t m, Enter enter, Leaf leaf) {
	float x = 0.0f;
	while (node != NH_Q_NONE) {
		const float4 na = nodes[node].a, nb = nodes[node].b;
		if (FILTER && !F.sees(node, m)) { node = __float_as_uint(nb.w); continue; }
		const bool in = enter(nh_make3(na.x, na.y, na.z), nh_make3(nb.x, nb.y, nb.z), x);
		const uint32_t left = __float_as_uint(na.w);
		const uint32_t rope = __float_as_uint(nb.w);
		if (!in) { node = rope; continue; }
		if (!(left & NH_Q_LEAF)) { node = left; continue; }
		node = rope;
		const uint32_t c = left & ~NH_Q_LEAF;
		const nh_QRec q = rec[c];
		if (__float_as_uint(q.a.w) == ignore) continue;
		if (leaf(c, q, x)) break;
	}
}

// ---- closest-hit casts ------------------------------------------------------------------------------------------------------------------------
// Every cast record starts as nh_Ray does: (origin, max_t), (direction, bits(ignore_body)).  A cast shape adds its own words and gives the walk three
// things: read() -- the decode, `ok` (every field it reads is finite and no size is negative) and the grow w of the node boxes; node() -- the node
// test, nh_q_cast_node / nh_q_cast_node3 (nh_query.h) under that grow; leaf() -- the two predicates of nh_query.h and, for a shape with a size, the
// reach rule: the hit is at max(t_pred, the leaf's entry t0), which is what makes the pruning exact.  The all-hits kernels below read
// their casts through the same structs, and each shape gives them three more: raylike() -- the shape has no size, so the set is the predicates' and the
// walk adds nh_q_all_pad to grow(), the one number its grow then is; all() -- the per-collider decision of nh_query.h (leaf() and then 0 <= t <= max_t); entry() -- the leaf entry t0 rebuilt where
// all() reads it, for the gather, which has no walk to take it from.  ALL_WAVES is the waves-per-EU hint of the all-hits kernels (0: none).
struct nh_QCastHead {
	nh_f3 o, d, inv;
	float max_t;
	uint32_t ignore;
	bool ok;
	__device__ __forceinline__ void head(float4 c0, float4 c1) {
		o = nh_make3(c0.x, c0.y, c0.z); d = nh_make3(c1.x, c1.y, c1.z);
		max_t = c0.w; ignore = __float_as_uint(c1.w);
		ok = nh_q_finite(o) && nh_q_finite(d);
		inv = nh_make3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
	}
};

// nh_Ray.  The pad is 2^-18 of the largest coordinate of the origin: nh_q_cast_pad(o, 0), the number a ball of radius 0 gets.
struct nh_QRay : nh_QCastHead {
	static constexpr uint32_t WORDS = 2u;
	float r, w;
	__device__ __forceinline__ void read(const float4* __restrict__ cp) { set(cp[0], cp[1]); }
	// the decode of the record's two 16-byte words, for k_q_sense as well, which builds each of its rays in registers
	__device__ __forceinline__ void set(float4 c0, float4 c1) {
		head(c0, c1);
		r = 0.0f;
		w = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z)) * 3.814697265625e-06f;
	}
	__device__ __forceinline__ bool node(nh_f3 lo, nh_f3 hi, float& t0) const { return nh_q_cast_node(lo, hi, o, inv, w, t0); }
	__device__ __forceinline__ nh_QHit leaf(const nh_QShape& c, bool box, float) const {
		return box ? nh_q_ray_box(o, d, c.p, c.q, c.h) : nh_q_ray_sphere(o, d, c.p, c.h.x);
	}
	static constexpr int ALL_WAVES = 0, K_WAVES = 0;
	__device__ __forceinline__ bool raylike() const { return true; }
	__device__ __forceinline__ float grow() const { return w; }
	__device__ __forceinline__ void entry(const nh_QShape&, bool, float&) const {}
	__device__ __forceinline__ nh_QHit all(const nh_QShape& c, bool box, float t0) const { return nh_q_all_hit<false>(o, d, r, max_t, t0, c.p, c.q, c.h, box); }
};

// nh_SphereCast: every node box grown by w = r + pad.  r = 0 walks and answers as the ray does.
struct nh_QBall : nh_QCastHead {
	static constexpr uint32_t WORDS = 3u;
	float r, w;
	__device__ __forceinline__ void read(const float4* __restrict__ cp) {
		head(cp[0], cp[1]);
		r = cp[2].x;
		ok = ok && nh_q_finite(r) && !(r < 0.0f);
		w = r + nh_q_cast_pad(o, r);
	}
	// the same decode from registers, for k_q_sweep, which builds each of its casts there (read() stays as it is: its kernels keep their code)
	__device__ __forceinline__ void set(float4 c0, float4 c1, float radius) {
		head(c0, c1);
		r = radius;
		ok = ok && nh_q_finite(r) && !(r < 0.0f);
		w = r + nh_q_cast_pad(o, r);
	}
	__device__ __forceinline__ bool node(nh_f3 lo, nh_f3 hi, float& t0) const { return nh_q_cast_node(lo, hi, o, inv, w, t0); }
	__device__ __forceinline__ nh_QHit leaf(const nh_QShape& c, bool box, float t0) const {
		nh_QHit hit = box ? nh_q_sweep_box(o, d, r, c.p, c.q, c.h) : nh_q_sweep_sphere(o, d, r, c.p, c.h.x);
		if (r > 0.0f && t0 > hit.t) hit.t = t0;
		return hit;
	}
	static constexpr int ALL_WAVES = 0, K_WAVES = 0;
	__device__ __forceinline__ bool raylike() const { return !(r > 0.0f); }
	__device__ __forceinline__ float grow() const { return w; }
	__device__ __forceinline__ void entry(const nh_QShape& c, bool box, float& t0) const { if (r > 0.0f) nh_q_leaf_entry(o, inv, w, c.p, c.q, c.h, box, t0); }
	__device__ __forceinline__ nh_QHit all(const nh_QShape& c, bool box, float t0) const { return nh_q_all_hit<true>(o, d, r, max_t, t0, c.p, c.q, c.h, box); }
};

// nh_BoxCast: the node box grown per axis by the cast box's world AABB half extent plus the pad.  Size 0 (`ray`) walks and answers as the
// ray does and does not read the rotation.
struct nh_QBox : nh_QCastHead {
	static constexpr uint32_t WORDS = 4u;
	nh_quat qa;
	nh_f3 h, w;
	bool ray;
	__device__ __forceinline__ void read(const float4* __restrict__ cp) { set(cp[0], cp[1], cp[2], cp[3]); }
	// the decode of the record's four 16-byte words, for k_q_move and k_q_walk as well, which build each of their casts in registers
	__device__ __forceinline__ void set(float4 c0, float4 c1, float4 c2, float4 c3) {
		head(c0, c1);
		qa = { c2.x, c2.y, c2.z, c2.w }; h = nh_make3(c3.x, c3.y, c3.z);
		ray = h.x == 0.0f && h.y == 0.0f && h.z == 0.0f;
		ok = ok && nh_q_finite(h) && !(h.x < 0.0f) && !(h.y < 0.0f) && !(h.z < 0.0f) && (ray || nh_q_finite(qa));
		const nh_f3 e = ray ? nh_make3(0.0f, 0.0f, 0.0f) : nh_q_box_extent(qa, h);
		const float s = nh_q_cast_pad(o, fmaxf(fmaxf(e.x, e.y), e.z));
		w = nh_make3(e.x + s, e.y + s, e.z + s);
	}
	__device__ __forceinline__ bool node(nh_f3 lo, nh_f3 hi, float& t0) const { return nh_q_cast_node3(lo, hi, o, inv, w, t0); }
	__device__ __forceinline__ nh_QHit leaf(const nh_QShape& c, bool box, float t0) const {
		nh_QHit hit = box ? nh_q_sweep_box_box(o, d, qa, h, c.p, c.q, c.h) : nh_q_sweep_box_sphere(o, d, qa, h, c.p, c.h.x);
		if (!ray && t0 > hit.t) hit.t = t0;
		return hit;
	}
	static constexpr int ALL_WAVES = 4, K_WAVES = 3;
	__device__ __forceinline__ bool raylike() const { return ray; }
	__device__ __forceinline__ float grow() const { return w.x; }          // (ray-like: the three are one number, the ray's)
	__device__ __forceinline__ void entry(const nh_QShape& c, bool box, float& t0) const { if (!ray) nh_q_leaf_entry3(o, inv, w, c.p, c.q, c.h, box, t0); }
	__device__ __forceinline__ nh_QHit all(const nh_QShape& c, bool box, float t0) const { return nh_q_all_hit_box(o, d, qa, h, max_t, t0, c.p, c.q, c.h, box); }
};

// nh_CapsuleCast: the box cast's node test with the capsule's world AABB half extent |a_k| + r, the reach rule unless r = hh = 0.  hh = 0
// walks and answers as the ball does (e = r on every axis, the same pad, the same node test's bits) and does not read the rotation.
struct nh_QCapsule : nh_QCastHead {
	static constexpr uint32_t WORDS = 4u;
	nh_quat qa;
	float r, hh;
	nh_f3 w;
	__device__ __forceinline__ void read(const float4* __restrict__ cp) { set(cp[0], cp[1], cp[2], cp[3]); }
	// the decode of the record's four 16-byte words, for k_q_move as well, which builds each of its casts in registers
	__device__ __forceinline__ void set(float4 c0, float4 c1, float4 c2, float4 c3) {
		head(c0, c1);
		qa = { c2.x, c2.y, c2.z, c2.w }; r = c3.x; hh = c3.y;
		ok = ok && nh_q_finite(r) && nh_q_finite(hh) && !(r < 0.0f) && !(hh < 0.0f) && (hh == 0.0f || nh_q_finite(qa));
		const nh_f3 e = nh_q_capsule_extent(nh_q_capsule_axis(qa, hh), r);
		const float s = nh_q_cast_pad(o, fmaxf(fmaxf(e.x, e.y), e.z));
		w = nh_make3(e.x + s, e.y + s, e.z + s);
	}
	__device__ __forceinline__ bool node(nh_f3 lo, nh_f3 hi, float& t0) const { return nh_q_cast_node3(lo, hi, o, inv, w, t0); }
	__device__ __forceinline__ nh_QHit leaf(const nh_QShape& c, bool box, float t0) const {
		nh_QHit hit = box ? nh_q_sweep_capsule_box(o, d, qa, r, hh, c.p, c.q, c.h) : nh_q_sweep_capsule_sphere(o, d, qa, r, hh, c.p, c.h.x);
		if ((r > 0.0f || hh > 0.0f) && t0 > hit.t) hit.t = t0;
		return hit;
	}
	static constexpr int ALL_WAVES = 4, K_WAVES = 4;
	__device__ __forceinline__ bool raylike() const { return r == 0.0f && hh == 0.0f; }
	__device__ __forceinline__ float grow() const { return w.x; }
	__device__ __forceinline__ void entry(const nh_QShape& c, bool box, float& t0) const { if (r > 0.0f || hh > 0.0f) nh_q_leaf_entry3(o, inv, w, c.p, c.q, c.h, box, t0); }
	__device__ __forceinline__ nh_QHit all(const nh_QShape& c, bool box, float t0) const { return nh_q_all_hit_capsule(o, d, qa, r, hh, max_t, t0, c.p, c.q, c.h, box); }
};

// One nh_RayHit, as two 16-byte stores: collider c hit at t with normal n, or, for c = NH_Q_NONE, the miss record, whose t is the cast's max_t (the
// caller's t) -- a quiet NaN where the cast itself is not `valid`.
__device__ __forceinline__ void nh_q_write_hit(nh_RayHit* __restrict__ hit, const nh_QRec* __restrict__ rec, uint32_t nbox, bool valid, uint32_t c, float t, nh_f3 n) {
	nh_RayHit out;
	out.t = valid ? t : __uint_as_float(0x7fc00000u);
	out.normal[0] = n.x; out.normal[1] = n.y; out.normal[2] = n.z;
	if (c == NH_Q_NONE) {
		out.body = out.collider = out.tag = NH_Q_NONE;
		out.shape = NH_SHAPE_NONE;
	} else {
		const uint4 id = nh_q_identity(c, nbox, rec[c]);
		out.body = id.x; out.collider = id.y; out.shape = id.z; out.tag = id.w;
	}
	float4* hp = reinterpret_cast<float4*>(hit);
	hp[0] = make_float4(out.t, out.normal[0], out.normal[1], out.normal[2]);
	hp[1] = make_float4(__uint_as_float(out.body), __uint_as_float(out.collider), __uint_as_float(out.shape), __uint_as_float(out.tag));
}

// One nh_PointHit, as three 16-byte stores: collider c at distance d with normal n and closest point x, or, for c = NH_Q_NONE, the miss record, whose distance
// is d (the caller's max_distance) -- a quiet NaN where the query itself is not `valid`.
__device__ __forceinline__ void nh_q_write_point(nh_PointHit* __restrict__ hit, const nh_QRec* __restrict__ rec, uint32_t nbox, bool valid, uint32_t c, float d, nh_f3 n, nh_f3 x) {
	float4* hp = reinterpret_cast<float4*>(hit);
	if (c == NH_Q_NONE) {
		hp[0] = make_float4(valid ? d : __uint_as_float(0x7fc00000u), 0.0f, 0.0f, 0.0f);
		hp[1] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(NH_Q_NONE));
		hp[2] = make_float4(__uint_as_float(NH_Q_NONE), __uint_as_float(NH_SHAPE_NONE), __uint_as_float(NH_Q_NONE), 0.0f);
	} else {
		const uint4 id = nh_q_identity(c, nbox, rec[c]);
		hp[0] = make_float4(d, n.x, n.y, n.z);
		hp[1] = make_float4(x.x, x.y, x.z, __uint_as_float(id.x));
		hp[2] = make_float4(__uint_as_float(id.y), __uint_as_float(id.z), __uint_as_float(id.w), 0.0f);
	}
}

// One decoded cast k under the mask m: the walk prunes at the best t so far, nh_q_better (nh_query.h) keeps the closest hit and the tie rule, any_hit stops
// at the first.  Leaves (bt, bc, bn) as nh_q_write_hit takes them: the hit, or bc = NH_Q_NONE with bt = the cast's max_t.  The closest-hit kernels and
// every round of k_q_move answer through this one body.
template <bool FILTER, class Shape>
__device__ __forceinline__ void nh_q_cast_one(const Shape& k, const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox,
                                              uint32_t any_hit, const nh_QFilter& F, uint32_t m, float& bt, uint32_t& bc, nh_f3& bn) {
	bt = k.max_t;
	bc = NH_Q_NONE;
	bn = nh_make3(0.0f, 0.0f, 0.0f);
	nh_q_walk<FILTER>(nodes, rec, k.ok && n ? 0u : NH_Q_NONE, k.ignore, F, m,
		[&](nh_f3 lo, nh_f3 hi, float& t0) { return k.node(lo, hi, t0) && t0 <= bt; },
		[&](uint32_t c, const nh_QRec& q, float t0) {
			const nh_QHit h = k.leaf(nh_q_unpack(q), c < nbox, t0);
			if (!(h.hit && nh_q_better(h.t, c, k.max_t, bt, bc))) return false;
			bt = h.t; bc = c; bn = h.n;
			return any_hit != 0u;
		});
}

// One lane per cast.
template <class Shape, bool FILTER>
__device__ __forceinline__ void nh_q_cast(const float4* __restrict__ casts, uint32_t count, nh_RayHit* __restrict__ hits, const nh_QNode* __restrict__ nodes,
                                          const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox, uint32_t any_hit, const nh_QFilter& F) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
		Shape k;
		k.read(casts + (size_t)i * Shape::WORDS);
		float bt;
		uint32_t bc;
		nh_f3 bn;
		nh_q_cast_one<FILTER>(k, nodes, rec, n, nbox, any_hit, F, FILTER ? F.of(i) : 0u, bt, bc, bn);
		nh_q_write_hit(hits + i, rec, nbox, k.ok, bc, bt, bn);
	}
}

template <bool FILTER>
__global__ __launch_bounds__(256) void k_q_raycast(const nh_Ray* __restrict__ rays, uint32_t count, nh_RayHit* __restrict__ hits,
                                                   const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox, uint32_t any_hit, nh_QFilter F) {
	nh_q_cast<nh_QRay, FILTER>(reinterpret_cast<const float4*>(rays), count, hits, nodes, rec, n, nbox, any_hit, F);
}

template <bool FILTER>
__global__ __launch_bounds__(256) void k_q_spherecast(const nh_SphereCast* __restrict__ casts, uint32_t count, nh_RayHit* __restrict__ hits,
                                                      const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox, uint32_t any_hit, nh_QFilter F) {
	nh_q_cast<nh_QBall, FILTER>(reinterpret_cast<const float4*>(casts), count, hits, nodes, rec, n, nbox, any_hit, F);
}

// (Without the waves-per-EU hint the box-box test lands at 129 VGPRs and 3 waves; with it, 128 and 4, no scratch.  The filtered walk holds two more
// values across the box-box test and under that hint spills them (8 bytes of scratch per lane): it is asked for 3 waves and keeps everything in registers.)
template <bool FILTER>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(FILTER ? 3 : 4))) void k_q_boxcast(const nh_BoxCast* __restrict__ casts, uint32_t count, nh_RayHit* __restrict__ hits,
                                                   const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox, uint32_t any_hit, nh_QFilter F) {
	nh_q_cast<nh_QBox, FILTER>(reinterpret_cast<const float4*>(casts), count, hits, nodes, rec, n, nbox, any_hit, F);
}

template <bool FILTER>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_q_capsulecast(const nh_CapsuleCast* __restrict__ casts, uint32_t count, nh_RayHit* __restrict__ hits,
                                                   const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox, uint32_t any_hit, nh_QFilter F) {
	nh_q_cast<nh_QCapsule, FILTER>(reinterpret_cast<const float4*>(casts), count, hits, nodes, rec, n, nbox, any_hit, F);
}

// ---- sensors ------------------------------------------------------------------------------------------------------------------------------------
// nh_sense, nh_sense_rays: the work item of a WAVE is (sensor s, block of 64 consecutive beams), count * ceil(beam_count / 64) of them, one a wave up to
// NH_Q_SENSE_GRID workgroups and dealt to the waves of that grid in turn beyond it.  s is the same in every lane by construction and is marked so (readfirstlane): the sensor's record, its mount's body transform and
// the pose composition (nh_q_sensor_pose, nh_query.h) are fetched and done once per wave from one address, and every lane shares the origin, the ignored
// body, the mask and the ray's pad.  The lanes read 64 adjacent nh_Beam (1 KB), rotate them (nh_q_sensor_ray) and -- k_q_sense -- answer the ray they hold
// in registers through nh_q_cast_one, the body of k_q_raycast: so (t, collider, normal) are nh_raycast's for the nh_Ray record k_q_sense_rays stores,
// under the same flags and the same mask (the sensor's index).  Each requested channel leaves as one 4-byte store per lane, adjacent across the wave; a
// NULL channel costs no store.  Tail lanes (beam >= beam_count) do nothing.  No packets, no shared stack: the per-lane stackless walk on near-identical
// rays already reads the same nodes in the same order.
static_assert(sizeof(nh_Beam) == 16 && sizeof(nh_Sensor) == 48 && offsetof(nh_Sensor, body) == 12 && offsetof(nh_Sensor, rotation) == 16 && offsetof(nh_Sensor, ignore_body) == 32,
              "nh_Beam is one 16-byte word, nh_Sensor three");
// Workgroups of four waves: 262,144 wave items a pass, 16.7 M rays at 64 beams an item.  A grid of one wave per SIMD slot (2048 workgroups) that strides over
// the items was measured first and lost: the stride is a multiple of the items of a sensor, so a wave takes the SAME block of the pattern of sensor after
// sensor -- the waves that hold a camera's horizon tiles or a lidar's level rings walk long every time, the ones that look at the sky finish at once -- and
// nh_sense took 1.4 x (pinhole) and 4.2 x (lidar) the time of nh_raycast on the same rays.  With an item a wave the hardware deals the work as it deals
// nh_raycast's, and the two take the same time (profiles/sense_rates.log).  Larger batches stride.
#define NH_Q_SENSE_GRID 65536u

struct nh_QSensorHead { nh_QPose w; uint32_t ignore; bool exists; };
__device__ __forceinline__ nh_QSensorHead nh_q_sensor_head(const nh_Sensor* __restrict__ sensors, uint32_t s, const nh_Transform* __restrict__ bodies, uint32_t body_count) {
	const float4* sp = reinterpret_cast<const float4*>(sensors + s);
	const float4 s0 = sp[0], s1 = sp[1];
	nh_QSensorHead h;
	h.ignore = __float_as_uint(sp[2].x);
	const uint32_t body = __float_as_uint(s0.w);
	const bool mounted = bodies != nullptr && body != NH_Q_NONE;
	h.exists = !mounted || body < body_count;
	nh_Transform b = {};
	if (mounted && h.exists) b = bodies[body];
	h.w = nh_q_sensor_pose(nh_make3(s0.x, s0.y, s0.z), nh_quat{ s1.x, s1.y, s1.z, s1.w }, mounted, h.exists, nh_make3(b.position[0], b.position[1], b.position[2]),
	                       nh_quat{ b.rotation[0], b.rotation[1], b.rotation[2], b.rotation[3] });
	return h;
}

// f(s, j, i, head) for every ray of the call whose wave item this wave is dealt: sensor s (wave-uniform), beam j, ray i = s * beam_count + j
template <class F>
__device__ __forceinline__ void nh_q_sense_items(const nh_Sensor* __restrict__ sensors, uint32_t count, uint32_t beam_count, const nh_Transform* __restrict__ bodies,
                                                 uint32_t body_count, F f) {
	const uint32_t lane = threadIdx.x & 63u, per = (beam_count + 63u) / 64u, items = count * per, waves = gridDim.x * (blockDim.x / 64u);
	for (uint32_t item = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u); item < items; item += waves) {
		const uint32_t s = item / per, j = (item - s * per) * 64u + lane;
		const nh_QSensorHead h = nh_q_sensor_head(sensors, s, bodies, body_count);
		if (j < beam_count) f(s, j, (size_t)s * beam_count + j, h);
	}
}

__device__ __forceinline__ nh_QSensorRay nh_q_sense_ray(const nh_Beam* __restrict__ beams, uint32_t j, const nh_QSensorHead& h) {
	const float4 b = reinterpret_cast<const float4*>(beams)[j];
	return nh_q_sensor_ray(h.w, h.exists, nh_make3(b.x, b.y, b.z), b.w, h.ignore);
}

template <bool FILTER>
__global__ __launch_bounds__(256) void k_q_sense(const nh_Sensor* __restrict__ sensors, uint32_t count, const nh_Beam* __restrict__ beams, uint32_t beam_count,
                                                 const nh_Transform* __restrict__ bodies, uint32_t body_count, nh_SenseOut out,
                                                 const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox, uint32_t any_hit, nh_QFilter F) {
	float* __restrict__ const out_t = out.t;
	uint32_t* __restrict__ const out_body = out.body;
	uint32_t* __restrict__ const out_tag = out.tag;
	nh_RayHit* __restrict__ const out_hits = out.hits;
	nh_q_sense_items(sensors, count, beam_count, bodies, body_count, [&](uint32_t s, uint32_t j, size_t i, const nh_QSensorHead& h) {
		const nh_QSensorRay r = nh_q_sense_ray(beams, j, h);
		nh_QRay k;
		k.set(make_float4(r.o.x, r.o.y, r.o.z, r.max_t), make_float4(r.d.x, r.d.y, r.d.z, __uint_as_float(r.ignore)));
		float bt;
		uint32_t bc;
		nh_f3 bn;
		nh_q_cast_one<FILTER>(k, nodes, rec, n, nbox, any_hit, F, FILTER ? F.of(s) : 0u, bt, bc, bn);
		if (out_t) out_t[i] = k.ok ? bt : __uint_as_float(0x7fc00000u);
		uint32_t body = NH_Q_NONE, tag = NH_Q_NONE;
		if ((out_body || out_tag) && bc != NH_Q_NONE) { body = __float_as_uint(rec[bc].a.w); tag = __float_as_uint(rec[bc].c.w); }      // (nh_q_identity's words)
		if (out_body) out_body[i] = body;
		if (out_tag) out_tag[i] = tag;
		if (out_hits) nh_q_write_hit(out_hits + i, rec, nbox, k.ok, bc, bt, bn);
	});
}

__global__ __launch_bounds__(256) void k_q_sense_rays(const nh_Sensor* __restrict__ sensors, uint32_t count, const nh_Beam* __restrict__ beams, uint32_t beam_count,
                                                      const nh_Transform* __restrict__ bodies, uint32_t body_count, nh_Ray* __restrict__ rays) {
	nh_q_sense_items(sensors, count, beam_count, bodies, body_count, [&](uint32_t, uint32_t j, size_t i, const nh_QSensorHead& h) {
		const nh_QSensorRay r = nh_q_sense_ray(beams, j, h);
		float4* rp = reinterpret_cast<float4*>(rays + i);
		rp[0] = make_float4(r.o.x, r.o.y, r.o.z, r.max_t);
		rp[1] = make_float4(r.d.x, r.d.y, r.d.z, __uint_as_float(r.ignore));
	});
}

// ---- fast bodies ----------------------------------------------------------------------------------------------------------------------------------
// nh_sweep, nh_sweep_limit (header, "fast bodies"): every collider that travels far in the coming step is swept along its own velocity, and
// its body's velocity cut to where the sweep first touches.  The per-item arithmetic is nh_query.h's ("fast bodies"), which the host oracle runs as well.
//   k_q_sweep_flag     one lane per collider: its travel d from the tree's record and its body's state, 1 where it is selected; a closing 0
//   nh_scan_u32        in place: a selected collider's word is its place in the list, word nbox the number of boxes, word n the total
//   k_q_sweep_gather   one lane per collider: a selected one writes its index and its 64-byte cast record at its place -- iff the total fits; its first
//                      lane writes the two counts
//   k_q_sweep<BALL>    one lane per ENTRY of one shape's share of the list, [0, boxes) or [boxes, total): the lane finds its collider in the scan
//                      words (the last c whose word is <= the entry: 20 probes for a million colliders, against a walk of hundreds of nodes), rebuilds the
//                      cast in registers as the gather built it, decodes it through nh_QBox::set / nh_QBall::set and answers through nh_q_cast_one,
//                      nh_boxcast's and nh_spherecast's own body.  No cast record is read back, and a wave holds casts of one shape
//   k_q_limit_init     one lane per entry: its body's two words = (1.0f, nobody)
//   k_q_limit_min      one lane per entry: atomic min of the entry into its body's second word and, where the entry limits, of t's bits into the first
//                      (non-negative floats order as their bits do, and a minimum does not depend on the order: the bytes are a function of the input)
//   k_q_limit_apply    one lane per entry: the factor out; the one entry a body's second word names scales the body's velocity
// Every collider index read from a list is checked against n, every body index against the body count, every entry against the capacity.
struct nh_QSweepIn { const nh_Transform* transforms; const nh_BodyMomentum* momentum; uint32_t body_count; float time_step, min_travel, core; };

// The cast of collider c as four 16-byte words (nh_BoxCast's; a sphere's: nh_CapsuleCast's), and whether it is selected.  A body that does not exist is
// not read.
struct nh_QSweepCast { float4 c0, c1, c2, c3; bool selected; };
__device__ __forceinline__ nh_QSweepCast nh_q_sweep_cast(const nh_QRec& r, bool box, const nh_QSweepIn& in) {
	nh_QSweepCast k;
	const uint32_t b = __float_as_uint(r.a.w);
	k.selected = nh_q_sweep_body(b, in.body_count);
	nh_f3 d = nh_make3(0.0f, 0.0f, 0.0f);
	const nh_f3 h = nh_make3(r.c.x, r.c.y, r.c.z);
	if (k.selected) {
		const float4 pb = *reinterpret_cast<const float4*>(in.transforms + b);
		const float4* m = reinterpret_cast<const float4*>(in.momentum + b);
		const float4 v = m[0], w = m[1];
		d = nh_q_sweep_travel(nh_make3(r.a.x, r.a.y, r.a.z), nh_make3(pb.x, pb.y, pb.z), nh_make3(v.x, v.y, v.z), nh_make3(w.x, w.y, w.z), in.time_step);
		k.selected = nh_q_sweep_far(d, h, box, in.min_travel);
	}
	const nh_f3 s = nh_q_sweep_core(h, box, in.core);
	k.c0 = make_float4(r.a.x, r.a.y, r.a.z, 1.0f);
	k.c1 = make_float4(d.x, d.y, d.z, r.a.w);
	k.c2 = box ? r.b : make_float4(0.0f, 0.0f, 0.0f, 1.0f);
	k.c3 = make_float4(s.x, s.y, s.z, 0.0f);
	return k;
}

__global__ __launch_bounds__(256) void k_q_sweep_flag(const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox, nh_QSweepIn in, uint32_t* __restrict__ scan) {
	for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c <= n; c += gridDim.x * blockDim.x)
		scan[c] = c < n && nh_q_sweep_cast(rec[c], c < nbox, in).selected ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_q_sweep_gather(const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox, nh_QSweepIn in, const uint32_t* __restrict__ scan,
                                                        uint32_t* __restrict__ counts, uint32_t* __restrict__ colliders, nh_BoxCast* __restrict__ casts, uint32_t capacity) {
	const uint32_t boxes = scan[nbox], total = scan[n];
	if (blockIdx.x == 0 && threadIdx.x == 0) { counts[0] = boxes; counts[1] = total - boxes; }
	if ((!colliders && !casts) || total > capacity) return;          // all or none
	for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
		const uint32_t at = scan[c];
		if (scan[c + 1u] == at || at >= capacity) continue;          // not selected
		if (colliders) colliders[at] = c;
		if (!casts) continue;
		const nh_QSweepCast k = nh_q_sweep_cast(rec[c], c < nbox, in);
		float4* cp = reinterpret_cast<float4*>(casts + at);
		cp[0] = k.c0; cp[1] = k.c1; cp[2] = k.c2; cp[3] = k.c3;
	}
}

// the collider of entry e among [lo, hi): the last c whose scan word is <= e (the words do not decrease, and a selected collider's is its own place)
__device__ __forceinline__ uint32_t nh_q_sweep_find(const uint32_t* __restrict__ scan, uint32_t lo, uint32_t hi, uint32_t e) {
	while (hi - lo > 1u) {
		const uint32_t mid = lo + (hi - lo) / 2u;
		if (scan[mid] <= e) lo = mid; else hi = mid;
	}
	return lo;
}

// (the hint: k_q_boxcast's, for the same box-box test under the same walk; the ball's walk needs none, as k_q_spherecast's)
template <bool BALL, bool FILTER>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(BALL ? 0 : FILTER ? 3 : 4)))
void k_q_sweep(const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox, nh_QSweepIn in, const uint32_t* __restrict__ scan, nh_RayHit* __restrict__ hits,
               uint32_t capacity, const nh_QNode* __restrict__ nodes, nh_QFilter F) {
	const uint32_t boxes = scan[nbox], total = scan[n];
	if (total > capacity) return;
	const uint32_t first = BALL ? boxes : 0u, end = BALL ? total : boxes, c_lo = BALL ? nbox : 0u, c_hi = BALL ? n : nbox;
	for (uint32_t e = first + blockIdx.x * blockDim.x + threadIdx.x; e < end; e += gridDim.x * blockDim.x) {
		const uint32_t c = nh_q_sweep_find(scan, c_lo, c_hi, e);
		const nh_QSweepCast k = nh_q_sweep_cast(rec[c], !BALL, in);
		typename std::conditional<BALL, nh_QBall, nh_QBox>::type shape;
		if constexpr (BALL) shape.set(k.c0, k.c1, k.c3.x);
		else shape.set(k.c0, k.c1, k.c2, k.c3);
		float bt;
		uint32_t bc;
		nh_f3 bn;
		nh_q_cast_one<FILTER>(shape, nodes, rec, n, nbox, 0u, F, FILTER ? F.of(c) : 0u, bt, bc, bn);
		nh_q_write_hit(hits + e, rec, nbox, shape.ok, bc, bt, bn);
	}
}

// the entries of a list nh_sweep filled, as nh_sweep_limit reads them: none where the list was not written
struct nh_QSweepEntries { const uint32_t* counts; const uint32_t* colliders; const nh_RayHit* hits; uint32_t capacity; };
__device__ __forceinline__ uint32_t nh_q_limit_total(const nh_QSweepEntries& L) {
	const uint32_t a = L.counts[0], b = L.counts[1];
	return a <= L.capacity && b <= L.capacity - a ? a + b : 0u;
}
// the body of entry i, or NH_Q_NONE for an entry that names no collider of the tree or no body of the call
__device__ __forceinline__ uint32_t nh_q_limit_body(const nh_QSweepEntries& L, uint32_t i, const nh_QRec* __restrict__ rec, uint32_t n, uint32_t body_count) {
	const uint32_t c = L.colliders[i];
	if (c >= n) return NH_Q_NONE;
	const uint32_t b = __float_as_uint(rec[c].a.w);
	return b < body_count ? b : NH_Q_NONE;
}

__global__ __launch_bounds__(256) void k_q_limit_init(nh_QSweepEntries L, const nh_QRec* __restrict__ rec, uint32_t n, uint32_t body_count, uint2* __restrict__ words) {
	const uint32_t total = nh_q_limit_total(L);
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
		const uint32_t b = nh_q_limit_body(L, i, rec, n, body_count);
		if (b != NH_Q_NONE) words[b] = make_uint2(0x3f800000u, NH_Q_NONE);          // (every entry of a body stores the same two words)
	}
}

__global__ __launch_bounds__(256) void k_q_limit_min(nh_QSweepEntries L, const nh_QRec* __restrict__ rec, uint32_t n, uint32_t body_count, uint2* __restrict__ words) {
	const uint32_t total = nh_q_limit_total(L);
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
		const uint32_t b = nh_q_limit_body(L, i, rec, n, body_count);
		if (b == NH_Q_NONE) continue;
		atomicMin(&words[b].y, i);
		const float4 h0 = reinterpret_cast<const float4*>(L.hits + i)[0];
		const uint32_t shape = reinterpret_cast<const uint32_t*>(L.hits + i)[6];
		if (nh_q_sweep_limits(shape, h0.x)) atomicMin(&words[b].x, __float_as_uint(h0.x));
	}
}

__global__ __launch_bounds__(256) void k_q_limit_apply(nh_QSweepEntries L, const nh_QRec* __restrict__ rec, uint32_t n, uint32_t body_count, const uint2* __restrict__ words,
                                                       nh_BodyMomentum* __restrict__ momentum, float* __restrict__ factors) {
	const uint32_t total = nh_q_limit_total(L);
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
		const uint32_t b = nh_q_limit_body(L, i, rec, n, body_count);
		const uint2 w = b != NH_Q_NONE ? words[b] : make_uint2(0x3f800000u, NH_Q_NONE);
		const float f = __uint_as_float(w.x);
		if (factors) factors[i] = f;
		if (w.y != i || !(f < 1.0f)) continue;
		float4* m = reinterpret_cast<float4*>(momentum + b);
		float4 v = m[0];          // (.w: unused0, stored back as loaded)
		v.x *= f; v.y *= f; v.z *= f;
		m[0] = v;
	}
}

// ---- move -------------------------------------------------------------------------------------------------------------------------------------
// nh_move, nh_boxmove: one lane per move, Shape = nh_QCapsule or nh_QBox (nh_QMover<Shape> holds what differs).  The state machine is nh_query.h's ("move": nh_q_move_begin / _go / _advance, which the host's brute force runs as well);
// each round's cast is the record { p, 1.0f, v, ignore_body, rotation, radius, half_height } (for the box: rotation, size) decoded by Shape::set and answered by
// nh_q_cast_one, the body of k_q_capsulecast / k_q_boxcast -- so a round's (t, collider, normal) are nh_capsulecast's / nh_boxcast's for that record, under the same mask (the move's index).  The loop
// bound is a constant and every round is a walk that terminates, so the kernel terminates on any input.  A lane whose move has ended waits for the slowest
// of its wave.  The record leaves as four 16-byte stores; `ok` of the last cast decides its miss t as it does in nh_capsulecast (a position
// that overflowed makes an invalid cast: a miss with t = NaN).
static_assert(NH_Q_MOVE_HIT == NH_MOVE_HIT && NH_Q_MOVE_START_OVERLAP == NH_MOVE_START_OVERLAP && NH_Q_MOVE_SLIDES_OUT == NH_MOVE_SLIDES_OUT &&
              NH_Q_MOVE_WEDGED == NH_MOVE_WEDGED && NH_Q_MOVE_MAX_SLIDES == NH_MOVE_MAX_SLIDES, "nh_query.h's move constants are the header's");
static_assert(sizeof(nh_Move) == 64 && sizeof(nh_MoveResult) == 64, "nh_Move and nh_MoveResult are four 16-byte words each");
static_assert(sizeof(nh_BoxMove) == 64 && offsetof(nh_BoxMove, skin) == offsetof(nh_BoxCast, max_t) && offsetof(nh_BoxMove, max_slides) == offsetof(nh_BoxCast, reserved) &&
              offsetof(nh_BoxMove, size) == offsetof(nh_BoxCast, size), "nh_BoxMove is nh_BoxCast with skin at max_t and max_slides at reserved");
static_assert(sizeof(nh_BoxWalk) == 96 && offsetof(nh_BoxWalk, up) == offsetof(nh_Walk, up) && offsetof(nh_BoxWalk, options) == offsetof(nh_Walk, options),
              "nh_BoxWalk is nh_Walk's tail behind nh_BoxMove");

// What nh_move / nh_walk and nh_boxmove / nh_boxwalk do not share: the record types, where max_slides sits in the record's fourth word (the shape's own
// fields come first), the validity functions of nh_query.h, and the occupancy each kernel is asked for (its own comment).
template <class Shape> struct nh_QMover;
template <> struct nh_QMover<nh_QCapsule> {
	typedef nh_Move Move;
	typedef nh_Walk Walk;
	__device__ __forceinline__ static uint32_t max_slides(float4 m3) { return __float_as_uint(m3.z); }
	__device__ __forceinline__ static bool move_valid(nh_f3 o, nh_f3 d, float4 m2, float4 m3, float skin, uint32_t max_slides) {
		return nh_q_move_valid(o, d, nh_quat{ m2.x, m2.y, m2.z, m2.w }, m3.x, m3.y, skin, max_slides);
	}
	__device__ __forceinline__ static bool walk_valid(const nh_QWalkIn& W, float4 m2, float4 m3) { return nh_q_walk_valid(W, nh_quat{ m2.x, m2.y, m2.z, m2.w }, m3.x, m3.y); }
};
template <> struct nh_QMover<nh_QBox> {
	typedef nh_BoxMove Move;
	typedef nh_BoxWalk Walk;
	__device__ __forceinline__ static uint32_t max_slides(float4 m3) { return __float_as_uint(m3.w); }
	__device__ __forceinline__ static bool move_valid(nh_f3 o, nh_f3 d, float4 m2, float4 m3, float skin, uint32_t max_slides) {
		return nh_q_boxmove_valid(o, d, nh_quat{ m2.x, m2.y, m2.z, m2.w }, nh_make3(m3.x, m3.y, m3.z), skin, max_slides);
	}
	__device__ __forceinline__ static bool walk_valid(const nh_QWalkIn& W, float4 m2, float4 m3) {
		return nh_q_boxwalk_valid(W, nh_quat{ m2.x, m2.y, m2.z, m2.w }, nh_make3(m3.x, m3.y, m3.z));
	}
};
// waves per SIMD asked for: the capsule's 4 (k_q_capsulecast's).  The box move holds a move's state across the box-box sweep: 146 / 147 VGPRs (filter off / on) at 3
// waves, no scratch; asked for 4 waves the compiler spills 28 / 32 bytes per lane (-DNH_Q_BOXMOVE_WAVES=4 -DNH_Q_BOXMOVE_WAVES_FILTER=4 reproduces it)
#ifndef NH_Q_BOXMOVE_WAVES
#define NH_Q_BOXMOVE_WAVES 3
#endif
#ifndef NH_Q_BOXMOVE_WAVES_FILTER
#define NH_Q_BOXMOVE_WAVES_FILTER 3
#endif
template <class Shape> constexpr int nh_q_move_waves(bool) { return 4; }
template <> constexpr int nh_q_move_waves<nh_QBox>(bool filter) { return filter ? NH_Q_BOXMOVE_WAVES_FILTER : NH_Q_BOXMOVE_WAVES; }

// ---- touched ----------------------------------------------------------------------------------------------------------------------------------
// nh_move_touched and kin (TOUCHED = true of k_q_move and k_q_walk): the mover's own loop, and behind every cast that found a collider one nh_Touch, written
// while the state still holds the cast's origin and direction -- before the advance.  A lane owns the k slots touches[i * k ..] (a size_t index: count * k
// passes 2^32), fills them in cast order with four 16-byte stores each (nh_q_write_hit for the first two) and counts on where they are full; slots behind
// the count are never written (header, "nh_move_touched").  TOUCHED = false compiles none of it: k, counts and touches are then not read.
static_assert(NH_Q_TOUCH_SLIDE == NH_TOUCH_SLIDE && NH_Q_TOUCH_UP == NH_TOUCH_UP && NH_Q_TOUCH_FORWARD == NH_TOUCH_FORWARD && NH_Q_TOUCH_DOWN == NH_TOUCH_DOWN &&
              NH_Q_TOUCH_PROBE == NH_TOUCH_PROBE, "nh_query.h's touch phases are the header's");
static_assert(sizeof(nh_Touch) == 64 && offsetof(nh_Touch, origin) == 32 && offsetof(nh_Touch, phase) == 44 && offsetof(nh_Touch, direction) == 48 && offsetof(nh_Touch, cast) == 60,
              "nh_Touch is nh_RayHit and two 16-byte words");
__device__ __forceinline__ void nh_q_write_touch(nh_Touch* __restrict__ touch, const nh_QRec* __restrict__ rec, uint32_t nbox, uint32_t c, float t, nh_f3 n, nh_f3 o, nh_f3 d,
                                                 uint32_t phase, uint32_t cast) {
	nh_q_write_hit(&touch->hit, rec, nbox, true, c, t, n);
	float4* tp = reinterpret_cast<float4*>(touch);
	tp[2] = make_float4(o.x, o.y, o.z, __uint_as_float(phase));
	tp[3] = make_float4(d.x, d.y, d.z, __uint_as_float(cast));
}
// waves per SIMD asked for by the TOUCHED moves: their plain siblings' (the count and the slot address are held across the sweep: 128 VGPRs still for the capsule,
// 150 / 151 for the box, no scratch; the register table is DESIGN 10.20)
#ifndef NH_Q_MOVE_TOUCHED_WAVES
#define NH_Q_MOVE_TOUCHED_WAVES 4
#endif
template <class Shape> constexpr int nh_q_move_waves(bool filter, bool touched) { return touched ? NH_Q_MOVE_TOUCHED_WAVES : nh_q_move_waves<Shape>(filter); }
template <> constexpr int nh_q_move_waves<nh_QBox>(bool filter, bool) { return nh_q_move_waves<nh_QBox>(filter); }

template <class Shape, bool FILTER, bool TOUCHED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(nh_q_move_waves<Shape>(FILTER, TOUCHED)))) void k_q_move(const typename nh_QMover<Shape>::Move* __restrict__ moves, uint32_t count,
                                                   nh_MoveResult* __restrict__ results,
                                                   const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox, nh_QFilter F,
                                                   uint32_t k_touches, uint32_t* __restrict__ counts, nh_Touch* __restrict__ touches) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
		const float4* mp = reinterpret_cast<const float4*>(moves + i);
		const float4 m0 = mp[0], m1 = mp[1], m2 = mp[2], m3 = mp[3];
		const float skin = m0.w;
		const uint32_t max_slides = nh_QMover<Shape>::max_slides(m3);
		const bool valid = nh_QMover<Shape>::move_valid(nh_make3(m0.x, m0.y, m0.z), nh_make3(m1.x, m1.y, m1.z), m2, m3, skin, max_slides);
		nh_QMove s = nh_q_move_begin(nh_make3(m0.x, m0.y, m0.z), nh_make3(m1.x, m1.y, m1.z));
		const uint32_t fm = FILTER ? F.of(i) : 0u;
		float bt = 1.0f;
		uint32_t bc = NH_Q_NONE;
		nh_f3 bn = nh_make3(0.0f, 0.0f, 0.0f);
		bool ok = valid;
		uint32_t touched = 0u;
		for (uint32_t round = 0u; round <= NH_MOVE_MAX_SLIDES; ++round) {
			if (!valid || !nh_q_move_go(s)) break;
			Shape k;
			k.set(make_float4(s.p.x, s.p.y, s.p.z, 1.0f), make_float4(s.v.x, s.v.y, s.v.z, m1.w), m2, m3);
			nh_q_cast_one<FILTER>(k, nodes, rec, n, nbox, 0u, F, fm, bt, bc, bn);
			ok = k.ok;
			if (TOUCHED && bc != NH_Q_NONE) {
				if (touched < k_touches) nh_q_write_touch(touches + ((size_t)i * k_touches + touched), rec, nbox, bc, bt, bn, s.p, s.v, NH_TOUCH_SLIDE, round);
				++touched;
			}
			if (!nh_q_move_advance(s, bc != NH_Q_NONE, bt, bn, skin, max_slides)) break;
		}
		float4* out = reinterpret_cast<float4*>(results + i);
		out[0] = make_float4(s.p.x, s.p.y, s.p.z, __uint_as_float(valid ? s.flags : (uint32_t)NH_MOVE_INVALID));
		out[1] = make_float4(s.v.x, s.v.y, s.v.z, __uint_as_float(s.slides));
		nh_q_write_hit(&results[i].last_hit, rec, nbox, ok, bc, bt, bn);
		if (TOUCHED) counts[i] = touched;
	}
}

// ---- walk -------------------------------------------------------------------------------------------------------------------------------------
// nh_walk, nh_boxwalk: one lane per walk, Shape = nh_QCapsule or nh_QBox.  The phase machine is nh_query.h's ("walk": nh_q_walk_begin / _cast / _advance, which the host's brute force runs as well): up
// to five move loops one after the other (slide, up, forward, down, probe), each cast the record { s.m.p, 1.0f, s.m.v, ignore_body, rotation, radius,
// half_height } (for the box: rotation, size) decoded by Shape::set and answered by nh_q_cast_one, the body of k_q_capsulecast / k_q_boxcast.  There is ONE call site of the
// cast in ONE loop: the lane's phase only picks the origin and the direction, so the capsule sweep -- or the box-box SAT sweep -- is instantiated once and the lanes of a wave walk the tree together whatever
// phase each is in.  The loop bound is the constant NH_WALK_MAX_CASTS and every round is a walk that terminates, so the kernel terminates on any input.
// The record leaves as seven 16-byte stores.
static_assert(NH_Q_WALK_STEPPED == NH_WALK_STEPPED && NH_Q_WALK_GROUNDED == NH_WALK_GROUNDED && NH_Q_WALK_SNAPPED == NH_WALK_SNAPPED && NH_Q_WALK_STEEP == NH_WALK_STEEP &&
              NH_Q_WALK_ON_STEEP == NH_WALK_ON_STEEP && NH_Q_WALK_PROBE_ONLY == NH_WALK_PROBE_ONLY && NH_Q_WALK_MAX_CASTS == NH_WALK_MAX_CASTS && NH_WALK_MAX_CASTS == 21u &&
              NH_Q_WALK_NOBODY == NH_Q_NONE, "nh_query.h's walk constants are the header's");
static_assert(sizeof(nh_Walk) == 96 && sizeof(nh_WalkResult) == 112 && offsetof(nh_WalkResult, last_hit) == 32 && offsetof(nh_WalkResult, ground) == 64,
              "nh_Walk is six and nh_WalkResult seven 16-byte words");
// (What a walk keeps between two casts -- the record's rules, the kept slide, F's end while D runs: some 50 values -- lies idle during the tree walk.  Asked
// for k_q_move's 4 waves the compiler puts 132 (filter off) and 144 (on) bytes of it per lane into scratch; at 3 waves both instantiations hold everything in
// 168 VGPRs, no scratch.  DESIGN 10.18; -DNH_Q_WALK_WAVES=4 -Rpass-analysis=kernel-resource-usage reproduces the 4-wave figures.)
#ifndef NH_Q_WALK_WAVES
#define NH_Q_WALK_WAVES 3
#endif

// (The box walk holds a walk's state across the box-box sweep: 194 / 195 VGPRs (filter off / on) at 2 waves, no scratch; at nh_walk's 3 waves the compiler spills 56 / 60
// bytes per lane, at 4 waves 216 / 228.  DESIGN 10.19; -DNH_Q_BOXWALK_WAVES=3 -DNH_Q_BOXWALK_WAVES_FILTER=3 -Rpass-analysis=kernel-resource-usage reproduces the row.)
#ifndef NH_Q_BOXWALK_WAVES
#define NH_Q_BOXWALK_WAVES 2
#endif
#ifndef NH_Q_BOXWALK_WAVES_FILTER
#define NH_Q_BOXWALK_WAVES_FILTER 2
#endif
template <class Shape> constexpr int nh_q_walk_waves(bool) { return NH_Q_WALK_WAVES; }
template <> constexpr int nh_q_walk_waves<nh_QBox>(bool filter) { return filter ? NH_Q_BOXWALK_WAVES_FILTER : NH_Q_BOXWALK_WAVES; }
// (The TOUCHED capsule walk holds the touch count across the sweep on top of nh_walk's 168 VGPRs: asked for nh_walk's 3 waves the compiler spills 20 / 28 bytes
// per lane (filter off / on); at 2 waves it keeps everything in registers.  The box walk is at 2 waves already.  DESIGN 10.20;
// -DNH_Q_WALK_TOUCHED_WAVES=3 -Rpass-analysis=kernel-resource-usage reproduces the 3-wave figures.)
#ifndef NH_Q_WALK_TOUCHED_WAVES
#define NH_Q_WALK_TOUCHED_WAVES 2
#endif
template <class Shape> constexpr int nh_q_walk_waves(bool filter, bool touched) { return touched ? NH_Q_WALK_TOUCHED_WAVES : nh_q_walk_waves<Shape>(filter); }
template <> constexpr int nh_q_walk_waves<nh_QBox>(bool filter, bool) { return nh_q_walk_waves<nh_QBox>(filter); }

template <class Shape, bool FILTER, bool TOUCHED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(nh_q_walk_waves<Shape>(FILTER, TOUCHED)))) void k_q_walk(const typename nh_QMover<Shape>::Walk* __restrict__ walks, uint32_t count,
                                                   nh_WalkResult* __restrict__ results,
                                                   const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox, nh_QFilter F,
                                                   uint32_t k_touches, uint32_t* __restrict__ counts, nh_Touch* __restrict__ touches) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
		const float4* wp = reinterpret_cast<const float4*>(walks + i);
		const float4 m0 = wp[0], m1 = wp[1], m2 = wp[2], m3 = wp[3], m4 = wp[4], m5 = wp[5];
		nh_QWalkIn W;
		W.origin = nh_make3(m0.x, m0.y, m0.z); W.skin = m0.w;
		W.disp = nh_make3(m1.x, m1.y, m1.z); W.max_slides = nh_QMover<Shape>::max_slides(m3);
		W.up = nh_make3(m4.x, m4.y, m4.z); W.step_height = m4.w;
		W.snap = m5.x; W.mgu = m5.y; W.options = __float_as_uint(m5.z);
		const bool valid = nh_QMover<Shape>::walk_valid(W, m2, m3);
		nh_QWalk s = nh_q_walk_begin(W);
		const uint32_t fm = FILTER ? F.of(i) : 0u;
		uint32_t touched = 0u;
		for (uint32_t round = 0u; round < NH_WALK_MAX_CASTS; ++round) {
			if (!valid || !nh_q_walk_cast(s, W)) break;
			Shape k;
			k.set(make_float4(s.m.p.x, s.m.p.y, s.m.p.z, 1.0f), make_float4(s.m.v.x, s.m.v.y, s.m.v.z, m1.w), m2, m3);
			float bt;
			uint32_t bc;
			nh_f3 bn;
			nh_q_cast_one<FILTER>(k, nodes, rec, n, nbox, 0u, F, fm, bt, bc, bn);
			if (TOUCHED && bc != NH_Q_NONE) {
				if (touched < k_touches)
					nh_q_write_touch(touches + ((size_t)i * k_touches + touched), rec, nbox, bc, bt, bn, s.m.p, s.m.v, nh_q_walk_touch_phase(s.phase), s.casts);
				++touched;
			}
			nh_q_walk_advance(s, W, bc != NH_Q_NONE, bt, bc, bn, k.ok);
		}
		float4* out = reinterpret_cast<float4*>(results + i);
		out[0] = make_float4(s.kp.x, s.kp.y, s.kp.z, __uint_as_float(valid ? s.kflags : (uint32_t)NH_WALK_INVALID));
		out[1] = make_float4(s.kv.x, s.kv.y, s.kv.z, __uint_as_float(s.kslides));
		const nh_QWalkHit g = nh_q_walk_ground(s);
		nh_q_write_hit(&results[i].last_hit, rec, nbox, valid, s.klast.c, s.klast.t, s.klast.n);
		nh_q_write_hit(&results[i].ground, rec, nbox, valid, g.c, g.t, g.n);
		out[6] = make_float4(s.step_up, nh_q_walk_drop(s, W), __uint_as_float(s.casts), 0.0f);
		if (TOUCHED) counts[i] = touched;
	}
}

// ---- closest point ----------------------------------------------------------------------------------------------------------------------------
// One lane per query.  The bound bd starts at max_distance and only ever falls to the key of a real candidate (nh_q_point_key, nh_q_closer: the reach
// rule of DESIGN 10.5), so a node of squared distance d2 > 0 from p with sqrtf(d2) > bd can be skipped, and one with d2 = 0 is always entered.
//   seed  nh_q_seed: p's Morton key in the frame of the last build (clamped to its bounds), its place among the sorted keys by binary search, and the exact keys of
//         the NH_Q_SEED leaves on either side of that place: a bound near p before the walk, which otherwise goes left first from the root -- towards
//         the lowest Morton region, usually far from p.  Compiled out by -DNH_Q_CLOSEST_NO_SEED (tools/closest_rates.py measures both).
//   walk  nh_q_walk with the node test above; the leaves evaluate nh_q_point_box / nh_q_point_sphere and the key.  A seeded winner
//         met again does not replace itself (equal key and index), so the seed changes the work, never the answer.
#define NH_Q_SEED 4
// The Morton seed of the nearest-collider walks (k_q_closest, k_q_closest_k, k_q_distance): p's Morton key in the frame of the last build (clamped to its
// bounds), its place among the sorted keys by binary search, and the `win` leaves on either side of that place -- visit(c, record, lo, hi) for each whose
// body is not `ignore`, with its leaf box.  It only proposes real colliders to the caller's own leaf function, so it changes the work, never the answer.
// FILTER: a leaf the query's mask does not see is skipped, as the walk skips it.
template <bool FILTER, class Visit>
__device__ __forceinline__ void nh_q_seed(nh_f3 p, uint32_t win, uint32_t ignore, const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec,
                                          const uint64_t* __restrict__ keys, const nh_QCtl* __restrict__ ctl, uint32_t n, const nh_QFilter& F, uint32_t m, Visit visit) {
	const nh_f3 smin = nh_make3(nh_float_unflip(ctl->kmin[0]), nh_float_unflip(ctl->kmin[1]), nh_float_unflip(ctl->kmin[2]));
	const nh_f3 smax = nh_make3(nh_float_unflip(ctl->kmax[0]), nh_float_unflip(ctl->kmax[1]), nh_float_unflip(ctl->kmax[2]));
	const float scale = nh_morton_scale(smin, smax);
	const nh_f3 pc = nh_make3(fminf(fmaxf(p.x, smin.x), smax.x), fminf(fmaxf(p.y, smin.y), smax.y), fminf(fmaxf(p.z, smin.z), smax.z));
	const uint64_t key = nh_morton_of(pc, scale, smin * scale);
	uint32_t lo = 0u, hi = n;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (keys[mid] < key) lo = mid + 1u; else hi = mid;
	}
	const uint32_t j0 = lo > win ? lo - win : 0u, j1 = n - lo > win ? lo + win : n;
	for (uint32_t j = j0; j < j1; ++j) {
		if (FILTER && !F.sees(n - 1u + j, m)) continue;
		const float4 na = nodes[n - 1u + j].a, nb = nodes[n - 1u + j].b;
		const uint32_t c = __float_as_uint(na.w) & ~NH_Q_LEAF;
		const nh_QRec q = rec[c];
		if (__float_as_uint(q.a.w) == ignore) continue;
		visit(c, q, nh_make3(na.x, na.y, na.z), nh_make3(nb.x, nb.y, nb.z));
	}
}

// nh_PointQuery as k_q_closest and k_q_closest_k read it, and the point function of a collider's record
struct nh_QPointQuery {
	nh_f3 p;
	float max_d;
	uint32_t ignore;
	bool ok;
	__device__ __forceinline__ void read(const float4* __restrict__ qp) {
		const float4 q0 = qp[0], q1 = qp[1];
		p = nh_make3(q0.x, q0.y, q0.z);
		max_d = q0.w;
		ignore = __float_as_uint(q1.x);
		ok = nh_q_finite(p) && max_d >= 0.0f;       // (+inf is a valid max_distance; NaN is not)
	}
	__device__ __forceinline__ nh_QPoint to(const nh_QRec& q, bool box) const {
		const nh_QShape s = nh_q_unpack(q);
		return box ? nh_q_point_box(p, s.p, s.q, s.h) : nh_q_point_sphere(p, s.p, s.h.x);
	}
};

template <bool FILTER>
__global__ __launch_bounds__(256) void k_q_closest(const nh_PointQuery* __restrict__ queries, uint32_t count, nh_PointHit* __restrict__ hits,
                                                   const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec, const uint64_t* __restrict__ keys,
                                                   const nh_QCtl* __restrict__ ctl, uint32_t n, uint32_t nbox, nh_QFilter F) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
		nh_QPointQuery Q;
		Q.read(reinterpret_cast<const float4*>(queries + i));
		float bd = Q.max_d;
		uint32_t bc = NH_Q_NONE;
		nh_f3 bn = nh_make3(0.0f, 0.0f, 0.0f), bx = nh_make3(0.0f, 0.0f, 0.0f);
		const bool walk = Q.ok && n;
		const uint32_t fm = FILTER ? F.of(i) : 0u;
		// a leaf of squared box distance d2, for the seed and the walk alike
		const auto leaf = [&](uint32_t c, const nh_QRec& q, float d2) {
			const nh_QPoint h = Q.to(q, c < nbox);
			const float k = nh_q_point_key(h.d, d2);
			if (nh_q_closer(k, c, Q.max_d, bd, bc)) { bd = k; bc = c; bn = h.n; bx = h.x; }
			return false;
		};
#ifndef NH_Q_CLOSEST_NO_SEED
		if (walk) nh_q_seed<FILTER>(Q.p, NH_Q_SEED, Q.ignore, nodes, rec, keys, ctl, n, F, fm, [&](uint32_t c, const nh_QRec& q, nh_f3 lo, nh_f3 hi) { leaf(c, q, nh_q_point_node(lo, hi, Q.p)); });
#endif
		nh_q_walk<FILTER>(nodes, rec, walk ? 0u : NH_Q_NONE, Q.ignore, F, fm,
			[&](nh_f3 lo, nh_f3 hi, float& d2) { d2 = nh_q_point_node(lo, hi, Q.p); return !(d2 > 0.0f && sqrtf(d2) > bd); }, leaf);
		nh_q_write_point(hits + i, rec, nbox, Q.ok, bc, bd, bn, bx);
	}
}

// ---- the k nearest ------------------------------------------------------------------------------------------------------------------------------
// One lane per query on nh_q_walk, as k_q_closest; what a lane keeps is not one best candidate but the bounded ordered list of nh_query.h
// (nh_q_nearest_insert: (key, combined index), nh_q_closer's order, a candidate met twice goes in once).
//   list   in LDS, slot-major: entry j of lane l at lds[j * blockDim.x + l], 8 bytes -- a wave's access to one slot is contiguous, and no register
//          array is indexed dynamically (it would go to scratch).  Dynamic shared memory of blockDim.x * k * 8 bytes, the block size by k:
//              k  1 ..  8   256 lanes   at most 16 KiB
//              k  9 .. 16   128 lanes   at most 16 KiB
//              k 17 .. 32    64 lanes   at most 16 KiB
//          so a workgroup never takes more than a quarter of the 64 KiB it may have, and a CU's 160 KiB hold ten of the largest.
//   bound  bd, in a register: max_distance while fewer than k are held, the k-th key once the list is full.  A leaf whose key is not <= bd is
//          dropped by that one compare without touching LDS (equality goes on: a tie can still win by index).  The node test is k_q_closest's:
//          skip iff d2 > 0 && sqrtf(d2) > bd.
//   exact  bd is always the k-th key of a SUBSET of the candidates (or max_distance), hence at least the final k-th key K.  A collider of the
//          answer has key <= K, and its key is at least sqrtf(d2) of its own leaf box (nh_q_point_key); every ancestor's d2 is at most the
//          leaf's (nh_query.h).  So sqrtf(d2) <= K <= bd at every ancestor of a winner: none is ever skipped, whatever the order of the walk.
//   seed   k_q_closest's, the window widened to NH_Q_SEED + k / 2 leaves on either side (k = 1: the same leaves): the bound is usually the k-th
//          key of a neighbourhood of p before the walk starts.  The walk meets those leaves again and nh_q_nearest_insert drops them, so the
//          seed changes the work, never the bytes.  Compiled out by -DNH_Q_CLOSEST_K_NO_SEED (tools/nearest_rates.py measures both).
//   out    the list holds (key, index) only: nh_q_point_box / nh_q_point_sphere run again for the m held colliders -- the same bits -- and each
//          record leaves as three 16-byte stores, then the k - m miss records, then counts[i] = m.
static inline uint32_t nh_q_nearest_block(uint32_t k) { return k <= 8u ? 256u : k <= 16u ? 128u : 64u; }

template <bool FILTER>
__global__ __launch_bounds__(256) void k_q_closest_k(const nh_PointQuery* __restrict__ queries, uint32_t count, uint32_t k, uint32_t* __restrict__ counts,
                                                     nh_PointHit* __restrict__ hits, const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec,
                                                     const uint64_t* __restrict__ keys, const nh_QCtl* __restrict__ ctl, uint32_t n, uint32_t nbox, nh_QFilter F) {
	extern __shared__ nh_QNear q_near[];
	const uint32_t stride = blockDim.x;
	nh_QNear* const list = q_near + threadIdx.x;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
		nh_QPointQuery Q;
		Q.read(reinterpret_cast<const float4*>(queries + i));
		float bd = Q.max_d;
		uint32_t held = 0u;
		const bool walk = Q.ok && n;
		const uint32_t fm = FILTER ? F.of(i) : 0u;
		// a leaf of squared box distance d2, for the seed and the walk alike
		const auto leaf = [&](uint32_t c, const nh_QRec& q, float d2) {
			const float key = nh_q_point_key(Q.to(q, c < nbox).d, d2);
			if (!(key <= bd)) return false;
			if (nh_q_nearest_insert(list, stride, k, &held, key, c, Q.max_d) && held == k) bd = list[(k - 1u) * stride].key;
			return false;
		};
#ifndef NH_Q_CLOSEST_K_NO_SEED
		if (walk) nh_q_seed<FILTER>(Q.p, NH_Q_SEED + k / 2u, Q.ignore, nodes, rec, keys, ctl, n, F, fm, [&](uint32_t c, const nh_QRec& q, nh_f3 lo, nh_f3 hi) { leaf(c, q, nh_q_point_node(lo, hi, Q.p)); });
#endif
		nh_q_walk<FILTER>(nodes, rec, walk ? 0u : NH_Q_NONE, Q.ignore, F, fm,
			[&](nh_f3 lo, nh_f3 hi, float& d2) { d2 = nh_q_point_node(lo, hi, Q.p); return !(d2 > 0.0f && sqrtf(d2) > bd); }, leaf);
		nh_PointHit* out = hits + (size_t)i * k;
		for (uint32_t j = 0u; j < held; ++j, ++out) {
			const nh_QNear e = list[j * stride];
			const nh_QPoint h = Q.to(rec[e.c], e.c < nbox);
			nh_q_write_point(out, rec, nbox, true, e.c, e.key, h.n, h.x);
		}
		// (one cursor through both loops: with out[j] the kernel compiles to 13 more VGPRs and a wave less)
		for (uint32_t j = held; j < k; ++j, ++out) nh_q_write_point(out, rec, nbox, Q.ok, NH_Q_NONE, Q.max_d, nh_make3(0.0f, 0.0f, 0.0f), nh_make3(0.0f, 0.0f, 0.0f));
		if (counts) counts[i] = held;
	}
}

// ---- distance ---------------------------------------------------------------------------------------------------------------------------------
// nh_distance: one lane per query shape on nh_q_walk, k_q_closest with a volume in place of the point.
//   decode  nh_QVolume: the shape, its validity (nh_overlap's, and max_distance >= 0), the half axis of a capsule, the world AABB [qlo, qhi] (not padded)
//   bound   bd starts at max_distance and only ever falls to the key of a real candidate (nh_q_point_key of the pair function's separation and the gap to
//           the collider's own leaf box, nh_q_closer), so a node at squared gap g2 > 0 from the query's AABB with sqrtf(g2) > bd can be skipped: the gap is
//           monotone from a leaf box to every box that contains it (nh_q_dist_node), and a collider's key is at least sqrtf of its leaf's gap
//   seed    nh_q_seed at the query's centre, k_q_closest's window
//   leaf    the pair function of nh_query.h, "distance"; one instantiation serves every shape, the lanes of a wave diverge by the shapes of neighbouring
//           queries and colliders (the box / box enumeration sets the registers)
template <bool FILTER>
__global__ __launch_bounds__(256) void k_q_distance(const nh_DistanceQuery* __restrict__ queries, uint32_t count, nh_PointHit* __restrict__ hits,
                                                    const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec, const uint64_t* __restrict__ keys,
                                                    const nh_QCtl* __restrict__ ctl, uint32_t n, uint32_t nbox, nh_QFilter F) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
		const float4* qp = reinterpret_cast<const float4*>(queries + i);
		nh_QVolume v;
		v.read(qp);
		const float max_d = qp[3].x;          // (the record moves as four 16-byte words; of the fourth only .x is used: `reserved` takes part in nothing)
		const bool ok = v.ok && max_d >= 0.0f;
		const nh_f3 qlo = v.c - v.e, qhi = v.c + v.e;
		float bd = max_d;
		uint32_t bc = NH_Q_NONE;
		nh_f3 bn = nh_make3(0.0f, 0.0f, 0.0f), bx = nh_make3(0.0f, 0.0f, 0.0f);
		const bool walk = ok && n;
		const uint32_t fm = FILTER ? F.of(i) : 0u;
		// a leaf at squared box gap g2, for the seed and the walk alike
		const auto leaf = [&](uint32_t cc, const nh_QRec& r, float g2) {
			const nh_QShape s = nh_q_unpack(r);
			nh_QPoint d;
			if (v.capsule) d = cc < nbox ? nh_q_dist_capsule_box_a(v.c, v.a, v.h.x, s.p, s.q, s.h) : nh_q_dist_capsule_sphere_a(v.c, v.a, v.h.x, s.p, s.h.x);
			else if (cc < nbox) d = v.sphere ? nh_q_dist_sphere_box(v.c, v.h.x, s.p, s.q, s.h) : nh_q_dist_box_box(v.c, v.q, v.h, s.p, s.q, s.h);
			else d = v.sphere ? nh_q_dist_sphere_sphere(v.c, v.h.x, s.p, s.h.x) : nh_q_dist_box_sphere(v.c, v.q, v.h, s.p, s.h.x);
			const float k = nh_q_point_key(d.d, g2);
			if (nh_q_closer(k, cc, max_d, bd, bc)) { bd = k; bc = cc; bn = d.n; bx = d.x; }
			return false;
		};
		if (walk) nh_q_seed<FILTER>(v.c, NH_Q_SEED, v.ignore, nodes, rec, keys, ctl, n, F, fm, [&](uint32_t cc, const nh_QRec& r, nh_f3 lo, nh_f3 hi) { leaf(cc, r, nh_q_dist_node(lo, hi, qlo, qhi)); });
		nh_q_walk<FILTER>(nodes, rec, walk ? 0u : NH_Q_NONE, v.ignore, F, fm,
			[&](nh_f3 lo, nh_f3 hi, float& g2) { g2 = nh_q_dist_node(lo, hi, qlo, qhi); return !(g2 > 0.0f && sqrtf(g2) > bd); }, leaf);
		nh_q_write_point(hits + i, rec, nbox, ok, bc, bd, bn, bx);
	}
}

// ---- overlap ---------------------------------------------------------------------------------------------------------------------------------
// nh_overlap is a chain of launches with kernel boundaries as the only hand-offs; no atomic decides where a record goes:
//   k_q_overlap<false, false>  one lane per query: nh_q_walk (stackless, escape links) with the query's padded world AABB as the node test, the exact
//                       predicate at the leaves; offsets[i] = the count (offsets[count] = 0, scanned along)
//   k_q_overlap<false, true>   the same for the capsule queries of nonzero half height, which the first skips: their predicates need more registers
//                       than the sphere and box walk's occupancy allows, so they run in an instantiation of their own
//   nh_scan_u32         in place over count + 1 words: offsets and the total
//   k_q_overlap_fix     the wrap (offsets[i+1] < offsets[i]) and the written prefix: the one i with offsets[i] <= capacity < offsets[i+1], or the total
//   k_q_overlap_fin     one lane: on a wrap or a total equal to the marker, offsets[count] = 0xffffffff and nothing is written
//   k_q_overlap<true, *> the same walks (the same template: the same set) for the queries whose segment fits: key (i << cbits | c), value c at offsets[i] + k
//   nh_sort_u64_u32     over the written prefix (its length from the device): keys are unique, so (query, combined index) ascending is the only order
//   k_q_overlap_gather  nh_OverlapHit {body, collider, shape, tag} from the record of each sorted collider, one 16-byte store each
template <bool LIST, bool CAPSULE, bool FILTER>
__global__ __launch_bounds__(256) void k_q_overlap(const nh_OverlapQuery* __restrict__ queries, uint32_t count, uint32_t* offsets,
                                                   const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox,
                                                   nh_QCtl* ctl, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t cbits, nh_QFilter F) {
	const uint32_t written = nh_QSegment<LIST>::begin(!CAPSULE, offsets, count, ctl);
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
		nh_QSegment<LIST> seg;
		if (!seg.open(offsets, i, written)) continue;
		nh_QVolume v;
		v.read(reinterpret_cast<const float4*>(queries + i));
		// (a capsule of half height 0 is a sphere query: the same walk, the same predicates.  Every other capsule -- an invalid half height included -- is
		// the CAPSULE instantiation's, and only its; each instantiation drops the other's predicates at compile time)
		if (v.capsule != CAPSULE) continue;
		const bool capsule = CAPSULE, sphere = !CAPSULE && v.sphere;
		// the query's world AABB, padded by 2^-18 of its largest coordinate (only ever more generous than the exact test)
		nh_f3 lo = v.c - v.e, hi = v.c + v.e;
		const float s = fmaxf(fmaxf(fmaxf(fabsf(lo.x), fabsf(lo.y)), fmaxf(fabsf(lo.z), fabsf(hi.x))), fmaxf(fabsf(hi.y), fabsf(hi.z))) * 3.814697265625e-06f;
		lo = nh_make3(lo.x - s, lo.y - s, lo.z - s); hi = nh_make3(hi.x + s, hi.y + s, hi.z + s);
		nh_q_walk<FILTER>(nodes, rec, v.ok && n ? 0u : NH_Q_NONE, v.ignore, F, FILTER ? F.of(i) : 0u,
			[&](nh_f3 nlo, nh_f3 nhi, float&) { return nlo.x <= hi.x && lo.x <= nhi.x && nlo.y <= hi.y && lo.y <= nhi.y && nlo.z <= hi.z && lo.z <= nhi.z; },
			[&](uint32_t cc, const nh_QRec& r, float) {
				const nh_QShape col = nh_q_unpack(r);
				bool hit;
				if (capsule) hit = cc < nbox ? nh_q_overlap_capsule_box_a(v.c, v.a, v.h.x, col.p, col.q, col.h) : nh_q_overlap_capsule_sphere_a(v.c, v.a, v.h.x, col.p, col.h.x);
				else if (cc < nbox) hit = sphere ? nh_q_overlap_sphere_box(v.c, v.h.x, col.p, col.q, col.h) : nh_q_overlap_box_box(v.c, v.q, v.h, col.p, col.q, col.h);
				else hit = sphere ? nh_q_overlap_sphere_sphere(v.c, v.h.x, col.p, col.h.x) : nh_q_overlap_sphere_box(col.p, col.h.x, v.c, v.q, v.h);
				if (!hit) return false;
				if (LIST) { keys[seg.at()] = ((uint64_t)i << cbits) | cc; vals[seg.at()] = cc; }
				return seg.add();
			});
		if (!LIST) offsets[i] = seg.k;
	}
}

__global__ __launch_bounds__(256) void k_q_overlap_fix(const uint32_t* __restrict__ offsets, uint32_t count, uint32_t capacity, nh_QCtl* __restrict__ ctl) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= count; i += gridDim.x * blockDim.x) {
		const uint32_t lo = offsets[i];
		if (i == count) {
			if (lo <= capacity) ctl->ov_written = lo;             // everything fits
			continue;
		}
		const uint32_t hi = offsets[i + 1u];
		if (hi < lo) ctl->ov_wrap = 1u;                            // (every store writes the same word)
		else if (lo <= capacity && capacity < hi) ctl->ov_written = lo;   // monotone offsets: exactly one lane, when there is no wrap
	}
}

__global__ void k_q_overlap_fin(uint32_t* __restrict__ offsets, uint32_t count, nh_QCtl* __restrict__ ctl) {
	if (ctl->ov_wrap || offsets[count] == NH_Q_NONE) { offsets[count] = NH_Q_NONE; ctl->ov_written = 0u; }
}

__global__ __launch_bounds__(256) void k_q_overlap_gather(const uint32_t* __restrict__ vals, const nh_QCtl* __restrict__ ctl, const nh_QRec* __restrict__ rec,
                                                          uint32_t n, uint32_t nbox, nh_OverlapHit* __restrict__ hits) {
	const uint32_t m = ctl->ov_written;
	for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
		const uint32_t c = vals[j];
		if (c >= n) continue;          // (cannot happen: the list pass fills the whole prefix; a guard against reading outside the records)
		*reinterpret_cast<uint4*>(hits + j) = nh_q_identity(c, nbox, rec[c]);
	}
}

// nh_penetration's gather: one lane per written record.  The sort carries keys and values, so the query index is the sorted key's upper part
// (key >> cbits) and the collider the sorted value: the lane re-reads the 48-byte query and the 48-byte collider record, evaluates the pair function
// (nh_query.h, "penetration") under the query decode of k_q_overlap, and writes {normal, depth} and nh_OverlapHit's four words as two 16-byte stores.
// Records are sorted by query and, within a query, boxes come before spheres: a wave diverges only by the shape mix of neighbouring queries.  One
// instantiation serves every shape (the capsule / box function sets the register count at 7 of 8 waves per SIMD, and a lane does one
// record -- 140 bytes moved, no loop for occupancy to pay for).
__global__ __launch_bounds__(256) void k_q_penetration_gather(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, const nh_QCtl* __restrict__ ctl,
                                                              const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox,
                                                              const nh_OverlapQuery* __restrict__ queries, uint32_t count, uint32_t cbits,
                                                              nh_PenetrationHit* __restrict__ hits) {
	const uint32_t m = ctl->ov_written;
	for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
		const uint32_t cc = vals[j];
		const uint64_t i = keys[j] >> cbits;
		if (cc >= n || i >= count) continue;          // (cannot happen: the list pass fills the whole prefix; a guard against reading outside the records)
		nh_QVolume v;
		v.read(reinterpret_cast<const float4*>(queries + i));
		const nh_QRec r = rec[cc];
		const nh_QShape s = nh_q_unpack(r);
		nh_QPen o;
		if (v.capsule) o = cc < nbox ? nh_q_pen_capsule_box_a(v.c, v.a, v.h.x, s.p, s.q, s.h) : nh_q_pen_capsule_sphere_a(v.c, v.a, v.h.x, s.p, s.h.x);
		else if (cc < nbox) o = v.sphere ? nh_q_pen_sphere_box(v.c, v.h.x, s.p, s.q, s.h) : nh_q_pen_box_box(v.c, v.q, v.h, s.p, s.q, s.h);
		else o = v.sphere ? nh_q_pen_sphere_sphere(v.c, v.h.x, s.p, s.h.x) : nh_q_pen_box_sphere(v.c, v.q, v.h, s.p, s.h.x);
		uint4* out = reinterpret_cast<uint4*>(hits + j);
		out[0] = make_uint4(__float_as_uint(o.n.x), __float_as_uint(o.n.y), __float_as_uint(o.n.z), __float_as_uint(o.depth));
		out[1] = nh_q_identity(cc, nbox, r);
	}
}

// ---- recover ----------------------------------------------------------------------------------------------------------------------------------
// nh_recover: one lane per query.  The state machine is nh_query.h's ("recover": nh_q_recover_begin / _better / _advance, which the host's brute force runs
// as well).  The record's first 48 bytes go through nh_QVolume, k_q_overlap's decode; a round is k_q_overlap's walk with the shape at p -- p finite, the
// padded world AABB of k_q_overlap as the node test, its predicate at the leaf -- and, where the predicate accepts, the pair function
// k_q_penetration_gather picks for that pair; nh_q_recover_better keeps the deepest.  So a round's set is nh_overlap's for the shape at p and its (normal,
// depth) nh_penetration's, under the same mask (the query's index).  Capsules of nonzero half height run in an instantiation of their own, as in k_q_overlap:
// each writes the results of its own queries, every query is exactly one's.  The loop bound is a constant and every round is a walk that terminates, so the
// kernel terminates on any input.  A lane whose recover has ended waits for the slowest of its wave.  The result leaves as four 16-byte
// stores, the last two the nh_PenetrationHit of the last pair kept (nh_q_identity of its collider).
static_assert(NH_Q_RECOVER_PUSHED == NH_RECOVER_PUSHED && NH_Q_RECOVER_OVERLAPPING == NH_RECOVER_OVERLAPPING && NH_Q_RECOVER_TOUCHING == NH_RECOVER_TOUCHING &&
              NH_Q_RECOVER_MAX_ITERATIONS == NH_RECOVER_MAX_ITERATIONS, "nh_query.h's recover constants are the header's");
static_assert(sizeof(nh_Recover) == 64 && sizeof(nh_RecoverResult) == 64 && sizeof(nh_OverlapQuery) == 48 && sizeof(nh_PenetrationHit) == 32,
              "nh_Recover is nh_OverlapQuery and one more 16-byte word, nh_RecoverResult two words and an nh_PenetrationHit");

template <bool CAPSULE, bool FILTER>
__global__ __launch_bounds__(256) void k_q_recover(const nh_Recover* __restrict__ queries, uint32_t count, nh_RecoverResult* __restrict__ results,
                                                   const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox, nh_QFilter F) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
		const float4* qp = reinterpret_cast<const float4*>(queries + i);
		nh_QVolume v;
		v.read(qp);
		if (v.capsule != CAPSULE) continue;
		const float4 q3 = qp[3];
		const float skin = q3.x;
		const uint32_t max_iterations = __float_as_uint(q3.y);
		const bool capsule = CAPSULE, sphere = !CAPSULE && v.sphere;
		const bool valid = v.ok && nh_q_recover_valid(skin, max_iterations);
		const uint32_t fm = FILTER ? F.of(i) : 0u;
		nh_QRecover s = nh_q_recover_begin(v.c);
		float ld = 0.0f;
		uint32_t lc = NH_Q_NONE;
		nh_f3 ln = nh_make3(0.0f, 0.0f, 0.0f);
		for (uint32_t round = 0u; round <= NH_RECOVER_MAX_ITERATIONS; ++round) {
			if (!valid) break;
			const nh_f3 c = s.p;
			// the shape's world AABB at p, padded by 2^-18 of its largest coordinate: k_q_overlap's node test
			nh_f3 lo = c - v.e, hi = c + v.e;
			const float pad = fmaxf(fmaxf(fmaxf(fabsf(lo.x), fabsf(lo.y)), fmaxf(fabsf(lo.z), fabsf(hi.x))), fmaxf(fabsf(hi.y), fabsf(hi.z))) * 3.814697265625e-06f;
			lo = nh_make3(lo.x - pad, lo.y - pad, lo.z - pad); hi = nh_make3(hi.x + pad, hi.y + pad, hi.z + pad);
			float bd = 0.0f;
			uint32_t bc = NH_Q_NONE;
			nh_f3 bn = nh_make3(0.0f, 0.0f, 0.0f);
			nh_q_walk<FILTER>(nodes, rec, nh_q_finite(c) && n ? 0u : NH_Q_NONE, v.ignore, F, fm,
				[&](nh_f3 nlo, nh_f3 nhi, float&) { return nlo.x <= hi.x && lo.x <= nhi.x && nlo.y <= hi.y && lo.y <= nhi.y && nlo.z <= hi.z && lo.z <= nhi.z; },
				[&](uint32_t cc, const nh_QRec& r, float) {
					const nh_QShape col = nh_q_unpack(r);
					bool hit;
					if (capsule) hit = cc < nbox ? nh_q_overlap_capsule_box_a(c, v.a, v.h.x, col.p, col.q, col.h) : nh_q_overlap_capsule_sphere_a(c, v.a, v.h.x, col.p, col.h.x);
					else if (cc < nbox) hit = sphere ? nh_q_overlap_sphere_box(c, v.h.x, col.p, col.q, col.h) : nh_q_overlap_box_box(c, v.q, v.h, col.p, col.q, col.h);
					else hit = sphere ? nh_q_overlap_sphere_sphere(c, v.h.x, col.p, col.h.x) : nh_q_overlap_sphere_box(col.p, col.h.x, c, v.q, v.h);
					if (!hit) return false;
					nh_QPen o;
					if (capsule) o = cc < nbox ? nh_q_pen_capsule_box_a(c, v.a, v.h.x, col.p, col.q, col.h) : nh_q_pen_capsule_sphere_a(c, v.a, v.h.x, col.p, col.h.x);
					else if (cc < nbox) o = sphere ? nh_q_pen_sphere_box(c, v.h.x, col.p, col.q, col.h) : nh_q_pen_box_box(c, v.q, v.h, col.p, col.q, col.h);
					else o = sphere ? nh_q_pen_sphere_sphere(c, v.h.x, col.p, col.h.x) : nh_q_pen_box_sphere(c, v.q, v.h, col.p, col.h.x);
					if (nh_q_recover_better(o.depth, cc, bd, bc)) { bd = o.depth; bc = cc; bn = o.n; }
					return false;
				});
			if (bc != NH_Q_NONE) { ld = bd; lc = bc; ln = bn; }
			if (!nh_q_recover_advance(s, bc != NH_Q_NONE, bd, bn, skin, max_iterations)) break;
		}
		float4* out = reinterpret_cast<float4*>(results + i);
		const nh_f3 push = valid ? s.p - v.c : nh_make3(0.0f, 0.0f, 0.0f);
		out[0] = make_float4(s.p.x, s.p.y, s.p.z, __uint_as_float(valid ? s.flags : (uint32_t)NH_RECOVER_INVALID));
		out[1] = make_float4(push.x, push.y, push.z, __uint_as_float(s.iterations));
		out[2] = make_float4(ln.x, ln.y, ln.z, ld);
		reinterpret_cast<uint4*>(out)[3] = lc != NH_Q_NONE ? nh_q_identity(lc, nbox, rec[lc]) : make_uint4(NH_Q_NONE, NH_Q_NONE, NH_SHAPE_NONE, NH_Q_NONE);
	}
}

// ---- region -----------------------------------------------------------------------------------------------------------------------------------
// nh_region: the colliders inside each of `count` convex regions (nh_query.h, "region").  No lane owns a region: a WORK ITEM is (region, entry node), the
// entry nodes being nh_QueryState::top -- the roots of disjoint subtrees, each inside one run of NH_Q_RUN consecutive leaves, every leaf below exactly one
// of them (k_q_tree lists the children, inside one run, of every node that crosses a run boundary; the root crosses iff n > NH_Q_RUN).  A tree of one run
// has no such list: its one entry is the root.  An entry may be a leaf.  top_n lives on the device, so the grid is capped and the items, region-major, are
// dealt to the waves in chunks of `ch` consecutive ones, ch = ceil(items / waves) clamped to 1 .. 64: few items spread over many waves, many fill the lanes.
//   node test  one LANE per item of the chunk: the region's validity (nh_q_region_valid), under the filter the entry's layer word, then the entry's box
//              against each plane (nh_q_region_node_outside: a margin of 2^-18 of |n| times the box's coordinates plus |d|; only a TRUE comparison
//              prunes).  Outside any plane: the item is done after one node load.  The list pass takes the regions inside the written prefix only.
//   leaf sweep one WAVE per item that is left, one after the other: its region and entry go to scalar registers (readlane), and with them the planes --
//              every lane reads them at one address.  The entry's leaves are contiguous: [first, last[e]], the entry's own index being one end of its
//              range (Karras), so first = e unless last[e] == e, and then a leftmost descent finds it.  64 leaves a step: idx[j] coalesced, rec[idx[j]]
//              gathered, `ignore_body`, the leaf's layer word (FILTER), the exact predicate -- on every leaf, also where the entry's box lies wholly inside:
//              that keeps the NaN poses out and needs no second margin.
//   count      ballot and popcount per step, summed in a scalar register; one integer atomic per item on offsets[region] (zeroed at the head of the chain).
//              Integer sums do not depend on their order: the counts are deterministic.
//   list       per step, one atomic on the region's cursor reserves popcount slots of its segment; key (region << cbits) | c, value c.  Slot order is
//              arbitrary; nh_overlap's sort over the written prefix and k_q_overlap_gather make the bytes deterministic.
// No LDS, no barrier, no walk.  (registers and occupancy.)
static_assert(sizeof(nh_Region) == 144 && NH_REGION_MAX_PLANES == NH_Q_REGION_MAX_PLANES, "nh_Region is nine 16-byte words; nh_query.h's plane bound is the header's");
#define NH_Q_REGION_GRID 2048u

// The volume of an item loop (nh_q_items, below).  valid(i): one lane decodes volume i for the node test and says whether it can list anything at all;
// enters(lo, hi): false only where nothing in that box can be kept; sweep(i): i is wave-uniform, so every lane reads the volume at one address; keeps():
// the exact per-collider decision; ignore: the volume's ignore_body.
// nh_Region: the planes.
struct nh_QPlanes {
	const nh_Region* __restrict__ regions;
	const float* pl;
	uint32_t pc, ignore;
	__device__ __forceinline__ bool valid(uint32_t i) {
		pl = &regions[i].planes[0][0];
		pc = regions[i].plane_count;
		return nh_q_region_valid(pl, pc);
	}
	__device__ __forceinline__ bool enters(nh_f3 lo, nh_f3 hi) const {
		bool in = true;
		for (uint32_t k = 0u; k < pc; ++k)
			if (nh_q_region_node_outside(nh_make3(pl[4u * k], pl[4u * k + 1u], pl[4u * k + 2u]), pl[4u * k + 3u], lo, hi)) in = false;
		return in;
	}
	__device__ __forceinline__ void sweep(uint32_t i) {
		pl = &regions[i].planes[0][0];
		pc = regions[i].plane_count; ignore = regions[i].ignore_body;
	}
	__device__ __forceinline__ bool keeps(const nh_QShape& s, bool box) const { return nh_q_region_keeps(pl, pc, s.p, s.q, s.h, box); }
};

// nh_OverlapQuery, for nh_overlap_wide / nh_penetration_wide: k_q_overlap's geometry.  The decode is nh_QVolume; the node test is the query's world AABB
// padded by 2^-18 of its largest coordinate against the box -- the expressions of k_q_overlap's `enter`, applied to the entry node alone -- and keeps() is
// the predicate k_q_overlap picks for the shape pair.  CAPSULE: as in k_q_overlap, the capsules of nonzero half height (an invalid half height included)
// run in an instantiation of their own and the other takes the spheres and boxes; one kernel for every shape needs 86 to 91 VGPRs, 5 waves per SIMD
// where the two have 7.  A launch takes its own queries and adds nothing for the others.  In the sweep the shape is wave-uniform, so the
// shape branch of keeps() is one branch for the wave.
template <bool CAPSULE>
struct nh_QWide {
	const nh_OverlapQuery* __restrict__ queries;
	nh_QVolume v;
	nh_f3 lo, hi;
	uint32_t ignore;
	__device__ __forceinline__ bool valid(uint32_t i) {
		v.read(reinterpret_cast<const float4*>(queries + i));
		lo = v.c - v.e; hi = v.c + v.e;
		const float s = fmaxf(fmaxf(fmaxf(fabsf(lo.x), fabsf(lo.y)), fmaxf(fabsf(lo.z), fabsf(hi.x))), fmaxf(fabsf(hi.y), fabsf(hi.z))) * 3.814697265625e-06f;
		lo = nh_make3(lo.x - s, lo.y - s, lo.z - s); hi = nh_make3(hi.x + s, hi.y + s, hi.z + s);
		return v.ok && v.capsule == CAPSULE;
	}
	__device__ __forceinline__ bool enters(nh_f3 nlo, nh_f3 nhi) const {
		return nlo.x <= hi.x && lo.x <= nhi.x && nlo.y <= hi.y && lo.y <= nhi.y && nlo.z <= hi.z && lo.z <= nhi.z;
	}
	__device__ __forceinline__ void sweep(uint32_t i) {
		v.read(reinterpret_cast<const float4*>(queries + i));
		ignore = v.ignore;
	}
	__device__ __forceinline__ bool keeps(const nh_QShape& col, bool box) const {
		const bool capsule = CAPSULE, sphere = !CAPSULE && v.sphere;
		if (capsule) return box ? nh_q_overlap_capsule_box_a(v.c, v.a, v.h.x, col.p, col.q, col.h) : nh_q_overlap_capsule_sphere_a(v.c, v.a, v.h.x, col.p, col.h.x);
		if (box) return sphere ? nh_q_overlap_sphere_box(v.c, v.h.x, col.p, col.q, col.h) : nh_q_overlap_box_box(v.c, v.q, v.h, col.p, col.q, col.h);
		return sphere ? nh_q_overlap_sphere_sphere(v.c, v.h.x, col.p, col.h.x) : nh_q_overlap_sphere_box(col.p, col.h.x, v.c, v.q, v.h);
	}
};

// The item loop of k_q_region and k_q_wide (the comment above): `first` -- the chain's first count launch -- resets the words k_q_overlap_fix sets; wpb: the
// kernel's waves per workgroup (blockDim.x >> 6, read in the kernel itself).
template <bool LIST, bool FILTER, class Vol>
__device__ __forceinline__ void nh_q_items(const Vol V, bool first, uint32_t wpb, uint32_t count, uint32_t* offsets, const nh_QNode* __restrict__ nodes,
                                           const nh_QRec* __restrict__ rec, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ last,
                                           const uint32_t* __restrict__ top, uint32_t n, uint32_t nbox, nh_QCtl* ctl, uint32_t* __restrict__ cursor,
                                           uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t cbits, const nh_QFilter& F) {
	if (!LIST && first && blockIdx.x == 0 && threadIdx.x == 0) { ctl->ov_wrap = 0u; ctl->ov_written = 0u; }   // (k_q_overlap_fix sets both)
	const uint32_t written = LIST ? ctl->ov_written : 0u;
	const uint32_t entries = n > NH_Q_RUN ? ctl->top_n : (n ? 1u : 0u);
	const uint64_t total = (uint64_t)count * entries;
	const uint32_t lane = nh_lane();
	const uint64_t waves = (uint64_t)gridDim.x * wpb;
	const uint64_t per = (total + waves - 1u) / waves;
	const uint32_t ch = per > 64u ? 64u : (uint32_t)per;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * wpb + (threadIdx.x >> 6));
	for (uint64_t item0 = (uint64_t)wave * ch; item0 < total; item0 += waves * ch) {
		// ---- node test: lane l takes item item0 + l
		const uint64_t item = item0 + lane;
		uint32_t ri = 0u, node = 0u;
		bool live = lane < ch && item < total;
		if (live) {
			ri = (uint32_t)(item / entries);
			const uint32_t e = (uint32_t)(item - (uint64_t)ri * entries);
			if (LIST) {
				const uint32_t base = offsets[ri], end = offsets[ri + 1u];
				live = base < end && end <= written;
			}
			if (live) {
				Vol t = V;
				live = t.valid(ri);
				node = n > NH_Q_RUN ? top[e] : 0u;
				if (node >= 2u * n - 1u) live = false;          // (cannot happen: a guard against reading outside the nodes)
				if (FILTER && live) live = F.sees(node, F.of(ri));
				if (live) {
					const float4 na = nodes[node].a, nb = nodes[node].b;
					live = t.enters(nh_make3(na.x, na.y, na.z), nh_make3(nb.x, nb.y, nb.z));
				}
			}
		}
		// ---- leaf sweep: the wave takes the items left, one after the other
		uint64_t todo = __ballot(live);
		while (todo) {
			const int src = __ffsll((long long)todo) - 1;
			todo &= todo - 1ull;
			const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)ri, src), e = (uint32_t)__builtin_amdgcn_readlane((int)node, src);
			uint32_t jf, jl;
			if (e >= n - 1u) jf = jl = e - (n - 1u);            // the entry is a leaf
			else {
				jl = last[e];
				uint32_t u = e;
				if (jl == e) while (u < n - 1u) u = __float_as_uint(nodes[u].a.w);      // leftmost descent (internal nodes carry their left child's id there)
				jf = jl == e ? u - (n - 1u) : e;
			}
			if (jl >= n) jl = n - 1u;                           // (cannot happen; the sweep stays inside idx)
			Vol t = V;
			t.sweep(r);
			const uint32_t fm = FILTER ? F.of(r) : 0u;
			const uint32_t seg = LIST ? offsets[r] : 0u, seg_end = LIST ? offsets[r + 1u] : 0u;
			uint32_t found = 0u;
			for (uint32_t j0 = jf; j0 <= jl; j0 += 64u) {
				const uint32_t j = j0 + lane;
				bool keep = false;
				uint32_t c = 0u;
				if (j <= jl) {
					c = idx[j];
					if (c < n && (!FILTER || F.sees(n - 1u + j, fm))) {
						const nh_QRec q = rec[c];
						if (__float_as_uint(q.a.w) != t.ignore) keep = t.keeps(nh_q_unpack(q), c < nbox);
					}
				}
				const uint64_t bal = __ballot(keep);
				if (!LIST) found += (uint32_t)__popcll(bal);
				else if (bal) {
					uint32_t at = 0u;
					if (lane == 0u) at = atomicAdd(&cursor[r], (uint32_t)__popcll(bal));
					at = seg + (uint32_t)__shfl((int)at, 0) + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
					// (at < seg_end: the count pass found the same set; a guard against writing outside the volume's segment)
					if (keep && at < seg_end) { keys[at] = ((uint64_t)r << cbits) | c; vals[at] = c; }
				}
			}
			if (!LIST && found && lane == 0u) atomicAdd(&offsets[r], found);
		}
	}
}

template <bool LIST, bool FILTER>
__global__ __launch_bounds__(256) void k_q_region(const nh_Region* __restrict__ regions, uint32_t count, uint32_t* offsets, const nh_QNode* __restrict__ nodes,
                                                  const nh_QRec* __restrict__ rec, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ last,
                                                  const uint32_t* __restrict__ top, uint32_t n, uint32_t nbox, nh_QCtl* ctl, uint32_t* __restrict__ cursor,
                                                  uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t cbits, nh_QFilter F) {
	nh_QPlanes V;
	V.regions = regions;
	nh_q_items<LIST, FILTER>(V, true, blockDim.x >> 6, count, offsets, nodes, rec, idx, last, top, n, nbox, ctl, cursor, keys, vals, cbits, F);
}

// ---- wide overlap -----------------------------------------------------------------------------------------------------------------------------
// nh_overlap_wide / nh_penetration_wide: nh_overlap's and nh_penetration's bytes for volumes too large for a lane -- k_q_region's decomposition (a work
// item is (query, entry node); a lane per node test, a wave per leaf sweep; ballot counts, an integer atomic per item on offsets[query], one per step
// on the query's cursor) with k_q_overlap's geometry (nh_QWide).  The set is nh_overlap's: the entry's box is tested by the expressions of k_q_overlap's
// walk, which never prune what the predicates accept, and below an entry every leaf meets the predicate itself, which rejects a NaN pose.
// The atomics decide slots inside a segment only; nh_overlap's sort and gathers decide the bytes.  (registers, occupancy, rates.)
template <bool LIST, bool CAPSULE, bool FILTER>
__global__ __launch_bounds__(256) void k_q_wide(const nh_OverlapQuery* __restrict__ queries, uint32_t count, uint32_t* offsets, const nh_QNode* __restrict__ nodes,
                                                const nh_QRec* __restrict__ rec, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ last,
                                                const uint32_t* __restrict__ top, uint32_t n, uint32_t nbox, nh_QCtl* ctl, uint32_t* __restrict__ cursor,
                                                uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t cbits, nh_QFilter F) {
	nh_QWide<CAPSULE> V;
	V.queries = queries;
	nh_q_items<LIST, FILTER>(V, !CAPSULE, blockDim.x >> 6, count, offsets, nodes, rec, idx, last, top, n, nbox, ctl, cursor, keys, vals, cbits, F);
}

// ---- all-hits casts ---------------------------------------------------------------------------------------------------------------------------
// nh_raycast_all / nh_spherecast_all / nh_boxcast_all / nh_capsulecast_all: every collider a cast passes through, ordered along the cast.  nh_overlap's chain (kernel boundaries are the
// only hand-offs, no atomic decides where a record goes) with the casts' walk in place of the volume walk and an ordering by t behind it:
//   k_q_castall<S, false>  one lane per cast: the decode and node test of the shape S (nh_QRay, nh_QBall, nh_QBox, nh_QCapsule) in nh_q_walk, with the pruning
//                       bound FIXED at max_t -- there is no best hit to tighten it -- and S::all at every entered leaf; offsets[i] = the number of hits.
//                       For a ray-like shape (a ray, r = 0, a box of size 0, a capsule of r = hh = 0) every node box is grown by nh_q_all_pad as well: the
//                       set is every collider the PREDICATE accepts, and the closest-hit walk's pad does not cover the predicates' rounding at a distance
//                       (nh_query.h).  A shape with a size needs none: its reach rule makes the set a function of the leaf test
//   nh_scan_u32, k_q_overlap_fix, k_q_overlap_fin   nh_overlap's own (nh_overlap_offsets)
//   k_q_castall<S, true>   the same walk (the same template: the same set) for the casts whose segment fits; hit k of cast i goes to offsets[i] + k
//   the ordering by (cast, t, combined collider index), one of
//     ONE SORT   where bits(count) + 32 + cbits <= 64: key (i << (32 + cbits)) | (tbits << cbits) | c, value c, one nh_sort_u64_u32
//     TWO SORTS  otherwise (a million rays on a million colliders need 72 bits): key (i << cbits) | c, value tbits; nh_sort_u64_u32 over the cbits of c
//                (LSD: the least significant part first); k_q_castall_rekey to key (i << 32) | tbits, value c; a second, stable nh_sort_u64_u32 over
//                32 + bits(count) bits, whose stability carries the index order into the ties of t
//   k_q_castall_gather<S>  one lane per written record: the cast index from the key, the collider from the value; it re-reads the cast and the 48-byte
//                       collider record and evaluates S::all again -- the same function on the same inputs, the leaf entry of the reach rule
//                       rebuilt by S::entry (nh_q_leaf_entry / nh_q_leaf_entry3) as the build stores it -- and writes nh_RayHit as two 16-byte stores.  No
//                       normal goes through a sort.
// every shape's decode, validity and grow are the closest-hit casts' own: a shape without a size gives the ray's bytes, a capsule of hh = 0 the ball's, and
// the first record of a cast is the closest-hit record.  The box and capsule instantiations take their closest-hit siblings' waves-per-EU hint (ALL_WAVES)
// The node test of "every hit up to `bound`" (max_t for the all-hits casts, the k-th t so far for the first-k casts); ray = k.raylike().  A ray's node box
// also takes the predicates' own rounding, nh_q_all_pad; a sized shape's reach rule reads the entry of the box as the build stores it.
template <class Shape>
__device__ __forceinline__ bool nh_q_all_node(const Shape& k, bool ray, nh_f3 lo, nh_f3 hi, float bound, float& t0) {
	if (ray) return nh_q_cast_node(lo, hi, k.o, k.inv, k.grow() + nh_q_all_pad(lo, hi, k.o), t0) && t0 <= bound;
	return k.node(lo, hi, t0) && t0 <= bound;
}

// The record of a collider c the walk of cast k listed, rebuilt where no walk is at hand: the 48-byte collider record re-read, the leaf entry of the reach
// rule from S::entry, S::all again -- the same function on the same inputs, the same bits -- and out through nh_q_write_hit.
template <class Shape>
__device__ __forceinline__ void nh_q_rebuild_hit(const Shape& k, uint32_t c, nh_RayHit* __restrict__ hit, const nh_QRec* __restrict__ rec, uint32_t nbox) {
	const nh_QShape s = nh_q_unpack(rec[c]);
	float t0 = 0.0f;
	k.entry(s, c < nbox, t0);                          // (entered: the walk listed it)
	const nh_QHit h = k.all(s, c < nbox, t0);
	nh_q_write_hit(hit, rec, nbox, true, c, h.t, h.n);
}

template <class Shape, bool LIST, bool FILTER>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(Shape::ALL_WAVES))) void k_q_castall(const float4* __restrict__ casts, uint32_t count, uint32_t* offsets,
                                                   const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox,
                                                   nh_QCtl* ctl, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t cbits, uint32_t one_sort, nh_QFilter F) {
	const uint32_t written = nh_QSegment<LIST>::begin(true, offsets, count, ctl);
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
		nh_QSegment<LIST> seg;
		if (!seg.open(offsets, i, written)) continue;
		Shape k;
		k.read(casts + (size_t)i * Shape::WORDS);
		const bool ray = k.raylike();
		nh_q_walk<FILTER>(nodes, rec, k.ok && n ? 0u : NH_Q_NONE, k.ignore, F, FILTER ? F.of(i) : 0u,
			[&](nh_f3 lo, nh_f3 hi, float& t0) { return nh_q_all_node(k, ray, lo, hi, k.max_t, t0); },
			[&](uint32_t c, const nh_QRec& q, float t0) {
				const nh_QHit h = k.all(nh_q_unpack(q), c < nbox, t0);
				if (!h.hit) return false;
				if (LIST) {
					const uint32_t tb = nh_q_tbits(h.t);
					keys[seg.at()] = one_sort ? ((uint64_t)i << (32u + cbits)) | ((uint64_t)tb << cbits) | c : ((uint64_t)i << cbits) | c;
					vals[seg.at()] = one_sort ? c : tb;
				}
				return seg.add();
			});
		if (!LIST) offsets[i] = seg.k;
	}
}

// between the two sorts: (i << cbits | c, tbits) becomes (i << 32 | tbits, c), in place
__global__ __launch_bounds__(256) void k_q_castall_rekey(uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, const nh_QCtl* __restrict__ ctl, uint32_t cbits) {
	const uint32_t m = ctl->ov_written;
	for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
		const uint64_t key = keys[j];
		const uint32_t tb = vals[j];
		keys[j] = ((key >> cbits) << 32) | tb;
		vals[j] = (uint32_t)(key & ((1ull << cbits) - 1ull));
	}
}

template <class Shape>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(Shape::ALL_WAVES))) void k_q_castall_gather(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, const nh_QCtl* __restrict__ ctl,
                                                          const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox,
                                                          const float4* __restrict__ casts, uint32_t count, uint32_t ishift, nh_RayHit* __restrict__ hits) {
	const uint32_t m = ctl->ov_written;
	for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
		const uint32_t c = vals[j];
		const uint64_t i = keys[j] >> ishift;
		if (c >= n || i >= count) continue;          // (cannot happen: the list pass fills the whole prefix; a guard against reading outside the records)
		Shape k;
		k.read(casts + (size_t)i * Shape::WORDS);
		nh_q_rebuild_hit(k, c, hits + j, rec, nbox);
	}
}

// ---- first-k casts ------------------------------------------------------------------------------------------------------------------------------
// nh_raycast_k / nh_spherecast_k / nh_boxcast_k / nh_capsulecast_k: the first k records of the all-hits segment of each cast, in ONE launch.  One lane
// per cast on nh_q_walk, the decode, node test and per-collider decision (S::all) of k_q_castall, and k_q_closest_k's list in place of the count:
//   list   nh_QNear / nh_q_nearest_insert (nh_query.h) unchanged, key = t, max_d = max_t.  Its order, nh_q_closer, is ascending key as floats (-0 equals
//          +0), ties to the lower combined index: the all-hits order.  In LDS, slot-major: entry j of lane l at lds[j * blockDim.x + l], dynamic shared
//          memory of blockDim.x * k * 8 bytes, the block size from nh_q_nearest_block(k) (the table at k_q_closest_k); no register array is indexed
//          dynamically.  A lane that takes another cast (the grid is capped) starts again from held = 0: nothing of the last list is read.
//   bound  bd, in a register: max_t while fewer than k are held, the k-th t once the list is full, reloaded from the last slot after an insert that
//          changed a full list.  The node test is k_q_castall's with bd in place of max_t; a leaf whose t is not <= bd is dropped by that one compare
//          without touching LDS (equality goes on: a tie can still win by index).
//   exact  DESIGN 10.13: bd is never below the final k-th t, and the entry t0 of every ancestor of a listed collider is at most the collider's t.
//   out    the list holds (t, index) only: each held entry is rebuilt as k_q_castall_gather rebuilds a record (the record re-read, S::entry, S::all --
//          the same function on the same inputs, the same bits) and leaves through nh_q_write_hit; the k - held miss records follow (t = max_t, or a
//          quiet NaN for an invalid cast: the closest-hit call's miss), then counts[i] = held.  No normal is kept in LDS.
// The box and capsule instantiations take their siblings' waves-per-EU hint (ALL_WAVES).
template <class Shape, bool FILTER>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(Shape::K_WAVES))) void k_q_cast_k(const float4* __restrict__ casts, uint32_t count, uint32_t kk,
                                                   uint32_t* __restrict__ counts, nh_RayHit* __restrict__ hits, const nh_QNode* __restrict__ nodes,
                                                   const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox, nh_QFilter F) {
	extern __shared__ nh_QNear q_first[];
	const uint32_t stride = blockDim.x;
	nh_QNear* const list = q_first + threadIdx.x;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
		Shape k;
		k.read(casts + (size_t)i * Shape::WORDS);
		const bool ray = k.raylike();
		float bd = k.max_t;
		uint32_t held = 0u;
		nh_q_walk<FILTER>(nodes, rec, k.ok && n ? 0u : NH_Q_NONE, k.ignore, F, FILTER ? F.of(i) : 0u,
			[&](nh_f3 lo, nh_f3 hi, float& t0) { return nh_q_all_node(k, ray, lo, hi, bd, t0); },
			[&](uint32_t c, const nh_QRec& q, float t0) {
				const nh_QHit h = k.all(nh_q_unpack(q), c < nbox, t0);
				if (!h.hit || !(h.t <= bd)) return false;
				if (nh_q_nearest_insert(list, stride, kk, &held, h.t, c, k.max_t) && held == kk) bd = list[(kk - 1u) * stride].key;
				return false;
			});
		nh_RayHit* out = hits + (size_t)i * kk;
		for (uint32_t j = 0u; j < held; ++j) nh_q_rebuild_hit(k, list[j * stride].c, out + j, rec, nbox);
		for (uint32_t j = held; j < kk; ++j) nh_q_write_hit(out + j, rec, nbox, k.ok, NH_Q_NONE, k.max_t, nh_make3(0.0f, 0.0f, 0.0f));
		if (counts) counts[i] = held;
	}
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
// What the walking kernels get of the context's filter; `on`: the call launches the FILTER = true instantiation.
static nh_QFilter nh_query_filter_of(const nh_QueryState* q, bool* on) {
	*on = q->filter_mode != NH_FILTER_OFF;
	nh_QFilter F;
	F.words = q->layers_set ? q->node_layers : nullptr;
	F.masks = q->filter_mode == NH_FILTER_PER_QUERY ? q->filter_masks : nullptr;
	F.mask = q->filter_mask;
	return F;
}

// The argument rules of the calls that write a fixed number of records per query, in the order that decides the error code: the flags the call takes, its k
// bound (k_max = 0: it has no k), its count bound (count_end = 0: none), its optional counts.  The caller returns what this returns where that is an error
// or count == 0.
static int nh_query_call(nh_context* ctx, uint32_t flags, uint32_t flags_allowed, uint32_t k, uint32_t k_max, uint32_t count, uint32_t count_end,
                         const void* in, const void* out, const uint32_t* counts) {
	if (!ctx || !ctx->query || !ctx->query->built) return NH_ERR_INVALID;
	if ((flags & ~flags_allowed) || (k_max && (k == 0u || k > k_max)) || (count_end && count >= count_end)) return NH_ERR_INVALID;
	if (count == 0u) return NH_OK;
	if (!in || !out || (((uintptr_t)in | (uintptr_t)out) & 15u) || ((uintptr_t)counts & 3u)) return NH_ERR_INVALID;    // (records are moved as 16-byte words)
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	return NH_OK;
}

// The four closest-hit casts: one record type and one kernel each.
template <class Cast>
using nh_CastKernel = void (*)(const Cast*, uint32_t, nh_RayHit*, const nh_QNode*, const nh_QRec*, uint32_t, uint32_t, uint32_t, nh_QFilter);
template <class Cast>
static int nh_cast(nh_context* ctx, const char* label, nh_CastKernel<Cast> plain, nh_CastKernel<Cast> filtered, const Cast* casts, uint32_t count, nh_RayHit* hits,
                   uint32_t flags) {
	{ const int rc = nh_query_call(ctx, flags, NH_RAY_ANY_HIT, 0u, 0u, count, 0u, casts, hits, nullptr); if (rc || count == 0u) return rc; }
	nh_QueryState* q = ctx->query;
	bool on;
	const nh_QFilter F = nh_query_filter_of(q, &on);
	NH_LAUNCH(ctx, label, on ? filtered : plain, nh_grid_for(count, 256, 1u << 20), 256, casts, count, hits, q->nodes, q->rec, q->n, q->nbox,
	          (flags & NH_RAY_ANY_HIT) ? 1u : 0u, F);
	return NH_OK;
}

extern "C" int nh_raycast(nh_context* ctx, const nh_Ray* rays, uint32_t count, nh_RayHit* hits, uint32_t flags) {
	return nh_cast(ctx, "q_raycast", k_q_raycast<false>, k_q_raycast<true>, rays, count, hits, flags);
}

extern "C" int nh_spherecast(nh_context* ctx, const nh_SphereCast* casts, uint32_t count, nh_RayHit* hits, uint32_t flags) {
	return nh_cast(ctx, "q_spherecast", k_q_spherecast<false>, k_q_spherecast<true>, casts, count, hits, flags);
}

extern "C" int nh_capsulecast(nh_context* ctx, const nh_CapsuleCast* casts, uint32_t count, nh_RayHit* hits, uint32_t flags) {
	return nh_cast(ctx, "q_capsulecast", k_q_capsulecast<false>, k_q_capsulecast<true>, casts, count, hits, flags);
}

extern "C" int nh_boxcast(nh_context* ctx, const nh_BoxCast* casts, uint32_t count, nh_RayHit* hits, uint32_t flags) {
	return nh_cast(ctx, "q_boxcast", k_q_boxcast<false>, k_q_boxcast<true>, casts, count, hits, flags);
}

// The two sensor calls: nh_raycast's checks in nh_raycast's order, then their own.  *rays = 0 where the call is a no-op (or refused): nothing is read then.
static int nh_sense_args(nh_context* ctx, const nh_BodyData* bodies, const nh_Sensor* sensors, uint32_t count, const nh_Beam* beams, uint32_t beam_count,
                         uint32_t flags, uint32_t flags_allowed, uint64_t* rays) {
	*rays = 0u;
	if (!ctx || !ctx->query || !ctx->query->built) return NH_ERR_INVALID;
	if ((flags & ~flags_allowed) || (uint64_t)count * beam_count >= (1ull << 31)) return NH_ERR_INVALID;
	if (count == 0u || beam_count == 0u) return NH_OK;
	if (!sensors || !beams || (((uintptr_t)sensors | (uintptr_t)beams) & 15u)) return NH_ERR_INVALID;          // (records are moved as 16-byte words)
	if (bodies && !bodies->transforms) return NH_ERR_INVALID;
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	*rays = (uint64_t)count * beam_count;
	return NH_OK;
}
static uint32_t nh_sense_grid(uint32_t count, uint32_t beam_count) { return nh_grid_for((uint64_t)count * ((beam_count + 63u) / 64u), 4, NH_Q_SENSE_GRID); }

extern "C" int nh_sense(nh_context* ctx, const nh_BodyData* bodies, const nh_Sensor* sensors, uint32_t count, const nh_Beam* beams, uint32_t beam_count,
                        const nh_SenseOut* out, uint32_t flags) {
	uint64_t rays;
	{ const int rc = nh_sense_args(ctx, bodies, sensors, count, beams, beam_count, flags, NH_RAY_ANY_HIT, &rays); if (rc || !rays) return rc; }
	if (!out || (!out->t && !out->body && !out->tag && !out->hits)) return NH_ERR_INVALID;
	if ((((uintptr_t)out->t | (uintptr_t)out->body | (uintptr_t)out->tag) & 3u) || ((uintptr_t)out->hits & 15u)) return NH_ERR_INVALID;
	nh_QueryState* q = ctx->query;
	bool on;
	const nh_QFilter F = nh_query_filter_of(q, &on);
	NH_LAUNCH(ctx, "q_sense", on ? k_q_sense<true> : k_q_sense<false>, nh_sense_grid(count, beam_count), 256, sensors, count, beams, beam_count,
	          bodies ? bodies->transforms : nullptr, bodies ? bodies->count : 0u, *out, q->nodes, q->rec, q->n, q->nbox, (flags & NH_RAY_ANY_HIT) ? 1u : 0u, F);
	return NH_OK;
}

extern "C" int nh_sense_rays(nh_context* ctx, const nh_BodyData* bodies, const nh_Sensor* sensors, uint32_t count, const nh_Beam* beams, uint32_t beam_count,
                             nh_Ray* rays, uint32_t flags) {
	uint64_t total;
	{ const int rc = nh_sense_args(ctx, bodies, sensors, count, beams, beam_count, flags, 0u, &total); if (rc || !total) return rc; }
	if (!rays || ((uintptr_t)rays & 15u)) return NH_ERR_INVALID;
	NH_LAUNCH(ctx, "q_sense_rays", k_q_sense_rays, nh_sense_grid(count, beam_count), 256, sensors, count, beams, beam_count,
	          bodies ? bodies->transforms : nullptr, bodies ? bodies->count : 0u, rays);
	return NH_OK;
}

// nh_sweep's flag and scan words, by collider of the tree (a growth waits for the stream first, as nh_overlap_reserve's does)
static int nh_sweep_reserve(nh_context* ctx, uint32_t colliders) {
	nh_QueryState* q = ctx->query;
	if (q->sw_scan && colliders <= q->sw_capacity) return NH_OK;
	const uint32_t cap = colliders + colliders / 8u + 64u;          // (colliders < 2^30)
	NH_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	q->sw_capacity = 0;
	{ int rc = nh_device_buffers(ctx, { { &q->sw_scan, sizeof(uint32_t) * ((size_t)cap + 1u + 16u) } }); if (rc) return rc; }
	q->sw_capacity = cap;
	return NH_OK;
}

extern "C" int nh_sweep(nh_context* ctx, const nh_BodyData* bodies, const nh_SweepParams* params, const nh_SweepList* list, uint32_t flags) {
	if (!ctx || !ctx->query || !ctx->query->built || flags || !bodies || !params || !list || !list->counts) return NH_ERR_INVALID;
	if (bodies->count && (!bodies->transforms || !bodies->momentum)) return NH_ERR_INVALID;
	if ((((uintptr_t)list->counts | (uintptr_t)list->colliders) & 3u) || (((uintptr_t)list->casts | (uintptr_t)list->hits) & 15u)) return NH_ERR_INVALID;
	if (list->capacity >= 0x80000000u || (!list->capacity && (list->colliders || list->casts || list->hits))) return NH_ERR_INVALID;
	const float ts = params->time_step, mt = params->min_travel, core = params->core;
	if (!std::isfinite(ts) || !std::isfinite(mt) || !std::isfinite(core) || !(mt >= 0.0f) || !(core >= 0.0f) || !(core <= 1.0f)) return NH_ERR_INVALID;
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	nh_QueryState* q = ctx->query;
	if (q->n == 0u) {          // no collider: no entry
		NH_HIP_CHECK(ctx, hipMemsetAsync(list->counts, 0, 2u * sizeof(uint32_t), ctx->stream));
		return NH_OK;
	}
	{ const int rc = nh_sweep_reserve(ctx, q->n); if (rc) return rc; }
	const nh_QSweepIn in{ bodies->transforms, bodies->momentum, bodies->count, ts, mt, core };
	const uint32_t per_collider = nh_grid_for((uint64_t)q->n + 1u, 256, 1u << 16);
	NH_LAUNCH(ctx, "q_sweep_flag", k_q_sweep_flag, per_collider, 256, q->rec, q->n, q->nbox, in, q->sw_scan);
	nh_scan_u32(ctx, q->sw_scan, q->sw_scan, &q->ctl->zero, q->n + 1u, q->hist, nullptr);
	NH_LAUNCH(ctx, "q_sweep_gather", k_q_sweep_gather, per_collider, 256, q->rec, q->n, q->nbox, in, q->sw_scan, list->counts, list->colliders, list->casts, list->capacity);
	if (!list->hits) return NH_OK;
	bool on;
	const nh_QFilter F = nh_query_filter_of(q, &on);
	// (the device knows how many entries there are; the host only that a share is no longer than the capacity or than its shape's colliders)
	const uint32_t nsph = q->n - q->nbox;
	if (q->nbox) NH_LAUNCH(ctx, "q_sweep_box", on ? (k_q_sweep<false, true>) : (k_q_sweep<false, false>), nh_grid_for(std::min(list->capacity, q->nbox), 256, 1u << 20), 256,
	                       q->rec, q->n, q->nbox, in, q->sw_scan, list->hits, list->capacity, q->nodes, F);
	if (nsph) NH_LAUNCH(ctx, "q_sweep_ball", on ? (k_q_sweep<true, true>) : (k_q_sweep<true, false>), nh_grid_for(std::min(list->capacity, nsph), 256, 1u << 20), 256,
	                    q->rec, q->n, q->nbox, in, q->sw_scan, list->hits, list->capacity, q->nodes, F);
	return NH_OK;
}

extern "C" int nh_sweep_limit(nh_context* ctx, const nh_BodyData* bodies, const nh_SweepList* list, float* factors, uint32_t flags) {
	if (!ctx || !ctx->query || !ctx->query->built || flags || !bodies || !list || !list->counts) return NH_ERR_INVALID;
	if (bodies->count && !bodies->momentum) return NH_ERR_INVALID;
	if ((((uintptr_t)list->counts | (uintptr_t)list->colliders | (uintptr_t)factors) & 3u) || ((uintptr_t)list->hits & 15u)) return NH_ERR_INVALID;
	if (list->capacity >= 0x80000000u || (list->capacity && (!list->colliders || !list->hits))) return NH_ERR_INVALID;
	{ int rc = nh_flush_pending(ctx); if (rc) return rc; }          // momentum is written: whatever was deferred comes first
	if (list->capacity == 0u || bodies->count == 0u) return NH_OK;          // no entry can be read: nobody is limited
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	nh_QueryState* q = ctx->query;
	if (bodies->count > q->sw_body_capacity) {          // (a growth waits for the stream first; the words are never cleared: a list's entries set the ones they use)
		NH_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
		q->sw_body_capacity = 0;
		{ int rc = nh_device_buffers(ctx, { { &q->sw_body, sizeof(uint2) * (size_t)bodies->count } }); if (rc) return rc; }
		q->sw_body_capacity = bodies->count;
	}
	const nh_QSweepEntries L{ list->counts, list->colliders, list->hits, list->capacity };
	const uint32_t grid = nh_grid_for(std::min(list->capacity, q->n ? q->n : 1u), 256, 1u << 16);
	NH_LAUNCH(ctx, "q_limit_init", k_q_limit_init, grid, 256, L, q->rec, q->n, bodies->count, q->sw_body);
	NH_LAUNCH(ctx, "q_limit_min", k_q_limit_min, grid, 256, L, q->rec, q->n, bodies->count, q->sw_body);
	NH_LAUNCH(ctx, "q_limit_apply", k_q_limit_apply, grid, 256, L, q->rec, q->n, bodies->count, q->sw_body, bodies->momentum, factors);
	return NH_OK;
}

// The four movers and their _touched forms: one record type, one result type and one kernel pair each.  One launch, nh_distance's checks in nh_distance's order; no
// allocation, no wait.  k_max = 0: the plain call (k, counts and touches are not read); otherwise the touched call, whose k, counts and touches follow the plain
// call's checks.  (`filtered` before `plain`: the callers name the instantiations in the order the code object has always held them.)
template <class In, class Out>
using nh_MoverKernel = void (*)(const In*, uint32_t, Out*, const nh_QNode*, const nh_QRec*, uint32_t, uint32_t, nh_QFilter, uint32_t, uint32_t*, nh_Touch*);
template <class In, class Out>
static int nh_mover(nh_context* ctx, const char* label, nh_MoverKernel<In, Out> filtered, nh_MoverKernel<In, Out> plain, const In* in, uint32_t count, Out* out,
                    uint32_t flags, uint32_t k = 0u, uint32_t k_max = 0u, uint32_t* counts = nullptr, nh_Touch* touches = nullptr) {
	{ const int rc = nh_query_call(ctx, flags, 0u, k, k_max, count, 1u << 30, in, out, counts); if (rc || count == 0u) return rc; }
	if (k_max && (!counts || !touches || ((uintptr_t)touches & 15u))) return NH_ERR_INVALID;
	nh_QueryState* q = ctx->query;
	bool on;
	const nh_QFilter F = nh_query_filter_of(q, &on);
	NH_LAUNCH(ctx, label, on ? filtered : plain, nh_grid_for(count, 256, 1u << 20), 256, in, count, out, q->nodes, q->rec, q->n, q->nbox, F, k, counts, touches);
	return NH_OK;
}

extern "C" int nh_move(nh_context* ctx, const nh_Move* moves, uint32_t count, nh_MoveResult* results, uint32_t flags) {
	return nh_mover(ctx, "q_move", k_q_move<nh_QCapsule, true, false>, k_q_move<nh_QCapsule, false, false>, moves, count, results, flags);
}

extern "C" int nh_boxmove(nh_context* ctx, const nh_BoxMove* moves, uint32_t count, nh_MoveResult* results, uint32_t flags) {
	return nh_mover(ctx, "q_boxmove", k_q_move<nh_QBox, true, false>, k_q_move<nh_QBox, false, false>, moves, count, results, flags);
}

extern "C" int nh_walk(nh_context* ctx, const nh_Walk* walks, uint32_t count, nh_WalkResult* results, uint32_t flags) {
	return nh_mover(ctx, "q_walk", k_q_walk<nh_QCapsule, true, false>, k_q_walk<nh_QCapsule, false, false>, walks, count, results, flags);
}

extern "C" int nh_boxwalk(nh_context* ctx, const nh_BoxWalk* walks, uint32_t count, nh_WalkResult* results, uint32_t flags) {
	return nh_mover(ctx, "q_boxwalk", k_q_walk<nh_QBox, true, false>, k_q_walk<nh_QBox, false, false>, walks, count, results, flags);
}

extern "C" int nh_move_touched(nh_context* ctx, const nh_Move* moves, uint32_t count, nh_MoveResult* results, uint32_t k, uint32_t* counts, nh_Touch* touches, uint32_t flags) {
	return nh_mover(ctx, "q_move_touched", k_q_move<nh_QCapsule, true, true>, k_q_move<nh_QCapsule, false, true>, moves, count, results, flags, k, NH_MOVE_MAX_SLIDES + 1u,
	                counts, touches);
}

extern "C" int nh_boxmove_touched(nh_context* ctx, const nh_BoxMove* moves, uint32_t count, nh_MoveResult* results, uint32_t k, uint32_t* counts, nh_Touch* touches, uint32_t flags) {
	return nh_mover(ctx, "q_boxmove_touched", k_q_move<nh_QBox, true, true>, k_q_move<nh_QBox, false, true>, moves, count, results, flags, k, NH_MOVE_MAX_SLIDES + 1u,
	                counts, touches);
}

extern "C" int nh_walk_touched(nh_context* ctx, const nh_Walk* walks, uint32_t count, nh_WalkResult* results, uint32_t k, uint32_t* counts, nh_Touch* touches, uint32_t flags) {
	return nh_mover(ctx, "q_walk_touched", k_q_walk<nh_QCapsule, true, true>, k_q_walk<nh_QCapsule, false, true>, walks, count, results, flags, k, NH_WALK_MAX_CASTS, counts,
	                touches);
}

extern "C" int nh_boxwalk_touched(nh_context* ctx, const nh_BoxWalk* walks, uint32_t count, nh_WalkResult* results, uint32_t k, uint32_t* counts, nh_Touch* touches, uint32_t flags) {
	return nh_mover(ctx, "q_boxwalk_touched", k_q_walk<nh_QBox, true, true>, k_q_walk<nh_QBox, false, true>, walks, count, results, flags, k, NH_WALK_MAX_CASTS, counts,
	                touches);
}

// nh_move's checks in nh_move's order; the sphere-and-box launch and the capsule launch under one label, as nh_overlap splits its walks; no allocation, no wait.
extern "C" int nh_recover(nh_context* ctx, const nh_Recover* queries, uint32_t count, nh_RecoverResult* results, uint32_t flags) {
	{ const int rc = nh_query_call(ctx, flags, 0u, 0u, 0u, count, 1u << 30, queries, results, nullptr); if (rc || count == 0u) return rc; }
	nh_QueryState* q = ctx->query;
	bool on;
	const nh_QFilter F = nh_query_filter_of(q, &on);
	const uint32_t grid = nh_grid_for(count, 256, 1u << 20);
	NH_LAUNCH(ctx, "q_recover", (on ? k_q_recover<false, true> : k_q_recover<false, false>), grid, 256, queries, count, results, q->nodes, q->rec, q->n, q->nbox, F);
	NH_LAUNCH(ctx, "q_recover", (on ? k_q_recover<true, true> : k_q_recover<true, false>), grid, 256, queries, count, results, q->nodes, q->rec, q->n, q->nbox, F);
	return NH_OK;
}

extern "C" int nh_closest(nh_context* ctx, const nh_PointQuery* queries, uint32_t count, nh_PointHit* hits, uint32_t flags) {
	{ const int rc = nh_query_call(ctx, flags, 0u, 0u, 0u, count, 0u, queries, hits, nullptr); if (rc || count == 0u) return rc; }
	nh_QueryState* q = ctx->query;
	bool on;
	const nh_QFilter F = nh_query_filter_of(q, &on);
	NH_LAUNCH(ctx, "q_closest", on ? k_q_closest<true> : k_q_closest<false>, nh_grid_for(count, 256, 1u << 20), 256, queries, count, hits, q->nodes, q->rec, q->keys,
	          q->ctl, q->n, q->nbox, F);
	return NH_OK;
}

// One launch with the lists' LDS sized by k (the table at k_q_closest_k); no allocation, no wait.
extern "C" int nh_closest_k(nh_context* ctx, const nh_PointQuery* queries, uint32_t count, uint32_t k, uint32_t* counts, nh_PointHit* hits, uint32_t flags) {
	{ const int rc = nh_query_call(ctx, flags, 0u, k, NH_CLOSEST_K_MAX, count, 1u << 30, queries, hits, counts); if (rc || count == 0u) return rc; }
	nh_QueryState* q = ctx->query;
	const uint32_t block = nh_q_nearest_block(k);
	bool on;
	const nh_QFilter F = nh_query_filter_of(q, &on);
	NH_LAUNCH_LDS(ctx, "q_closest_k", on ? k_q_closest_k<true> : k_q_closest_k<false>, nh_grid_for(count, block, 1u << 20), block, block * k * sizeof(nh_QNear),
	              queries, count, k, counts, hits, q->nodes, q->rec, q->keys, q->ctl, q->n, q->nbox, F);
	return NH_OK;
}

// One launch, as nh_closest; no allocation, no wait.
extern "C" int nh_distance(nh_context* ctx, const nh_DistanceQuery* queries, uint32_t count, nh_PointHit* hits, uint32_t flags) {
	{ const int rc = nh_query_call(ctx, flags, 0u, 0u, 0u, count, 1u << 30, queries, hits, nullptr); if (rc || count == 0u) return rc; }
	nh_QueryState* q = ctx->query;
	bool on;
	const nh_QFilter F = nh_query_filter_of(q, &on);
	NH_LAUNCH(ctx, "q_distance", on ? k_q_distance<true> : k_q_distance<false>, nh_grid_for(count, 256, 1u << 20), 256, queries, count, hits, q->nodes, q->rec, q->keys,
	          q->ctl, q->n, q->nbox, F);
	return NH_OK;
}

// nh_overlap's sort scratch, by record of the caller's capacity (a growth waits for the stream first, as nh_query_reserve's does)
static int nh_overlap_reserve(nh_context* ctx, uint32_t capacity) {
	nh_QueryState* q = ctx->query;
	if (capacity <= q->ov_capacity) return NH_OK;
	const uint64_t cap64 = (uint64_t)capacity + capacity / 8u + 64u;
	const uint32_t cap = cap64 > 0xffffffffull ? 0xffffffffu : (uint32_t)cap64;
	NH_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	q->ov_capacity = 0;
	{ int rc = nh_device_buffers(ctx, { { &q->ov_keys_a, sizeof(uint64_t) * (size_t)cap }, { &q->ov_keys_b, sizeof(uint64_t) * (size_t)cap },
	                                    { &q->ov_vals_a, sizeof(uint32_t) * (size_t)cap }, { &q->ov_vals_b, sizeof(uint32_t) * (size_t)cap } }); if (rc) return rc; }
	q->ov_capacity = cap;
	return NH_OK;
}

static int nh_q_bits(uint32_t x) { return x ? 32 - __builtin_clz(x) : 0; }

// The argument rules nh_overlap, nh_penetration and the all-hits casts share, in the order that decides the error code; then, for a list call (*list:
// hits and a capacity given), the sort scratch.  The caller returns what this returns where that is an error or count == 0.
static int nh_overlap_args(nh_context* ctx, const void* queries, uint32_t count, const uint32_t* offsets, const void* hits, uint32_t capacity, uint32_t flags,
                           bool* list) {
	if (!ctx || !ctx->query || !ctx->query->built) return NH_ERR_INVALID;
	if (flags != 0u || count >= NH_Q_MAX_COLLIDERS) return NH_ERR_INVALID;
	if (count == 0u) return NH_OK;
	if (!queries || ((uintptr_t)queries & 15u)) return NH_ERR_INVALID;        // (records are read as 16-byte words)
	if (!offsets || ((uintptr_t)offsets & 3u)) return NH_ERR_INVALID;
	if ((!hits && capacity) || ((uintptr_t)hits & 15u)) return NH_ERR_INVALID;
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	*list = hits != nullptr && capacity != 0u;
	return *list ? nh_overlap_reserve(ctx, capacity) : NH_OK;
}

// From the per-query counts in offsets[0 .. count) (offsets[count] = 0) to the complete offsets, the written prefix and the overflow marker: the three
// launches nh_overlap's chain and the all-hits casts share.
static void nh_overlap_offsets(nh_context* ctx, uint32_t* offsets, uint32_t count, uint32_t capacity) {
	nh_QueryState* q = ctx->query;
	nh_scan_u32(ctx, offsets, offsets, &q->ctl->zero, count + 1u, q->hist, nullptr);
	NH_LAUNCH(ctx, "q_overlap_fix", k_q_overlap_fix, nh_grid_for((uint64_t)count + 1u, 256, 4096), 256, offsets, count, capacity, q->ctl);
	NH_LAUNCH(ctx, "q_overlap_fin", k_q_overlap_fin, 1, 1, offsets, count, q->ctl);
}

// nh_region's cursors, by region of the caller's count (a growth waits for the stream first, as nh_overlap_reserve's does)
static int nh_region_reserve(nh_context* ctx, uint32_t count) {
	nh_QueryState* q = ctx->query;
	if (count <= q->rg_capacity) return NH_OK;
	const uint32_t cap = count + count / 8u + 64u;          // (count < 2^30)
	NH_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	q->rg_capacity = 0;
	{ int rc = nh_device_buffers(ctx, { { &q->rg_cursor, sizeof(uint32_t) * (size_t)cap } }); if (rc) return rc; }
	q->rg_capacity = cap;
	return NH_OK;
}

// ---- the list calls: one host chain --------------------------------------------------------------------------------------------------------------
// nh_overlap, nh_penetration, their wide forms, nh_region and the four all-hits casts run one chain, nh_list_chain, and end in their own gather.  They differ in
// `walk`, a callable that enqueues one pass over the tree given an nh_QPass (the count pass: list false, cursor / keys / vals null; then the list pass), and in
//   spread   the walk deals (query, entry node) items to waves (k_q_wide, k_q_region): it ADDS into offsets, so offsets[0 .. count] are zeroed before the count
//            pass; it takes nh_region's cursors, reserved for a list call and zeroed before the list pass; its grid is one wave per item at most
//   by_t     the all-hits casts' key plan (the comment above k_q_castall): one sort where query, t and collider fit 64 bits, or else the sort by collider,
//            q_castall_rekey, the sort by (query, t).  Otherwise one sort by (query, combined collider index).
struct nh_QPass { bool list, on; nh_QFilter F; uint32_t grid, cbits, one_sort; uint32_t* cursor; uint64_t* keys; uint32_t* vals; };
// Where the chain left the written prefix (ctl->ov_written records) of a list call, sorted; keys null: a count-only call, or count == 0.
struct nh_QSorted { uint64_t* keys; uint32_t* vals; uint32_t cbits, one_sort; };

// The instantiation a pass launches: LIST or not, FILTER or not.
template <class K>
static K nh_q_pass_kernel(const nh_QPass& p, K count, K count_filtered, K list, K list_filtered) {
	return p.list ? (p.on ? list_filtered : list) : (p.on ? count_filtered : count);
}

// From the argument checks to the sort or sorts: offsets are complete behind it.  `hits` is only checked here: records of any size are moved as 16-byte words.  The
// caller returns what this returns where that is an error or out->keys is null.
template <class Walk>
static int nh_list_chain(nh_context* ctx, const void* in, uint32_t count, uint32_t* offsets, const void* hits, uint32_t capacity, uint32_t flags, bool spread,
                         bool by_t, Walk walk, nh_QSorted* out) {
	*out = nh_QSorted{};
	bool list = false;
	{ const int rc = nh_overlap_args(ctx, in, count, offsets, hits, capacity, flags, &list); if (rc || count == 0u) return rc; }
	if (spread && list) { const int rc = nh_region_reserve(ctx, count); if (rc) return rc; }
	nh_QueryState* q = ctx->query;
	const int cbits = nh_q_bits(q->n), ibits = nh_q_bits(count);
	nh_QPass p{};
	p.cbits = (uint32_t)cbits;
	p.one_sort = by_t && ibits + 32 + cbits <= 64 ? 1u : 0u;
	// (spread: one wave per item at most -- a small world or a small batch launches a small grid)
	p.grid = spread ? nh_grid_for((uint64_t)count * (q->n ? q->n : 1u), 4u, NH_Q_REGION_GRID) : nh_grid_for(count, 256, 1u << 20);
	p.F = nh_query_filter_of(q, &p.on);
	if (spread) NH_HIP_CHECK(ctx, hipMemsetAsync(offsets, 0, sizeof(uint32_t) * ((size_t)count + 1u), ctx->stream));
	walk(p);
	nh_overlap_offsets(ctx, offsets, count, capacity);
	if (!list) return NH_OK;
	if (spread) NH_HIP_CHECK(ctx, hipMemsetAsync(q->rg_cursor, 0, sizeof(uint32_t) * (size_t)count, ctx->stream));
	nh_QSorted s{ q->ov_keys_a, q->ov_vals_a, p.cbits, p.one_sort };
	p.list = true; p.cursor = spread ? q->rg_cursor : nullptr; p.keys = s.keys; p.vals = s.vals;
	walk(p);
	// (the low `bits` of the keys, rounded to whole bytes; the sorted pairs lie in whichever pair of buffers the last digit wrote)
	uint64_t* keys_other = q->ov_keys_b;
	uint32_t* vals_other = q->ov_vals_b;
	const auto sort = [&](int bits) {
		if (!nh_sort_u64_u32(ctx, s.keys, keys_other, s.vals, vals_other, &q->ctl->ov_written, q->hist, 0, (bits + 7) / 8 * 8)) return;
		std::swap(s.keys, keys_other); std::swap(s.vals, vals_other);
	};
	if (!by_t) sort(cbits + ibits);
	else if (p.one_sort) sort(ibits + 32 + cbits);
	else {
		sort(cbits);
		NH_LAUNCH(ctx, "q_castall_rekey", k_q_castall_rekey, nh_grid_for(capacity, 256, 4096), 256, s.keys, s.vals, q->ctl, p.cbits);
		sort(ibits + 32);
	}
	*out = s;
	return NH_OK;
}

// The gather of nh_OverlapHit records (nh_overlap, nh_overlap_wide, nh_region), and nh_penetration's, which evaluates the pair function of each record (header: the
// same set, the same order, the same offsets).
static void nh_list_gather(nh_context* ctx, const nh_QSorted& s, const void*, uint32_t, nh_OverlapHit* hits, uint32_t capacity) {
	nh_QueryState* q = ctx->query;
	NH_LAUNCH(ctx, "q_overlap_gather", k_q_overlap_gather, nh_grid_for(capacity, 256, 4096), 256, s.vals, q->ctl, q->rec, q->n, q->nbox, hits);
}
static void nh_list_gather(nh_context* ctx, const nh_QSorted& s, const nh_OverlapQuery* queries, uint32_t count, nh_PenetrationHit* hits, uint32_t capacity) {
	nh_QueryState* q = ctx->query;
	NH_LAUNCH(ctx, "q_penetration_gather", k_q_penetration_gather, nh_grid_for(capacity, 256, 1u << 20), 256, s.keys, s.vals, q->ctl, q->rec, q->n, q->nbox, queries,
	          count, s.cbits, hits);
}

// nh_overlap and nh_penetration, or (wide) their wide forms with k_q_wide in place of the walks: the chain with the sphere-and-box walk and the capsule walk in each
// pass, sorted by (query, combined collider index), then the gather of the record type.
template <class Hit>
static int nh_overlap_call(nh_context* ctx, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets, Hit* hits, uint32_t capacity, uint32_t flags, bool wide) {
	const auto walks = [&](const nh_QPass& p) {
		nh_QueryState* q = ctx->query;
		NH_LAUNCH(ctx, p.list ? "q_overlap_list" : "q_overlap_count",
		          nh_q_pass_kernel(p, k_q_overlap<false, false, false>, k_q_overlap<false, false, true>, k_q_overlap<true, false, false>, k_q_overlap<true, false, true>),
		          p.grid, 256, queries, count, offsets, q->nodes, q->rec, q->n, q->nbox, q->ctl, p.keys, p.vals, p.cbits, p.F);
		NH_LAUNCH(ctx, p.list ? "q_overlap_list_capsule" : "q_overlap_count_capsule",
		          nh_q_pass_kernel(p, k_q_overlap<false, true, false>, k_q_overlap<false, true, true>, k_q_overlap<true, true, false>, k_q_overlap<true, true, true>),
		          p.grid, 256, queries, count, offsets, q->nodes, q->rec, q->n, q->nbox, q->ctl, p.keys, p.vals, p.cbits, p.F);
	};
	const auto spread_walks = [&](const nh_QPass& p) {
		nh_QueryState* q = ctx->query;
		NH_LAUNCH(ctx, p.list ? "q_wide_list" : "q_wide_count",
		          nh_q_pass_kernel(p, k_q_wide<false, false, false>, k_q_wide<false, false, true>, k_q_wide<true, false, false>, k_q_wide<true, false, true>),
		          p.grid, 256, queries, count, offsets, q->nodes, q->rec, q->idx, q->last, q->top, q->n, q->nbox, q->ctl, p.cursor, p.keys, p.vals, p.cbits, p.F);
		NH_LAUNCH(ctx, p.list ? "q_wide_list_capsule" : "q_wide_count_capsule",
		          nh_q_pass_kernel(p, k_q_wide<false, true, false>, k_q_wide<false, true, true>, k_q_wide<true, true, false>, k_q_wide<true, true, true>),
		          p.grid, 256, queries, count, offsets, q->nodes, q->rec, q->idx, q->last, q->top, q->n, q->nbox, q->ctl, p.cursor, p.keys, p.vals, p.cbits, p.F);
	};
	nh_QSorted s;
	const int rc = wide ? nh_list_chain(ctx, queries, count, offsets, hits, capacity, flags, true, false, spread_walks, &s)
	                    : nh_list_chain(ctx, queries, count, offsets, hits, capacity, flags, false, false, walks, &s);
	if (rc == NH_OK && s.keys) nh_list_gather(ctx, s, queries, count, hits, capacity);
	return rc;
}

extern "C" int nh_overlap(nh_context* ctx, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets, nh_OverlapHit* hits, uint32_t capacity,
                          uint32_t flags) {
	return nh_overlap_call(ctx, queries, count, offsets, hits, capacity, flags, false);
}

extern "C" int nh_penetration(nh_context* ctx, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets, nh_PenetrationHit* hits, uint32_t capacity,
                              uint32_t flags) {
	return nh_overlap_call(ctx, queries, count, offsets, hits, capacity, flags, false);
}

// The wide forms (header, "nh_overlap_wide"): the same bytes, the work of one query spread over the GPU.
extern "C" int nh_overlap_wide(nh_context* ctx, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets, nh_OverlapHit* hits, uint32_t capacity,
                               uint32_t flags) {
	return nh_overlap_call(ctx, queries, count, offsets, hits, capacity, flags, true);
}

extern "C" int nh_penetration_wide(nh_context* ctx, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets, nh_PenetrationHit* hits, uint32_t capacity,
                                   uint32_t flags) {
	return nh_overlap_call(ctx, queries, count, offsets, hits, capacity, flags, true);
}

// The spread chain with k_q_region as its walk (the comment above k_q_region), and nh_overlap's gather.
extern "C" int nh_region(nh_context* ctx, const nh_Region* regions, uint32_t count, uint32_t* offsets, nh_OverlapHit* hits, uint32_t capacity, uint32_t flags) {
	const auto walk = [&](const nh_QPass& p) {
		nh_QueryState* q = ctx->query;
		NH_LAUNCH(ctx, p.list ? "q_region_list" : "q_region_count",
		          nh_q_pass_kernel(p, k_q_region<false, false>, k_q_region<false, true>, k_q_region<true, false>, k_q_region<true, true>), p.grid, 256, regions, count,
		          offsets, q->nodes, q->rec, q->idx, q->last, q->top, q->n, q->nbox, q->ctl, p.cursor, p.keys, p.vals, p.cbits, p.F);
	};
	nh_QSorted s;
	const int rc = nh_list_chain(ctx, regions, count, offsets, hits, capacity, flags, true, false, walk, &s);
	if (rc == NH_OK && s.keys) nh_list_gather(ctx, s, regions, count, hits, capacity);
	return rc;
}

// The all-hits casts (the comment above k_q_castall): the chain with the casts' walk, ordered by t.  `label`: the timing labels' stem, q_<entry point without
// nh_>.
template <class Shape>
static int nh_castall(nh_context* ctx, const char* const label[3], const void* casts, uint32_t count, uint32_t* offsets, nh_RayHit* hits, uint32_t capacity,
                      uint32_t flags) {
	const float4* recs = static_cast<const float4*>(casts);
	const auto walk = [&](const nh_QPass& p) {
		nh_QueryState* q = ctx->query;
		NH_LAUNCH(ctx, label[p.list ? 1 : 0],
		          nh_q_pass_kernel(p, k_q_castall<Shape, false, false>, k_q_castall<Shape, false, true>, k_q_castall<Shape, true, false>, k_q_castall<Shape, true, true>),
		          p.grid, 256, recs, count, offsets, q->nodes, q->rec, q->n, q->nbox, q->ctl, p.keys, p.vals, p.cbits, p.one_sort, p.F);
	};
	nh_QSorted s;
	{ const int rc = nh_list_chain(ctx, casts, count, offsets, hits, capacity, flags, false, true, walk, &s); if (rc || !s.keys) return rc; }
	nh_QueryState* q = ctx->query;
	NH_LAUNCH(ctx, label[2], (k_q_castall_gather<Shape>), nh_grid_for(capacity, 256, 1u << 20), 256, s.keys, s.vals, q->ctl, q->rec, q->n, q->nbox, recs, count,
	          s.one_sort ? 32u + s.cbits : 32u, hits);
	return NH_OK;
}

#define NH_CASTALL_LABELS(stem) static const char* const label[3] = { stem "_count", stem "_list", stem "_gather" }

extern "C" int nh_raycast_all(nh_context* ctx, const nh_Ray* rays, uint32_t count, uint32_t* offsets, nh_RayHit* hits, uint32_t capacity, uint32_t flags) {
	NH_CASTALL_LABELS("q_raycast_all");
	return nh_castall<nh_QRay>(ctx, label, rays, count, offsets, hits, capacity, flags);
}

extern "C" int nh_spherecast_all(nh_context* ctx, const nh_SphereCast* casts, uint32_t count, uint32_t* offsets, nh_RayHit* hits, uint32_t capacity,
                                 uint32_t flags) {
	NH_CASTALL_LABELS("q_spherecast_all");
	return nh_castall<nh_QBall>(ctx, label, casts, count, offsets, hits, capacity, flags);
}

extern "C" int nh_boxcast_all(nh_context* ctx, const nh_BoxCast* casts, uint32_t count, uint32_t* offsets, nh_RayHit* hits, uint32_t capacity, uint32_t flags) {
	NH_CASTALL_LABELS("q_boxcast_all");
	return nh_castall<nh_QBox>(ctx, label, casts, count, offsets, hits, capacity, flags);
}

extern "C" int nh_capsulecast_all(nh_context* ctx, const nh_CapsuleCast* casts, uint32_t count, uint32_t* offsets, nh_RayHit* hits, uint32_t capacity,
                                  uint32_t flags) {
	NH_CASTALL_LABELS("q_capsulecast_all");
	return nh_castall<nh_QCapsule>(ctx, label, casts, count, offsets, hits, capacity, flags);
}

// The four first-k casts: nh_closest_k's checks in nh_closest_k's order, one launch with the lists' LDS sized by k (the table at k_q_closest_k); no
// allocation, no wait.  The grid is capped at NH_Q_CAST_K_GRID workgroups -- what 256 CUs hold of the 256-lane ones at 8 waves per SIMD -- so a batch of
// half a million casts or more goes round the kernel's loop, each lane starting its list again from empty.
#define NH_Q_CAST_K_GRID 2048u
template <class Shape>
static int nh_cast_k(nh_context* ctx, const char* label, const void* casts, uint32_t count, uint32_t k, uint32_t* counts, nh_RayHit* hits, uint32_t flags) {
	{ const int rc = nh_query_call(ctx, flags, 0u, k, NH_CAST_K_MAX, count, 1u << 30, casts, hits, counts); if (rc || count == 0u) return rc; }
	nh_QueryState* q = ctx->query;
	const uint32_t block = nh_q_nearest_block(k);
	bool on;
	const nh_QFilter F = nh_query_filter_of(q, &on);
	NH_LAUNCH_LDS(ctx, label, (on ? k_q_cast_k<Shape, true> : k_q_cast_k<Shape, false>), nh_grid_for(count, block, NH_Q_CAST_K_GRID), block, block * k * sizeof(nh_QNear),
	              static_cast<const float4*>(casts), count, k, counts, hits, q->nodes, q->rec, q->n, q->nbox, F);
	return NH_OK;
}

extern "C" int nh_raycast_k(nh_context* ctx, const nh_Ray* rays, uint32_t count, uint32_t k, uint32_t* counts, nh_RayHit* hits, uint32_t flags) {
	return nh_cast_k<nh_QRay>(ctx, "q_raycast_k", rays, count, k, counts, hits, flags);
}

extern "C" int nh_spherecast_k(nh_context* ctx, const nh_SphereCast* casts, uint32_t count, uint32_t k, uint32_t* counts, nh_RayHit* hits, uint32_t flags) {
	return nh_cast_k<nh_QBall>(ctx, "q_spherecast_k", casts, count, k, counts, hits, flags);
}

extern "C" int nh_boxcast_k(nh_context* ctx, const nh_BoxCast* casts, uint32_t count, uint32_t k, uint32_t* counts, nh_RayHit* hits, uint32_t flags) {
	return nh_cast_k<nh_QBox>(ctx, "q_boxcast_k", casts, count, k, counts, hits, flags);
}

extern "C" int nh_capsulecast_k(nh_context* ctx, const nh_CapsuleCast* casts, uint32_t count, uint32_t k, uint32_t* counts, nh_RayHit* hits, uint32_t flags) {
	return nh_cast_k<nh_QCapsule>(ctx, "q_capsulecast_k", casts, count, k, counts, hits, flags);
}

// ---- events ------------------------------------------------------------------------------------------------------------------------------------
// nh_overlap_bodies / nh_overlap_events (header, "trigger events") work on LISTS that a list call of nh_overlap / nh_region wrote: they read neither the
// hierarchy nor the colliders nor the layer filter.  The work item is the RECORD (nh_query.h, "events": the segment-of-record search, the identity search
// within a segment, which the host oracle compiles as well); kernel boundaries are the only hand-offs and no atomic decides where a record goes.
//   nh_overlap_events   k_q_events_flag     one lane per record slot of cur, then of prev: 1 where the record's segment is read and its identity is not in
//                                           the other list's segment (cur's flags at [0, cur.capacity], prev's behind them; a slot that is no record: 0)
//                       nh_scan_u32         in place over both ranges at once: a position among `entered` is scan[r], among `left` scan[base + r] - scan[base]
//                       k_q_events_offsets  one lane per offset: out offsets[i] = the scan at the input's offsets[i], clamped to its capacity, and the
//                                           written prefix of each output by k_q_overlap_fix's rule (no wrap: an output's total is at most its input's)
//                       k_q_events_compact  one lane per record slot again: a flagged record whose position lies in the written prefix is copied whole
//   nh_overlap_bodies   k_q_bodies_prefix   the length of the input's written prefix, by k_q_overlap_fix's rule, for the sort
//                       k_q_bodies_keys     key (segment << 32 | body), value the record's index
//                       nh_sort_u64_u32     STABLE, in nh_overlap's scratch: a segment keeps its place (the segment is the key's upper part) and within
//                                           a run of one body the records keep the input's order -- ascending combined collider index -- so the first of
//                                           a run is the body's lowest collider
//                       k_q_bodies_flag     1 at the first record of each run;  nh_scan_u32;  k_q_bodies_offsets;  k_q_bodies_compact through the values
// Every record index a kernel reads is below the list's capacity and every position it writes below the output's written prefix, which is at most the
// output's capacity, whatever the offsets hold.
struct nh_QList { const uint32_t* offsets; const uint32_t* hits; uint32_t capacity; };          // (hits: four words a record)

__global__ __launch_bounds__(256) void k_q_events_flag(nh_QList cur, nh_QList prev, bool has_prev, uint32_t count, uint32_t by_body, uint32_t* __restrict__ scan) {
	const uint64_t words = (uint64_t)cur.capacity + prev.capacity + 2u;
	for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (uint64_t)gridDim.x * blockDim.x) {
		const bool left = w > cur.capacity;
		const nh_QList& mine = left ? prev : cur;
		const nh_QList& other = left ? cur : prev;
		const uint32_t r = (uint32_t)(left ? w - cur.capacity - 1u : w);
		uint32_t f = 0u;
		if (r < mine.capacity) {
			const uint32_t i = nh_q_seg_of_present(mine.offsets, count, mine.capacity, r);
			if (i != NH_Q_NONE) {
				if (!has_prev) f = 1u;          // (the first frame: prev has no record slot, so this is a record of cur)
				else if (nh_q_seg_present(other.offsets, count, other.capacity, i))
					f = nh_q_ident_find(other.hits, other.offsets[i], other.offsets[i + 1u], nh_q_ident(mine.hits + 4u * (size_t)r, by_body), by_body) ? 0u : 1u;
			}
		}
		scan[w] = f;
	}
}

// (scan: the exclusive scan of one list's flags, `capacity` + 1 words; offsets: that list's)
__device__ __forceinline__ void nh_q_events_offset(const uint32_t* __restrict__ scan, const uint32_t* __restrict__ offsets, uint32_t capacity, uint32_t count,
                                                   uint32_t i, uint32_t* __restrict__ out, uint32_t out_capacity, uint32_t* __restrict__ written) {
	const uint32_t a = scan[min(offsets[i], capacity)] - scan[0];
	out[i] = a;
	if (i == count) { if (a <= out_capacity) *written = a; return; }          // everything fits
	const uint32_t b = scan[min(offsets[i + 1u], capacity)] - scan[0];
	if (a <= out_capacity && out_capacity < b) *written = a;                   // monotone offsets: exactly one lane
}

__global__ __launch_bounds__(256) void k_q_events_offsets(nh_QList cur, nh_QList prev, bool has_prev, uint32_t count, const uint32_t* __restrict__ scan,
                                                           uint32_t* __restrict__ entered, uint32_t entered_capacity, uint32_t* __restrict__ left,
                                                           uint32_t left_capacity, nh_QEventCtl* __restrict__ ctl) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= count; i += gridDim.x * blockDim.x) {
		nh_q_events_offset(scan, cur.offsets, cur.capacity, count, i, entered, entered_capacity, &ctl->out_written[0]);
		if (has_prev) nh_q_events_offset(scan + cur.capacity + 1u, prev.offsets, prev.capacity, count, i, left, left_capacity, &ctl->out_written[1]);
		else left[i] = 0u;
	}
}

__global__ __launch_bounds__(256) void k_q_events_compact(nh_QList cur, nh_QList prev, const uint32_t* __restrict__ scan, const nh_QEventCtl* __restrict__ ctl,
                                                           uint4* __restrict__ entered, uint4* __restrict__ left) {
	const uint64_t words = (uint64_t)cur.capacity + prev.capacity + 1u;          // (the last word is the flag of no record)
	const uint32_t base = scan[cur.capacity + 1u];
	for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t at = scan[w];
		if (scan[w + 1u] == at || w == cur.capacity) continue;
		const bool l = w > cur.capacity;
		const uint32_t r = (uint32_t)(l ? w - cur.capacity - 1u : w), pos = l ? at - base : at;
		if (pos >= ctl->out_written[l ? 1 : 0] || r >= (l ? prev.capacity : cur.capacity)) continue;
		(l ? left : entered)[pos] = reinterpret_cast<const uint4*>(l ? prev.hits : cur.hits)[r];
	}
}

__global__ __launch_bounds__(256) void k_q_bodies_prefix(nh_QList in, uint32_t count, nh_QEventCtl* __restrict__ ctl) {
	if (in.offsets[count] == NH_Q_NONE) return;          // (the marker: nothing was written; in_written stays 0)
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= count; i += gridDim.x * blockDim.x) {
		const uint32_t lo = in.offsets[i];
		if (i == count) { if (lo <= in.capacity) ctl->in_written = lo; continue; }
		const uint32_t hi = in.offsets[i + 1u];
		if (lo <= in.capacity && in.capacity < hi) ctl->in_written = lo;
	}
}

__global__ __launch_bounds__(256) void k_q_bodies_keys(nh_QList in, uint32_t count, const nh_QEventCtl* __restrict__ ctl, uint64_t* __restrict__ keys,
                                                        uint32_t* __restrict__ vals) {
	const uint32_t m = min(ctl->in_written, in.capacity);
	for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < m; r += gridDim.x * blockDim.x) {
		const uint32_t i = min(nh_q_seg_of(in.offsets, count, r), count - 1u);
		keys[r] = ((uint64_t)i << 32) | in.hits[4u * (size_t)r];
		vals[r] = r;
	}
}

__global__ __launch_bounds__(256) void k_q_bodies_flag(const uint64_t* __restrict__ keys, const nh_QEventCtl* __restrict__ ctl, uint32_t capacity,
                                                        uint32_t* __restrict__ scan) {
	const uint32_t m = min(ctl->in_written, capacity);
	for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w <= capacity; w += (uint64_t)gridDim.x * blockDim.x)
		scan[w] = w < m && (w == 0u || keys[w] != keys[w - 1u]) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_q_bodies_offsets(nh_QList in, uint32_t count, const uint32_t* __restrict__ scan, uint32_t* __restrict__ out,
                                                           uint32_t out_capacity, nh_QEventCtl* __restrict__ ctl) {
	const uint32_t m = min(ctl->in_written, in.capacity);          // (the sorted records of segment i lie where the input's did)
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= count; i += gridDim.x * blockDim.x)
		nh_q_events_offset(scan, in.offsets, m, count, i, out, out_capacity, &ctl->out_written[0]);
}

__global__ __launch_bounds__(256) void k_q_bodies_compact(nh_QList in, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ scan,
                                                           const nh_QEventCtl* __restrict__ ctl, uint4* __restrict__ out) {
	const uint32_t m = min(ctl->in_written, in.capacity), written = ctl->out_written[0];
	for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < m; w += gridDim.x * blockDim.x) {
		const uint32_t at = scan[w], r = vals[w];
		if (scan[w + 1u] == at || at >= written || r >= in.capacity) continue;
		out[at] = reinterpret_cast<const uint4*>(in.hits)[r];
	}
}

// The flag and scan words, by record of the input capacities' sum, and the control words (a growth waits for the stream first, as nh_overlap_reserve's does)
static int nh_events_reserve(nh_context* ctx, uint32_t records) {
	nh_QueryState* q = ctx->query;
	if (q->ev_ctl && records <= q->ev_capacity) return NH_OK;
	const uint64_t cap64 = (uint64_t)records + records / 8u + 64u;
	const uint32_t cap = cap64 > 0xfffffffdull ? 0xfffffffdu : (uint32_t)cap64;
	NH_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	q->ev_capacity = 0;
	{ int rc = nh_device_buffers(ctx, { { &q->ev_scan, sizeof(uint32_t) * ((size_t)cap + 2u) }, { &q->ev_ctl, sizeof(nh_QEventCtl) } }); if (rc) return rc; }
	q->ev_capacity = cap;
	return NH_OK;
}

static bool nh_hitlist_ok(const nh_HitList* l) {
	return l && l->offsets && !((uintptr_t)l->offsets & 3u) && !(!l->hits && l->capacity) && !((uintptr_t)l->hits & 15u);
}

static nh_QList nh_hitlist_of(const nh_HitList* l) {
	return l ? nh_QList{ l->offsets, reinterpret_cast<const uint32_t*>(l->hits), l->capacity } : nh_QList{ nullptr, nullptr, 0u };
}

// nh_overlap's checks in nh_overlap's order, then the lists'; then the scratch for `records` record slots.  The caller returns what this returns where
// that is an error or count == 0.
static int nh_events_args(nh_context* ctx, uint32_t count, uint32_t flags, uint32_t known_flags, std::initializer_list<const nh_HitList*> lists, uint64_t records) {
	if (!ctx || !ctx->query || !ctx->query->built) return NH_ERR_INVALID;
	if ((flags & ~known_flags) || count >= NH_Q_MAX_COLLIDERS) return NH_ERR_INVALID;
	if (count == 0u) return NH_OK;
	for (const nh_HitList* l : lists) if (!nh_hitlist_ok(l)) return NH_ERR_INVALID;
	if (records + 2u > 0xffffffffull) return NH_ERR_INVALID;          // (the scan counts its words in 32 bits)
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	{ const int rc = nh_events_reserve(ctx, (uint32_t)records); if (rc) return rc; }
	NH_HIP_CHECK(ctx, hipMemsetAsync(ctx->query->ev_ctl, 0, sizeof(nh_QEventCtl), ctx->stream));
	return NH_OK;
}

extern "C" int nh_overlap_bodies(nh_context* ctx, uint32_t count, const nh_HitList* in, const nh_HitList* out, uint32_t flags) {
	{ const int rc = nh_events_args(ctx, count, flags, 0u, { in, out }, in ? in->capacity : 0u); if (rc || count == 0u) return rc; }
	nh_QueryState* q = ctx->query;
	if (in->capacity == 0u || !in->hits) {          // (a count-only list holds no record: every segment counts 0)
		NH_HIP_CHECK(ctx, hipMemsetAsync(out->offsets, 0, sizeof(uint32_t) * ((size_t)count + 1u), ctx->stream));
		return NH_OK;
	}
	{ const int rc = nh_overlap_reserve(ctx, in->capacity); if (rc) return rc; }
	const nh_QList L = nh_hitlist_of(in);
	const bool list = out->hits != nullptr && out->capacity != 0u;
	const uint32_t per_offset = nh_grid_for((uint64_t)count + 1u, 256, 4096), per_record = nh_grid_for((uint64_t)L.capacity + 1u, 256, 1u << 20);
	NH_LAUNCH(ctx, "q_bodies_prefix", k_q_bodies_prefix, per_offset, 256, L, count, q->ev_ctl);
	NH_LAUNCH(ctx, "q_bodies_keys", k_q_bodies_keys, per_record, 256, L, count, q->ev_ctl, q->ov_keys_a, q->ov_vals_a);
	const int in_b = nh_sort_u64_u32(ctx, q->ov_keys_a, q->ov_keys_b, q->ov_vals_a, q->ov_vals_b, &q->ev_ctl->in_written, q->hist, 0,
	                                 (32 + nh_q_bits(count) + 7) / 8 * 8);
	NH_LAUNCH(ctx, "q_bodies_flag", k_q_bodies_flag, per_record, 256, in_b ? q->ov_keys_b : q->ov_keys_a, q->ev_ctl, L.capacity, q->ev_scan);
	nh_scan_u32(ctx, q->ev_scan, q->ev_scan, &q->ctl->zero, L.capacity + 1u, q->hist, nullptr);
	NH_LAUNCH(ctx, "q_bodies_offsets", k_q_bodies_offsets, per_offset, 256, L, count, q->ev_scan, out->offsets, list ? out->capacity : 0u, q->ev_ctl);
	if (list) NH_LAUNCH(ctx, "q_bodies_compact", k_q_bodies_compact, per_record, 256, L, in_b ? q->ov_vals_b : q->ov_vals_a, q->ev_scan, q->ev_ctl,
	                    reinterpret_cast<uint4*>(out->hits));
	return NH_OK;
}

extern "C" int nh_overlap_events(nh_context* ctx, uint32_t count, const nh_HitList* prev, const nh_HitList* cur, const nh_HitList* entered,
                                 const nh_HitList* left, uint32_t flags) {
	{
		const uint64_t records = (uint64_t)(cur ? cur->capacity : 0u) + (prev ? prev->capacity : 0u);
		const int rc = prev ? nh_events_args(ctx, count, flags, NH_EVENTS_BY_BODY, { cur, entered, left, prev }, records)
		                    : nh_events_args(ctx, count, flags, NH_EVENTS_BY_BODY, { cur, entered, left }, records);
		if (rc || count == 0u) return rc;
	}
	nh_QueryState* q = ctx->query;
	const nh_QList C = nh_hitlist_of(cur), P = nh_hitlist_of(prev);          // (a list without records has capacity 0: the argument rules)
	const bool has_prev = prev != nullptr;
	const bool list_e = entered->hits != nullptr && entered->capacity != 0u, list_l = left->hits != nullptr && left->capacity != 0u;
	const uint32_t words = C.capacity + P.capacity + 2u;
	const uint32_t per_record = nh_grid_for(words, 256, 1u << 20);
	NH_LAUNCH(ctx, "q_events_flag", k_q_events_flag, per_record, 256, C, P, has_prev, count, flags & NH_EVENTS_BY_BODY ? 1u : 0u, q->ev_scan);
	nh_scan_u32(ctx, q->ev_scan, q->ev_scan, &q->ctl->zero, words, q->hist, nullptr);
	NH_LAUNCH(ctx, "q_events_offsets", k_q_events_offsets, nh_grid_for((uint64_t)count + 1u, 256, 4096), 256, C, P, has_prev, count, q->ev_scan, entered->offsets,
	          list_e ? entered->capacity : 0u, left->offsets, list_l ? left->capacity : 0u, q->ev_ctl);
	if (list_e || list_l) NH_LAUNCH(ctx, "q_events_compact", k_q_events_compact, per_record, 256, C, P, q->ev_scan, q->ev_ctl,
	                                reinterpret_cast<uint4*>(entered->hits), reinterpret_cast<uint4*>(left->hits));
	return NH_OK;
}
