// nh_query.hip -- scene queries against the device-resident world: nh_query_build (a linear BVH over every box and sphere collider, built from
// the current transforms), nh_query_refit (the same tree with the boxes of the current transforms), nh_raycast (batched closest-hit / any-hit ray
// casts against the last build or refit), nh_spherecast, nh_boxcast and nh_capsulecast (the same for swept balls, oriented boxes and capsules) and
// nh_overlap (the colliders touching each of a batch of spheres, boxes or capsules, as variable-length segments).  include/nudge_hip.h, "scene queries".
// Layer masks (include/nudge_hip.h, "layer masks"): nh_query_set_layers gives every collider a word of layer bits and every node the OR of the words below it
// (the layer pass, below the box pass); nh_query_filter sets the mask(s) every later query call walks under, in the FILTER = true instantiation of its kernel.
//
// Build (one launch each, plus the library's radix sort):
//   k_q_xform   one lane per collider (boxes, then spheres): world pose (k_xform's arithmetic, nh_query.h) and the record the ray test reads; the
//               bounds of the collider positions by a wave reduction, a reduction over the workgroup's waves in LDS and one atomic per workgroup
//   k_q_keys    48-bit Morton key of each position in the frame of those bounds (nh_morton_scale / nh_morton_of), value = collider index
//   nh_sort_u64_u32  stable: equal keys keep collider order, which the tree's key comparison extends by the sorted index (Karras 2012, 4)
//   k_q_tree    one lane per internal node: range and split from common prefixes, children and parents (the parent word says whether the parent
//               crosses a run boundary, nh_query.h); per split, the node that starts right of it; the list of the top phase's entry nodes
//   k_q_links   one lane per internal node: its escape link, read from that table
//   the box pass, below
// Box pass (the tail of the build, and all of nh_query_refit: it reads the sorted index, the parent words, rchild and right_at of the last build):
//   k_q_boxes_runs  one workgroup per run of NH_Q_RUN consecutive leaves, a lane per leaf: world pose, record and padded leaf box straight from the
//               caller's arrays, then the internal nodes whose range lies inside the run, bottom-up with arrival counters in LDS
//   k_q_boxes_top   behind the kernel boundary, ONE workgroup: the nodes whose range crosses a run boundary, from the entry list, with arrival
//               counters in global memory at workgroup scope
// Node ids: internal nodes 0 .. n-2 (root 0), leaf j (j-th collider in key order) n-1+j; with one collider the root is that leaf.
// Traversal is stackless: a node that is missed or a leaf that is done continues at its ESCAPE link (the next node in pre-order after its subtree),
// a hit internal node at its left child.  A private stack array would go to scratch memory.
#include <type_traits>
#include <utility>
#include "nh_internal.h"
#include "nh_query.h"

#define NH_Q_LEAF 0x80000000u
#define NH_Q_NONE 0xffffffffu
#define NH_Q_MAX_COLLIDERS (1u << 30)

// The ray test's record of a collider, by collider index: a = (world position, bits(body)), b = world rotation, c = (half extents | radius, -, -,
// bits(tag))
struct nh_QRec { float4 a, b, c; };
// A node: a = (box min, left child | NH_Q_LEAF + collider), b = (box max, escape link)
struct nh_QNode { float4 a, b; };
// words the build's kernels share: collider count (the sort reads it), bounds of the positions (flipped floats); nh_overlap's: a word that stays 0
// (the element count of its scan is all `extra`), the length of the written prefix of records (its sort and gather read it), the wrap flag; the bounds
// of the LAST build (k_q_tree keeps them there before it resets smin / smax: nh_closest's seed finds a point's place among the keys in their frame);
// the box pass's: the number of entry nodes of the top phase (k_q_tree counts them) and the height of the tree of top nodes (k_q_boxes_top, for
// nh_query_stats).  A refit touches top_depth alone.
struct nh_QCtl { uint32_t count, zero, ov_written, ov_wrap; uint32_t smin[4]; uint32_t smax[4]; uint32_t kmin[4]; uint32_t kmax[4];
                 uint32_t top_n, top_depth, pad0, pad1; };

struct nh_QueryState {
	uint32_t capacity;           // colliders the buffers have room for
	bool built;
	uint32_t n, nbox;            // of the last build
	nh_QCtl* ctl;
	nh_QRec* rec;
	uint64_t* keys_a; uint64_t* keys_b; uint32_t* idx_a; uint32_t* idx_b; uint32_t* hist;
	const uint64_t* keys;        // the sorted keys of the last build (keys_a or keys_b, as the sort left them): leaf j's is keys[j]
	const uint32_t* idx;         // the leaf order of the last build (idx_a or idx_b): leaf j is collider idx[j]
	nh_QNode* nodes;             // 2 n - 1
	uint32_t* parent;            // by node id: nh_q_parent_word (nh_query.h)
	uint32_t* rchild;            // by internal node
	uint32_t* last;              // by internal node: last leaf of its range
	uint32_t* right_at;          // by split position: the right child of the node that splits there
	uint32_t* arrive;            // by internal node: arrival counter of the top phase (0 between launches)
	uint32_t* top;               // the entry nodes of the top phase: nodes inside one run whose parent crosses a run boundary (ctl->top_n of them)
	uint32_t ov_capacity;        // nh_overlap's sort scratch, by record of the caller's capacity
	uint64_t* ov_keys_a; uint64_t* ov_keys_b; uint32_t* ov_vals_a; uint32_t* ov_vals_b;
	// layer masks (header, "layer masks"): the layer word of every collider of the last build, by combined index, and per node the OR of the words of
	// the leaves below it (2 n - 1 words by node id, the layer pass writes them); both are only meaningful while layers_set
	uint32_t layer_capacity;     // colliders the two arrays have room for
	bool layers_set;
	uint32_t* layers;
	uint32_t* node_layers;
	uint32_t filter_mode;        // NH_FILTER_*: context state, read by every query call
	uint32_t filter_mask;
	const uint32_t* filter_masks;   // the caller's, kept by pointer (NH_FILTER_PER_QUERY)
};

// the caller's arrays as the kernels read them
struct nh_QWorld {
	const nh_Transform* body_xf; uint32_t nbodies;
	const nh_Transform* box_xf; const nh_BoxCollider* box_data; const uint32_t* box_tags; uint32_t nbox;
	const nh_Transform* sph_xf; const nh_SphereCollider* sph_data; const uint32_t* sph_tags; uint32_t nsph;
};

// Collider c (combined index): its record, and the half extents of its world AABB
__device__ __forceinline__ nh_f3 nh_q_collider(const nh_QWorld& W, uint32_t c, nh_QRec& r) {
	const bool is_box = c < W.nbox;
	const nh_Transform l = is_box ? W.box_xf[c] : W.sph_xf[c - W.nbox];
	nh_QPose w;
	nh_f3 h;
	if (l.body < W.nbodies) {
		const nh_Transform b = W.body_xf[l.body];
		w = nh_q_pose(b.position, b.rotation, l.position, l.rotation);
	} else {
		// (a collider of a body that does not exist: never hit, never in the bounds)
		const float q = __uint_as_float(0x7fc00000u);
		w.p = nh_make3(q, q, q); w.q = { q, q, q, q };
	}
	if (is_box) {
		const nh_BoxCollider bc = W.box_data[c];
		h = nh_make3(bc.size[0], bc.size[1], bc.size[2]);
	} else {
		const float rad = W.sph_data[c - W.nbox].radius;
		h = nh_make3(rad, rad, rad);
	}
	const uint32_t tag = is_box ? W.box_tags[c] : W.sph_tags[c - W.nbox];
	r.a = make_float4(w.p.x, w.p.y, w.p.z, __uint_as_float(l.body));
	r.b = make_float4(w.q.x, w.q.y, w.q.z, w.q.s);
	r.c = make_float4(h.x, h.y, h.z, __uint_as_float(tag));
	return is_box ? nh_q_box_extent(w.q, h) : h;
}

// ---- build ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_q_xform(nh_QWorld W, nh_QRec* __restrict__ rec, nh_QCtl* __restrict__ ctl) {
	__shared__ uint32_t wave_min[4][3], wave_max[4][3];
	const uint32_t n = W.nbox + W.nsph;
	if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->count = n; ctl->top_n = 0u; ctl->top_depth = 0u; }
	uint32_t lmin[3] = { 0xffffffffu, 0xffffffffu, 0xffffffffu }, lmax[3] = { 0u, 0u, 0u };
	for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
		nh_QRec r;
		nh_q_collider(W, c, r);
		rec[c] = r;
		if (r.a.x == r.a.x && r.a.y == r.a.y && r.a.z == r.a.z) {
			uint32_t f;
			f = nh_float_flip(r.a.x); lmin[0] = min(lmin[0], f); lmax[0] = max(lmax[0], f);
			f = nh_float_flip(r.a.y); lmin[1] = min(lmin[1], f); lmax[1] = max(lmax[1], f);
			f = nh_float_flip(r.a.z); lmin[2] = min(lmin[2], f); lmax[2] = max(lmax[2], f);
		}
	}
	for (int k = 0; k < 3; ++k) {
		for (int d = 32; d >= 1; d >>= 1) {
			lmin[k] = min(lmin[k], (uint32_t)__shfl_xor((int)lmin[k], d));
			lmax[k] = max(lmax[k], (uint32_t)__shfl_xor((int)lmax[k], d));
		}
	}
	if (nh_lane() == 0) {
		for (int k = 0; k < 3; ++k) { wave_min[threadIdx.x >> 6][k] = lmin[k]; wave_max[threadIdx.x >> 6][k] = lmax[k]; }
	}
	__syncthreads();
	if (threadIdx.x < 3u) {
		const uint32_t k = threadIdx.x;
		const uint32_t mn = min(min(wave_min[0][k], wave_min[1][k]), min(wave_min[2][k], wave_min[3][k]));
		const uint32_t mx = max(max(wave_max[0][k], wave_max[1][k]), max(wave_max[2][k], wave_max[3][k]));
		// (no finite position in this workgroup: mn stays all ones and mx 0, which change nothing)
		if (mn <= mx) { atomicMin(&ctl->smin[k], mn); atomicMax(&ctl->smax[k], mx); }
	}
}

__global__ __launch_bounds__(256) void k_q_keys(const nh_QRec* __restrict__ rec, const nh_QCtl* __restrict__ ctl, uint32_t n,
                                                uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
	const nh_f3 smin = nh_make3(nh_float_unflip(ctl->smin[0]), nh_float_unflip(ctl->smin[1]), nh_float_unflip(ctl->smin[2]));
	const nh_f3 smax = nh_make3(nh_float_unflip(ctl->smax[0]), nh_float_unflip(ctl->smax[1]), nh_float_unflip(ctl->smax[2]));
	const float scale = nh_morton_scale(smin, smax);
	const nh_f3 smin_scaled = smin * scale;
	for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
		const float4 a = rec[c].a;
		keys[c] = nh_morton_of(nh_make3(a.x, a.y, a.z), scale, smin_scaled);
		idx[c] = c;
	}
}

// Karras 2012: length of the common prefix of the keys at sorted positions i and j, extended by the positions themselves on equal keys; -1 outside
__device__ __forceinline__ int nh_q_delta(const uint64_t* __restrict__ keys, uint32_t n, int64_t i, int64_t j) {
	if (j < 0 || j >= (int64_t)n) return -1;
	const uint64_t a = keys[i], b = keys[j];
	if (a == b) return 64 + __clz((uint32_t)i ^ (uint32_t)j);
	return __clzll(a ^ b);
}

__global__ __launch_bounds__(256) void k_q_tree(const uint64_t* __restrict__ keys, uint32_t n, nh_QNode* __restrict__ nodes, uint32_t* __restrict__ parent,
                                                uint32_t* __restrict__ rchild, uint32_t* __restrict__ last, uint32_t* __restrict__ right_at,
                                                uint32_t* __restrict__ arrive, uint32_t* __restrict__ top, nh_QCtl* __restrict__ ctl) {
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		parent[0] = NH_Q_NONE;
		// the bounds the next build accumulates into (k_q_keys of this one has read them); this build's are kept for nh_closest
		for (int k = 0; k < 3; ++k) { ctl->kmin[k] = ctl->smin[k]; ctl->kmax[k] = ctl->smax[k]; ctl->smin[k] = 0xffffffffu; ctl->smax[k] = 0u; }
	}
	// (whole waves go round together: the entry list is reserved per wave)
	for (uint32_t u0 = blockIdx.x * blockDim.x; u0 + 1u < n; u0 += gridDim.x * blockDim.x) {
		const uint32_t u = u0 + threadIdx.x;
		bool enter_left = false, enter_right = false;
		uint32_t left = 0u, right = 0u;
		if (u + 1u < n) {
			const int64_t i = u;
			const int d = nh_q_delta(keys, n, i, i + 1) > nh_q_delta(keys, n, i, i - 1) ? 1 : -1;
			const int dmin = nh_q_delta(keys, n, i, i - d);
			int64_t lmax = 2;
			while (nh_q_delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
			int64_t l = 0;
			for (int64_t t = lmax / 2; t >= 1; t /= 2)
				if (nh_q_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
			const int64_t j = i + l * d;
			const int dnode = nh_q_delta(keys, n, i, j);
			int64_t s = 0, t = l;
			do {
				t = (t + 1) / 2;
				if (nh_q_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
			} while (t > 1);
			const int64_t gamma = i + s * d + (d < 0 ? -1 : 0);
			const int64_t first = i < j ? i : j, end = i < j ? j : i;
			left = first == gamma ? (uint32_t)(n - 1u + gamma) : (uint32_t)gamma;
			right = end == gamma + 1 ? (uint32_t)(n - 1u + gamma + 1) : (uint32_t)(gamma + 1);
			nodes[u].a.w = __uint_as_float(left);
			rchild[u] = right;
			last[u] = (uint32_t)end;
			right_at[gamma] = right;
			const bool crossing = nh_q_run_crossing((uint32_t)first, (uint32_t)end);
			parent[left] = nh_q_parent_word(u, false, crossing);
			parent[right] = nh_q_parent_word(u, true, crossing);
			arrive[u] = 0u;
			// the top phase starts at the children that lie inside one run
			enter_left = crossing && !nh_q_run_crossing((uint32_t)first, (uint32_t)gamma);
			enter_right = crossing && !nh_q_run_crossing((uint32_t)gamma + 1u, (uint32_t)end);
		}
		const uint32_t at_left = nh_wave_reserve1(&ctl->top_n, enter_left);
		if (enter_left) top[at_left] = left;
		const uint32_t at_right = nh_wave_reserve1(&ctl->top_n, enter_right);
		if (enter_right) top[at_right] = right;
	}
}

// escape links of the internal nodes: the subtree of a node ends at the last leaf of its range; the next node in pre-order is the right child of the
// split there (a leaf's is right_at[its position]: k_q_boxes_runs writes it with the leaf)
__global__ __launch_bounds__(256) void k_q_links(uint32_t n, nh_QNode* __restrict__ nodes, const uint32_t* __restrict__ last, const uint32_t* __restrict__ right_at) {
	for (uint32_t u = blockIdx.x * blockDim.x + threadIdx.x; u + 1u < n; u += gridDim.x * blockDim.x) {
		const uint32_t e = last[u];
		nodes[u].b.w = __uint_as_float(e + 1u == n ? NH_Q_NONE : right_at[e]);
	}
}

// ---- box pass -------------------------------------------------------------------------------------------------------------------------------
// Bottom phase.  Workgroup b owns leaves [b * NH_Q_RUN, (b + 1) * NH_Q_RUN) and the internal nodes whose range lies inside them (nh_query.h): LDS slot
// = node index - run start.  A slot holds the boxes of the node's two children, by side, and its arrival counter: a lane puts its box on its side,
// then counts itself in; the second to arrive reads the other side, merges and goes on with the parent, until the parent word says "top".  Every
// hand-off is inside the workgroup: LDS stores released and acquired at workgroup scope by the counter's atomic, no agent-scope fence, no global
// atomic.  fminf / fmaxf: the boxes do not depend on who arrives first, and a NaN leaf (a body that does not exist) drops out of its ancestors.
// The finished nodes leave through the slots after a barrier (the .w words of an internal node, child and escape links, stay as the build wrote them).
__global__ __launch_bounds__(NH_Q_RUN) void k_q_boxes_runs(nh_QWorld W, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ parent,
                                                           const uint32_t* __restrict__ right_at, uint32_t n, nh_QRec* __restrict__ rec, nh_QNode* __restrict__ nodes) {
	__shared__ float child_box[NH_Q_RUN][2][6];
	__shared__ uint32_t arrived[NH_Q_RUN];
	__shared__ uint32_t up[NH_Q_RUN];            // parent words of the run's internal nodes
	const uint32_t base = blockIdx.x * NH_Q_RUN, s = threadIdx.x, j = base + s;
	arrived[s] = 0u;
	up[s] = j + 1u < n ? parent[j] : NH_Q_NONE;
	uint32_t pw = NH_Q_NONE;
	float lo[3] = { 0.0f, 0.0f, 0.0f }, hi[3] = { 0.0f, 0.0f, 0.0f };
	if (j < n) {
		const uint32_t c = idx[j];
		nh_QRec r;
		const nh_f3 e = nh_q_collider(W, c, r);
		rec[c] = r;
		const nh_f3 mn = nh_make3(r.a.x - e.x, r.a.y - e.y, r.a.z - e.z), mx = nh_make3(r.a.x + e.x, r.a.y + e.y, r.a.z + e.z);
		const float pad = nh_q_pad(mn, mx);      // (nh_query.h: the host's sweep rule rebuilds this box)
		lo[0] = mn.x - pad; lo[1] = mn.y - pad; lo[2] = mn.z - pad;
		hi[0] = mx.x + pad; hi[1] = mx.y + pad; hi[2] = mx.z + pad;
		nh_QNode leaf;
		leaf.a = make_float4(lo[0], lo[1], lo[2], __uint_as_float(NH_Q_LEAF | c));
		leaf.b = make_float4(hi[0], hi[1], hi[2], __uint_as_float(j + 1u == n ? NH_Q_NONE : right_at[j]));
		nodes[n - 1u + j] = leaf;
		pw = parent[n - 1u + j];
	}
	__syncthreads();
	while (!(pw & NH_Q_PARENT_TOP)) {
		const uint32_t slot = (pw & NH_Q_PARENT_ID) - base, side = (pw & NH_Q_PARENT_RIGHT) ? 1u : 0u;
		float* mine = child_box[slot][side];
		for (int k = 0; k < 3; ++k) { mine[k] = lo[k]; mine[3 + k] = hi[k]; }
		const uint32_t before = __hip_atomic_fetch_add(&arrived[slot], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
		if (before == 0u) break;
		const float* other = child_box[slot][side ^ 1u];
		for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], other[k]); hi[k] = fmaxf(hi[k], other[3 + k]); }
		pw = up[slot];
	}
	__syncthreads();
	if (arrived[s] == 2u) {
		const float* l = child_box[s][0];
		const float* r = child_box[s][1];
		float* a = reinterpret_cast<float*>(&nodes[j].a);
		float* b = reinterpret_cast<float*>(&nodes[j].b);
		for (int k = 0; k < 3; ++k) { a[k] = fminf(l[k], r[k]); b[k] = fmaxf(l[3 + k], r[3 + k]); }
	}
}

// Top phase: the nodes that cross a run boundary -- with B runs at most B - 2 have two crossing children, the rest are chains with one child finished
// below; few (nh_query_stats counts them) but deep.  The launch boundary has made k_q_boxes_runs' boxes visible.  ONE workgroup climbs from the entry
// list: a lane whose box is in nodes[] counts itself in at the parent; the second to arrive merges its sibling's box, writes the parent and goes on.
// All hand-offs are between waves of this one workgroup -- one CU, one L1, one L2 -- so the counter's atomic releases and acquires at WORKGROUP
// scope and nothing in the pass needs an agent-scope fence.  The second arriver leaves the counter at 0 for the next pass.  The counter's upper 24
// bits carry the first arriver's height, so that the root's lane knows the height of the top tree (the longest chain, for nh_query_stats).
#define NH_Q_TOP_BLOCK 1024
__global__ __launch_bounds__(NH_Q_TOP_BLOCK) void k_q_boxes_top(const uint32_t* __restrict__ top, nh_QCtl* ctl, nh_QNode* nodes,
                                                                const uint32_t* __restrict__ parent, const uint32_t* __restrict__ rchild, uint32_t* arrive) {
	const uint32_t m = ctl->top_n;
	for (uint32_t e = threadIdx.x; e < m; e += NH_Q_TOP_BLOCK) {
		const uint32_t me = top[e];
		float4 mn = nodes[me].a, mx = nodes[me].b;
		uint32_t height = 0u;
		uint32_t pw = parent[me];
		while (pw != NH_Q_NONE) {
			const uint32_t id = pw & NH_Q_PARENT_ID;
			const uint32_t before = __hip_atomic_fetch_add(&arrive[id], 1u | (height << 8), __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
			if ((before & 0xffu) == 0u) break;
			__hip_atomic_store(&arrive[id], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			height = min(max(height, before >> 8) + 1u, 0xffffffu);
			const uint32_t other = (pw & NH_Q_PARENT_RIGHT) ? __float_as_uint(nodes[id].a.w) : rchild[id];
			const float4 omn = nodes[other].a, omx = nodes[other].b;
			mn = make_float4(fminf(mn.x, omn.x), fminf(mn.y, omn.y), fminf(mn.z, omn.z), 0.0f);
			mx = make_float4(fmaxf(mx.x, omx.x), fmaxf(mx.y, omx.y), fmaxf(mx.z, omx.z), 0.0f);
			float* a = reinterpret_cast<float*>(&nodes[id].a);
			float* b = reinterpret_cast<float*>(&nodes[id].b);
			a[0] = mn.x; a[1] = mn.y; a[2] = mn.z;
			b[0] = mx.x; b[1] = mx.y; b[2] = mx.z;
			pw = parent[id];
		}
		if (pw == NH_Q_NONE) ctl->top_depth = height;
	}
}

// ---- layer pass ------------------------------------------------------------------------------------------------------------------------------
// Per node, the OR of the layer words of the leaves below it: the box pass's split with a word in place of a box.  It reads the sorted index, the parent
// words, rchild and the entry list of the last build and counts arrivals as the box pass does; it runs behind nh_query_set_layers and at the tail of a
// build while layers are set, never in a refit (the topology stands).
// Bottom phase: workgroup b gathers the words of its run's colliders into leaf order and climbs inside the run, every hand-off in LDS, released and
// acquired at workgroup scope by the counter's atomic.  OR does not depend on who arrives first.
__global__ __launch_bounds__(NH_Q_RUN) void k_q_layers_runs(const uint32_t* __restrict__ layers, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ parent,
                                                            uint32_t n, uint32_t* __restrict__ node_layers) {
	__shared__ uint32_t child_word[NH_Q_RUN][2];
	__shared__ uint32_t arrived[NH_Q_RUN];
	__shared__ uint32_t up[NH_Q_RUN];            // parent words of the run's internal nodes
	const uint32_t base = blockIdx.x * NH_Q_RUN, s = threadIdx.x, j = base + s;
	arrived[s] = 0u;
	up[s] = j + 1u < n ? parent[j] : NH_Q_NONE;
	uint32_t pw = NH_Q_NONE, word = 0u;
	if (j < n) {
		word = layers[idx[j]];
		node_layers[n - 1u + j] = word;
		pw = parent[n - 1u + j];
	}
	__syncthreads();
	while (!(pw & NH_Q_PARENT_TOP)) {
		const uint32_t slot = (pw & NH_Q_PARENT_ID) - base, side = (pw & NH_Q_PARENT_RIGHT) ? 1u : 0u;
		child_word[slot][side] = word;
		const uint32_t before = __hip_atomic_fetch_add(&arrived[slot], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
		if (before == 0u) break;
		word |= child_word[slot][side ^ 1u];
		pw = up[slot];
	}
	__syncthreads();
	if (arrived[s] == 2u) node_layers[j] = child_word[s][0] | child_word[s][1];
}

// Top phase, behind the kernel boundary: k_q_boxes_top's climb from the entry list in ONE workgroup, the same counters (0 between launches, left at 0),
// hand-offs at workgroup scope.
__global__ __launch_bounds__(NH_Q_TOP_BLOCK) void k_q_layers_top(const uint32_t* __restrict__ top, const nh_QCtl* __restrict__ ctl, const nh_QNode* __restrict__ nodes,
                                                                 const uint32_t* __restrict__ parent, const uint32_t* __restrict__ rchild, uint32_t* arrive,
                                                                 uint32_t* node_layers) {
	const uint32_t m = ctl->top_n;
	for (uint32_t e = threadIdx.x; e < m; e += NH_Q_TOP_BLOCK) {
		const uint32_t me = top[e];
		uint32_t word = node_layers[me];
		uint32_t pw = parent[me];
		while (pw != NH_Q_NONE) {
			const uint32_t id = pw & NH_Q_PARENT_ID;
			const uint32_t before = __hip_atomic_fetch_add(&arrive[id], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
			if (before == 0u) break;
			__hip_atomic_store(&arrive[id], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			const uint32_t other = (pw & NH_Q_PARENT_RIGHT) ? __float_as_uint(nodes[id].a.w) : rchild[id];
			word |= node_layers[other];
			node_layers[id] = word;
			pw = parent[id];
		}
	}
}

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
	__device__ __forceinline__ void read(const float4* __restrict__ cp) {
		head(cp[0], cp[1]);
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
	__device__ __forceinline__ void read(const float4* __restrict__ cp) {
		head(cp[0], cp[1]);
		const float4 c2 = cp[2], c3 = cp[3];
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
	__device__ __forceinline__ void read(const float4* __restrict__ cp) {
		head(cp[0], cp[1]);
		const float4 c2 = cp[2], c3 = cp[3];
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

// One lane per cast: the walk prunes at the best t so far, nh_q_better (nh_query.h) keeps the closest hit and the tie rule, any_hit stops at the first.
template <class Shape, bool FILTER>
__device__ __forceinline__ void nh_q_cast(const float4* __restrict__ casts, uint32_t count, nh_RayHit* __restrict__ hits, const nh_QNode* __restrict__ nodes,
                                          const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox, uint32_t any_hit, const nh_QFilter& F) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
		Shape k;
		k.read(casts + (size_t)i * Shape::WORDS);
		float bt = k.max_t;
		uint32_t bc = NH_Q_NONE;
		nh_f3 bn = nh_make3(0.0f, 0.0f, 0.0f);
		nh_q_walk<FILTER>(nodes, rec, k.ok && n ? 0u : NH_Q_NONE, k.ignore, F, FILTER ? F.of(i) : 0u,
			[&](nh_f3 lo, nh_f3 hi, float& t0) { return k.node(lo, hi, t0) && t0 <= bt; },
			[&](uint32_t c, const nh_QRec& q, float t0) {
				const nh_QHit h = k.leaf(nh_q_unpack(q), c < nbox, t0);
				if (!(h.hit && nh_q_better(h.t, c, k.max_t, bt, bc))) return false;
				bt = h.t; bc = c; bn = h.n;
				return any_hit != 0u;
			});
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

template <bool FILTER>
__global__ __launch_bounds__(256) void k_q_closest(const nh_PointQuery* __restrict__ queries, uint32_t count, nh_PointHit* __restrict__ hits,
                                                   const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec, const uint64_t* __restrict__ keys,
                                                   const nh_QCtl* __restrict__ ctl, uint32_t n, uint32_t nbox, nh_QFilter F) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
		const float4* qp = reinterpret_cast<const float4*>(queries + i);
		const float4 q0 = qp[0], q1 = qp[1];
		const nh_f3 p = nh_make3(q0.x, q0.y, q0.z);
		const float max_d = q0.w;
		const uint32_t ignore = __float_as_uint(q1.x);
		const bool ok = nh_q_finite(p) && max_d >= 0.0f;       // (+inf is a valid max_distance; NaN is not)
		float bd = max_d;
		uint32_t bc = NH_Q_NONE;
		nh_f3 bn = nh_make3(0.0f, 0.0f, 0.0f), bx = nh_make3(0.0f, 0.0f, 0.0f);
		const bool walk = ok && n;
		const uint32_t fm = FILTER ? F.of(i) : 0u;
		// a leaf of squared box distance d2, for the seed and the walk alike
		const auto leaf = [&](uint32_t c, const nh_QRec& q, float d2) {
			const nh_QShape s = nh_q_unpack(q);
			const nh_QPoint h = c < nbox ? nh_q_point_box(p, s.p, s.q, s.h) : nh_q_point_sphere(p, s.p, s.h.x);
			const float k = nh_q_point_key(h.d, d2);
			if (nh_q_closer(k, c, max_d, bd, bc)) { bd = k; bc = c; bn = h.n; bx = h.x; }
			return false;
		};
#ifndef NH_Q_CLOSEST_NO_SEED
		if (walk) nh_q_seed<FILTER>(p, NH_Q_SEED, ignore, nodes, rec, keys, ctl, n, F, fm, [&](uint32_t c, const nh_QRec& q, nh_f3 lo, nh_f3 hi) { leaf(c, q, nh_q_point_node(lo, hi, p)); });
#endif
		nh_q_walk<FILTER>(nodes, rec, walk ? 0u : NH_Q_NONE, ignore, F, fm,
			[&](nh_f3 lo, nh_f3 hi, float& d2) { d2 = nh_q_point_node(lo, hi, p); return !(d2 > 0.0f && sqrtf(d2) > bd); }, leaf);
		float4* hp = reinterpret_cast<float4*>(hits + i);
		if (bc == NH_Q_NONE) {
			const float md = ok ? max_d : __uint_as_float(0x7fc00000u);
			hp[0] = make_float4(md, 0.0f, 0.0f, 0.0f);
			hp[1] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(NH_Q_NONE));
			hp[2] = make_float4(__uint_as_float(NH_Q_NONE), __uint_as_float(NH_SHAPE_NONE), __uint_as_float(NH_Q_NONE), 0.0f);
		} else {
			const uint4 id = nh_q_identity(bc, nbox, rec[bc]);
			hp[0] = make_float4(bd, bn.x, bn.y, bn.z);
			hp[1] = make_float4(bx.x, bx.y, bx.z, __uint_as_float(id.x));
			hp[2] = make_float4(__uint_as_float(id.y), __uint_as_float(id.z), __uint_as_float(id.w), 0.0f);
		}
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
		const float4* qp = reinterpret_cast<const float4*>(queries + i);
		const float4 q0 = qp[0], q1 = qp[1];
		const nh_f3 p = nh_make3(q0.x, q0.y, q0.z);
		const float max_d = q0.w;
		const uint32_t ignore = __float_as_uint(q1.x);
		const bool ok = nh_q_finite(p) && max_d >= 0.0f;       // (+inf is a valid max_distance; NaN is not)
		float bd = max_d;
		uint32_t held = 0u;
		const bool walk = ok && n;
		const uint32_t fm = FILTER ? F.of(i) : 0u;
		// a leaf of squared box distance d2, for the seed and the walk alike
		const auto leaf = [&](uint32_t c, const nh_QRec& q, float d2) {
			const nh_QShape s = nh_q_unpack(q);
			const nh_QPoint h = c < nbox ? nh_q_point_box(p, s.p, s.q, s.h) : nh_q_point_sphere(p, s.p, s.h.x);
			const float key = nh_q_point_key(h.d, d2);
			if (!(key <= bd)) return false;
			if (nh_q_nearest_insert(list, stride, k, &held, key, c, max_d) && held == k) bd = list[(k - 1u) * stride].key;
			return false;
		};
#ifndef NH_Q_CLOSEST_K_NO_SEED
		if (walk) nh_q_seed<FILTER>(p, NH_Q_SEED + k / 2u, ignore, nodes, rec, keys, ctl, n, F, fm, [&](uint32_t c, const nh_QRec& q, nh_f3 lo, nh_f3 hi) { leaf(c, q, nh_q_point_node(lo, hi, p)); });
#endif
		nh_q_walk<FILTER>(nodes, rec, walk ? 0u : NH_Q_NONE, ignore, F, fm,
			[&](nh_f3 lo, nh_f3 hi, float& d2) { d2 = nh_q_point_node(lo, hi, p); return !(d2 > 0.0f && sqrtf(d2) > bd); }, leaf);
		float4* hp = reinterpret_cast<float4*>(hits + (size_t)i * k);
		for (uint32_t j = 0u; j < held; ++j, hp += 3) {
			const nh_QNear e = list[j * stride];
			const nh_QRec q = rec[e.c];
			const nh_QShape s = nh_q_unpack(q);
			const nh_QPoint h = e.c < nbox ? nh_q_point_box(p, s.p, s.q, s.h) : nh_q_point_sphere(p, s.p, s.h.x);
			const uint4 id = nh_q_identity(e.c, nbox, q);
			hp[0] = make_float4(e.key, h.n.x, h.n.y, h.n.z);
			hp[1] = make_float4(h.x.x, h.x.y, h.x.z, __uint_as_float(id.x));
			hp[2] = make_float4(__uint_as_float(id.y), __uint_as_float(id.z), __uint_as_float(id.w), 0.0f);
		}
		const float md = ok ? max_d : __uint_as_float(0x7fc00000u);
		for (uint32_t j = held; j < k; ++j, hp += 3) {
			hp[0] = make_float4(md, 0.0f, 0.0f, 0.0f);
			hp[1] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(NH_Q_NONE));
			hp[2] = make_float4(__uint_as_float(NH_Q_NONE), __uint_as_float(NH_SHAPE_NONE), __uint_as_float(NH_Q_NONE), 0.0f);
		}
		if (counts) counts[i] = held;
	}
}

// ---- distance ---------------------------------------------------------------------------------------------------------------------------------
// nh_distance: one lane per query shape on nh_q_walk, k_q_closest with a volume in place of the point.
//   decode  k_q_overlap's: the shape, its validity (nh_overlap's, and max_distance >= 0), the half axis of a capsule, the world AABB [qlo, qhi] (not padded)
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
		const float4 q0 = qp[0], q1 = qp[1], q2 = qp[2];
		const float max_d = qp[3].x;          // (the record moves as four 16-byte words; of the fourth only .x is used: `reserved` takes part in nothing)
		const nh_f3 c = nh_make3(q0.x, q0.y, q0.z), h = nh_make3(q2.x, q2.y, q2.z);
		const nh_quat qr = { q1.x, q1.y, q1.z, q1.w };
		const uint32_t shape = __float_as_uint(q0.w), ignore = __float_as_uint(q2.w);
		// (a capsule of half height 0 is a sphere query: the same functions, its rotation not read)
		const bool capsule = shape == NH_SHAPE_CAPSULE && h.y != 0.0f;
		const bool sphere = !capsule && (shape == NH_SHAPE_SPHERE || shape == NH_SHAPE_CAPSULE);
		bool ok = (sphere || capsule || shape == NH_SHAPE_BOX) && nh_q_finite(c) && nh_q_finite(h.x) && !(h.x < 0.0f) && max_d >= 0.0f;
		if (!sphere) ok = ok && nh_q_finite(h.y) && !(h.y < 0.0f) && nh_q_finite(qr);
		if (!sphere && !capsule) ok = ok && nh_q_finite(h.z) && !(h.z < 0.0f);
		const nh_f3 a = capsule ? nh_q_capsule_axis(qr, h.y) : nh_make3(0.0f, 0.0f, 0.0f);
		const nh_f3 e = sphere ? nh_make3(h.x, h.x, h.x) : capsule ? nh_q_capsule_extent(a, h.x) : nh_q_box_extent(qr, h);
		const nh_f3 qlo = c - e, qhi = c + e;
		float bd = max_d;
		uint32_t bc = NH_Q_NONE;
		nh_f3 bn = nh_make3(0.0f, 0.0f, 0.0f), bx = nh_make3(0.0f, 0.0f, 0.0f);
		const bool walk = ok && n;
		const uint32_t fm = FILTER ? F.of(i) : 0u;
		// a leaf at squared box gap g2, for the seed and the walk alike
		const auto leaf = [&](uint32_t cc, const nh_QRec& r, float g2) {
			const nh_QShape s = nh_q_unpack(r);
			nh_QPoint d;
			if (capsule) d = cc < nbox ? nh_q_dist_capsule_box_a(c, a, h.x, s.p, s.q, s.h) : nh_q_dist_capsule_sphere_a(c, a, h.x, s.p, s.h.x);
			else if (cc < nbox) d = sphere ? nh_q_dist_sphere_box(c, h.x, s.p, s.q, s.h) : nh_q_dist_box_box(c, qr, h, s.p, s.q, s.h);
			else d = sphere ? nh_q_dist_sphere_sphere(c, h.x, s.p, s.h.x) : nh_q_dist_box_sphere(c, qr, h, s.p, s.h.x);
			const float k = nh_q_point_key(d.d, g2);
			if (nh_q_closer(k, cc, max_d, bd, bc)) { bd = k; bc = cc; bn = d.n; bx = d.x; }
			return false;
		};
		if (walk) nh_q_seed<FILTER>(c, NH_Q_SEED, ignore, nodes, rec, keys, ctl, n, F, fm, [&](uint32_t cc, const nh_QRec& r, nh_f3 lo, nh_f3 hi) { leaf(cc, r, nh_q_dist_node(lo, hi, qlo, qhi)); });
		nh_q_walk<FILTER>(nodes, rec, walk ? 0u : NH_Q_NONE, ignore, F, fm,
			[&](nh_f3 lo, nh_f3 hi, float& g2) { g2 = nh_q_dist_node(lo, hi, qlo, qhi); return !(g2 > 0.0f && sqrtf(g2) > bd); }, leaf);
		float4* hp = reinterpret_cast<float4*>(hits + i);
		if (bc == NH_Q_NONE) {
			const float md = ok ? max_d : __uint_as_float(0x7fc00000u);
			hp[0] = make_float4(md, 0.0f, 0.0f, 0.0f);
			hp[1] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(NH_Q_NONE));
			hp[2] = make_float4(__uint_as_float(NH_Q_NONE), __uint_as_float(NH_SHAPE_NONE), __uint_as_float(NH_Q_NONE), 0.0f);
		} else {
			const uint4 id = nh_q_identity(bc, nbox, rec[bc]);
			hp[0] = make_float4(bd, bn.x, bn.y, bn.z);
			hp[1] = make_float4(bx.x, bx.y, bx.z, __uint_as_float(id.x));
			hp[2] = make_float4(__uint_as_float(id.y), __uint_as_float(id.z), __uint_as_float(id.w), 0.0f);
		}
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
	if (!LIST && !CAPSULE && blockIdx.x == 0 && threadIdx.x == 0) { offsets[count] = 0u; ctl->ov_wrap = 0u; ctl->ov_written = 0u; }   // (k_q_overlap_fix sets both)
	const uint32_t written = LIST ? ctl->ov_written : 0u;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
		uint32_t base = 0u, end = 0u;
		if (LIST) {
			base = offsets[i]; end = offsets[i + 1u];
			if (!(base < end && end <= written)) continue;          // empty, or not in the written prefix
		}
		const float4* qp = reinterpret_cast<const float4*>(queries + i);
		const float4 q0 = qp[0], q1 = qp[1], q2 = qp[2];
		const nh_f3 c = nh_make3(q0.x, q0.y, q0.z), h = nh_make3(q2.x, q2.y, q2.z);
		const nh_quat qr = { q1.x, q1.y, q1.z, q1.w };
		const uint32_t shape = __float_as_uint(q0.w), ignore = __float_as_uint(q2.w);
		// (a capsule of half height 0 is a sphere query: the same walk, the same predicates, its rotation not read.  Every other capsule -- an invalid
		// half height included -- is the CAPSULE instantiation's, and only its)
		if ((shape == NH_SHAPE_CAPSULE && h.y != 0.0f) != CAPSULE) continue;
		const bool capsule = CAPSULE;
		const bool sphere = !CAPSULE && (shape == NH_SHAPE_SPHERE || shape == NH_SHAPE_CAPSULE);
		bool ok = (sphere || capsule || shape == NH_SHAPE_BOX) && nh_q_finite(c.x) && nh_q_finite(c.y) && nh_q_finite(c.z) && nh_q_finite(h.x) && !(h.x < 0.0f);
		if (!sphere) ok = ok && nh_q_finite(h.y) && !(h.y < 0.0f) && nh_q_finite(qr.x) && nh_q_finite(qr.y) && nh_q_finite(qr.z) && nh_q_finite(qr.s);
		if (!sphere && !capsule) ok = ok && nh_q_finite(h.z) && !(h.z < 0.0f);
		// the query's world AABB, padded by 2^-18 of its largest coordinate (only ever more generous than the exact test)
		const nh_f3 a = capsule ? nh_q_capsule_axis(qr, h.y) : nh_make3(0.0f, 0.0f, 0.0f);
		const nh_f3 e = sphere ? nh_make3(h.x, h.x, h.x) : capsule ? nh_q_capsule_extent(a, h.x) : nh_q_box_extent(qr, h);
		nh_f3 lo = c - e, hi = c + e;
		const float s = fmaxf(fmaxf(fmaxf(fabsf(lo.x), fabsf(lo.y)), fmaxf(fabsf(lo.z), fabsf(hi.x))), fmaxf(fabsf(hi.y), fabsf(hi.z))) * 3.814697265625e-06f;
		lo = nh_make3(lo.x - s, lo.y - s, lo.z - s); hi = nh_make3(hi.x + s, hi.y + s, hi.z + s);
		uint32_t k = 0u;
		nh_q_walk<FILTER>(nodes, rec, ok && n ? 0u : NH_Q_NONE, ignore, F, FILTER ? F.of(i) : 0u,
			[&](nh_f3 nlo, nh_f3 nhi, float&) { return nlo.x <= hi.x && lo.x <= nhi.x && nlo.y <= hi.y && lo.y <= nhi.y && nlo.z <= hi.z && lo.z <= nhi.z; },
			[&](uint32_t cc, const nh_QRec& r, float) {
				const nh_QShape col = nh_q_unpack(r);
				bool hit;
				if (capsule) hit = cc < nbox ? nh_q_overlap_capsule_box_a(c, a, h.x, col.p, col.q, col.h) : nh_q_overlap_capsule_sphere_a(c, a, h.x, col.p, col.h.x);
				else if (cc < nbox) hit = sphere ? nh_q_overlap_sphere_box(c, h.x, col.p, col.q, col.h) : nh_q_overlap_box_box(c, qr, h, col.p, col.q, col.h);
				else hit = sphere ? nh_q_overlap_sphere_sphere(c, h.x, col.p, col.h.x) : nh_q_overlap_sphere_box(col.p, col.h.x, c, qr, h);
				if (!hit) return false;
				if (LIST) {
					// (the count pass found exactly end - base: the segment is full once they are written, nothing else can follow)
					keys[base + k] = ((uint64_t)i << cbits) | cc;
					vals[base + k] = cc;
					if (base + k + 1u == end) return true;
				}
				++k;
				return false;
			});
		if (!LIST) offsets[i] = k;
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
		const float4* qp = reinterpret_cast<const float4*>(queries + i);
		const float4 q0 = qp[0], q1 = qp[1], q2 = qp[2];
		const nh_f3 c = nh_make3(q0.x, q0.y, q0.z), h = nh_make3(q2.x, q2.y, q2.z);
		const nh_quat qr = { q1.x, q1.y, q1.z, q1.w };
		const uint32_t shape = __float_as_uint(q0.w);
		const bool capsule = shape == NH_SHAPE_CAPSULE && h.y != 0.0f;
		const bool sphere = !capsule && (shape == NH_SHAPE_SPHERE || shape == NH_SHAPE_CAPSULE);
		const nh_QRec r = rec[cc];
		const nh_QShape s = nh_q_unpack(r);
		nh_QPen o;
		if (capsule) {
			const nh_f3 a = nh_q_capsule_axis(qr, h.y);
			o = cc < nbox ? nh_q_pen_capsule_box_a(c, a, h.x, s.p, s.q, s.h) : nh_q_pen_capsule_sphere_a(c, a, h.x, s.p, s.h.x);
		} else if (cc < nbox) o = sphere ? nh_q_pen_sphere_box(c, h.x, s.p, s.q, s.h) : nh_q_pen_box_box(c, qr, h, s.p, s.q, s.h);
		else o = sphere ? nh_q_pen_sphere_sphere(c, h.x, s.p, s.h.x) : nh_q_pen_box_sphere(c, qr, h, s.p, s.h.x);
		uint4* out = reinterpret_cast<uint4*>(hits + j);
		out[0] = make_uint4(__float_as_uint(o.n.x), __float_as_uint(o.n.y), __float_as_uint(o.n.z), __float_as_uint(o.depth));
		out[1] = nh_q_identity(cc, nbox, r);
	}
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
template <class Shape, bool LIST, bool FILTER>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(Shape::ALL_WAVES))) void k_q_castall(const float4* __restrict__ casts, uint32_t count, uint32_t* offsets,
                                                   const nh_QNode* __restrict__ nodes, const nh_QRec* __restrict__ rec, uint32_t n, uint32_t nbox,
                                                   nh_QCtl* ctl, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t cbits, uint32_t one_sort, nh_QFilter F) {
	if (!LIST && blockIdx.x == 0 && threadIdx.x == 0) { offsets[count] = 0u; ctl->ov_wrap = 0u; ctl->ov_written = 0u; }   // (k_q_overlap_fix sets both)
	const uint32_t written = LIST ? ctl->ov_written : 0u;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) {
		uint32_t base = 0u, end = 0u;
		if (LIST) {
			base = offsets[i]; end = offsets[i + 1u];
			if (!(base < end && end <= written)) continue;          // empty, or not in the written prefix
		}
		Shape k;
		k.read(casts + (size_t)i * Shape::WORDS);
		const bool ray = k.raylike();
		uint32_t hits = 0u;
		nh_q_walk<FILTER>(nodes, rec, k.ok && n ? 0u : NH_Q_NONE, k.ignore, F, FILTER ? F.of(i) : 0u,
			[&](nh_f3 lo, nh_f3 hi, float& t0) {
				// (a ray's node box also takes the predicates' own rounding, nh_q_all_pad; a sized shape's reach rule reads the entry of the box as the build stores it)
				if (ray) return nh_q_cast_node(lo, hi, k.o, k.inv, k.grow() + nh_q_all_pad(lo, hi, k.o), t0) && t0 <= k.max_t;
				return k.node(lo, hi, t0) && t0 <= k.max_t;
			},
			[&](uint32_t c, const nh_QRec& q, float t0) {
				const nh_QHit h = k.all(nh_q_unpack(q), c < nbox, t0);
				if (!h.hit) return false;
				if (LIST) {
					// (the count pass found exactly end - base: the segment is full once they are written, nothing else can follow)
					const uint32_t tb = nh_q_tbits(h.t);
					keys[base + hits] = one_sort ? ((uint64_t)i << (32u + cbits)) | ((uint64_t)tb << cbits) | c : ((uint64_t)i << cbits) | c;
					vals[base + hits] = one_sort ? c : tb;
					if (base + hits + 1u == end) return true;
				}
				++hits;
				return false;
			});
		if (!LIST) offsets[i] = hits;
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
		const nh_QShape s = nh_q_unpack(rec[c]);
		float t0 = 0.0f;
		k.entry(s, c < nbox, t0);                          // (entered: the walk listed it)
		const nh_QHit h = k.all(s, c < nbox, t0);
		nh_q_write_hit(hits + j, rec, nbox, true, c, h.t, h.n);
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
			[&](nh_f3 lo, nh_f3 hi, float& t0) {
				if (ray) return nh_q_cast_node(lo, hi, k.o, k.inv, k.grow() + nh_q_all_pad(lo, hi, k.o), t0) && t0 <= bd;
				return k.node(lo, hi, t0) && t0 <= bd;
			},
			[&](uint32_t c, const nh_QRec& q, float t0) {
				const nh_QHit h = k.all(nh_q_unpack(q), c < nbox, t0);
				if (!h.hit || !(h.t <= bd)) return false;
				if (nh_q_nearest_insert(list, stride, kk, &held, h.t, c, k.max_t) && held == kk) bd = list[(kk - 1u) * stride].key;
				return false;
			});
		nh_RayHit* out = hits + (size_t)i * kk;
		for (uint32_t j = 0u; j < held; ++j) {
			const uint32_t c = list[j * stride].c;
			const nh_QShape s = nh_q_unpack(rec[c]);
			float t0 = 0.0f;
			k.entry(s, c < nbox, t0);                          // (entered: the walk listed it)
			const nh_QHit h = k.all(s, c < nbox, t0);
			nh_q_write_hit(out + j, rec, nbox, true, c, h.t, h.n);
		}
		for (uint32_t j = held; j < kk; ++j) nh_q_write_hit(out + j, rec, nbox, k.ok, NH_Q_NONE, k.max_t, nh_make3(0.0f, 0.0f, 0.0f));
		if (counts) counts[i] = held;
	}
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
void nh_query_free(nh_context* ctx) {
	nh_QueryState* q = ctx->query;
	if (!q) return;
	void* bufs[] = { q->ctl, q->rec, q->keys_a, q->keys_b, q->idx_a, q->idx_b, q->hist, q->nodes, q->parent, q->rchild, q->last, q->right_at, q->arrive, q->top,
	                 q->ov_keys_a, q->ov_keys_b, q->ov_vals_a, q->ov_vals_b, q->layers, q->node_layers };
	for (void* b : bufs) if (b) hipFree(b);
	delete q;
	ctx->query = nullptr;
}

// (buffers by collider count; a growth waits for the stream first: the last build / cast may still read the old ones)
static int nh_query_reserve(nh_context* ctx, uint32_t C) {
	if (!ctx->query) ctx->query = new nh_QueryState();
	nh_QueryState* q = ctx->query;
	if (!q->ctl) {
		NH_HIP_CHECK(ctx, hipMalloc((void**)&q->ctl, sizeof(nh_QCtl)));
		NH_HIP_CHECK(ctx, hipMemsetAsync(q->ctl, 0, sizeof(nh_QCtl), ctx->stream));
		NH_HIP_CHECK(ctx, hipMemsetAsync(q->ctl->smin, 0xff, sizeof(q->ctl->smin), ctx->stream));
		NH_HIP_CHECK(ctx, hipMalloc((void**)&q->hist, sizeof(uint32_t) * (256u * NH_SORT_GRID + 512u)));
	}
	if (C <= q->capacity) return NH_OK;
	const uint32_t cap = C + C / 8u + 64u;
	NH_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	void* old[] = { q->rec, q->keys_a, q->keys_b, q->idx_a, q->idx_b, q->nodes, q->parent, q->rchild, q->last, q->right_at, q->arrive, q->top };
	for (void* b : old) if (b) hipFree(b);
	q->rec = nullptr; q->keys_a = q->keys_b = nullptr; q->idx_a = q->idx_b = nullptr; q->nodes = nullptr;
	q->parent = q->rchild = q->last = q->right_at = q->arrive = q->top = nullptr;
	q->capacity = 0; q->built = false; q->keys = nullptr; q->idx = nullptr;
	NH_HIP_CHECK(ctx, hipMalloc((void**)&q->rec, sizeof(nh_QRec) * (size_t)cap));
	NH_HIP_CHECK(ctx, hipMalloc((void**)&q->keys_a, sizeof(uint64_t) * (size_t)cap));
	NH_HIP_CHECK(ctx, hipMalloc((void**)&q->keys_b, sizeof(uint64_t) * (size_t)cap));
	NH_HIP_CHECK(ctx, hipMalloc((void**)&q->idx_a, sizeof(uint32_t) * (size_t)cap));
	NH_HIP_CHECK(ctx, hipMalloc((void**)&q->idx_b, sizeof(uint32_t) * (size_t)cap));
	NH_HIP_CHECK(ctx, hipMalloc((void**)&q->nodes, 2u * sizeof(nh_QNode) * (size_t)cap));
	NH_HIP_CHECK(ctx, hipMalloc((void**)&q->parent, 2u * sizeof(uint32_t) * (size_t)cap));
	NH_HIP_CHECK(ctx, hipMalloc((void**)&q->rchild, sizeof(uint32_t) * (size_t)cap));
	NH_HIP_CHECK(ctx, hipMalloc((void**)&q->last, sizeof(uint32_t) * (size_t)cap));
	NH_HIP_CHECK(ctx, hipMalloc((void**)&q->right_at, sizeof(uint32_t) * (size_t)cap));
	NH_HIP_CHECK(ctx, hipMalloc((void**)&q->arrive, sizeof(uint32_t) * (size_t)cap));
	// (a node has at most one entry child per side, and a tree of n leaves at most n entries: every entry is the root of a disjoint subtree)
	NH_HIP_CHECK(ctx, hipMalloc((void**)&q->top, sizeof(uint32_t) * (size_t)cap));
	q->capacity = cap;
	return NH_OK;
}

static int nh_query_args(const nh_BodyData* bodies, const nh_ColliderData* colliders, uint32_t* count) {
	const uint32_t nbox = colliders->boxes.count, nsph = colliders->spheres.count;
	const uint64_t C64 = (uint64_t)nbox + nsph;
	if (C64 >= NH_Q_MAX_COLLIDERS) return NH_ERR_INVALID;
	if (C64 && (!bodies->transforms && bodies->count)) return NH_ERR_INVALID;
	if (nbox && (!colliders->boxes.tags || !colliders->boxes.data || !colliders->boxes.transforms)) return NH_ERR_INVALID;
	if (nsph && (!colliders->spheres.tags || !colliders->spheres.data || !colliders->spheres.transforms)) return NH_ERR_INVALID;
	*count = (uint32_t)C64;
	return NH_OK;
}

static nh_QWorld nh_query_world(const nh_BodyData* bodies, const nh_ColliderData* colliders) {
	nh_QWorld W;
	W.body_xf = bodies->transforms; W.nbodies = bodies->count;
	W.box_xf = colliders->boxes.transforms; W.box_data = colliders->boxes.data; W.box_tags = colliders->boxes.tags; W.nbox = colliders->boxes.count;
	W.sph_xf = colliders->spheres.transforms; W.sph_data = colliders->spheres.data; W.sph_tags = colliders->spheres.tags; W.nsph = colliders->spheres.count;
	return W;
}

// The box pass over the tree of the last build: two launches, the second only where the tree has more than one run.
static void nh_query_boxes(nh_context* ctx, const nh_QWorld& W, uint32_t C) {
	nh_QueryState* q = ctx->query;
	NH_LAUNCH(ctx, "q_boxes_runs", k_q_boxes_runs, (C + NH_Q_RUN - 1u) / NH_Q_RUN, NH_Q_RUN, W, q->idx, q->parent, q->right_at, C, q->rec, q->nodes);
	if (C > NH_Q_RUN) NH_LAUNCH(ctx, "q_boxes_top", k_q_boxes_top, 1, NH_Q_TOP_BLOCK, q->top, q->ctl, q->nodes, q->parent, q->rchild, q->arrive);
}

// The layer pass over the tree of the last build (the comment above k_q_layers_runs): two launches, the second only where the tree has more than one run.
static void nh_query_layer_pass(nh_context* ctx) {
	nh_QueryState* q = ctx->query;
	const uint32_t C = q->n;
	if (!C) return;
	NH_LAUNCH(ctx, "q_layers_runs", k_q_layers_runs, (C + NH_Q_RUN - 1u) / NH_Q_RUN, NH_Q_RUN, q->layers, q->idx, q->parent, C, q->node_layers);
	if (C > NH_Q_RUN) NH_LAUNCH(ctx, "q_layers_top", k_q_layers_top, 1, NH_Q_TOP_BLOCK, q->top, q->ctl, q->nodes, q->parent, q->rchild, q->arrive, q->node_layers);
}

// What the walking kernels get of the context's filter; `on`: the call launches the FILTER = true instantiation.
static nh_QFilter nh_query_filter_of(const nh_QueryState* q, bool* on) {
	*on = q->filter_mode != NH_FILTER_OFF;
	nh_QFilter F;
	F.words = q->layers_set ? q->node_layers : nullptr;
	F.masks = q->filter_mode == NH_FILTER_PER_QUERY ? q->filter_masks : nullptr;
	F.mask = q->filter_mask;
	return F;
}

// Observer: no nh_flush_pending, no view export, no counter -- only launches on the stream and buffers of its own (header, "scene queries").
extern "C" int nh_query_build(nh_context* ctx, const nh_BodyData* bodies, const nh_ColliderData* colliders) {
	if (!ctx || !bodies || !colliders) return NH_ERR_INVALID;
	uint32_t C = 0;
	{ const int rc = nh_query_args(bodies, colliders, &C); if (rc) return rc; }
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	{ const int rc = nh_query_reserve(ctx, C); if (rc) return rc; }
	nh_QueryState* q = ctx->query;
	if (C) {
		const nh_QWorld W = nh_query_world(bodies, colliders);
		NH_LAUNCH(ctx, "q_xform", k_q_xform, nh_grid_for(C, 256, 4096), 256, W, q->rec, q->ctl);
		NH_LAUNCH(ctx, "q_keys", k_q_keys, nh_grid_for(C, 256, 4096), 256, q->rec, q->ctl, C, q->keys_a, q->idx_a);
		// 48-bit keys: six passes, the result back in the *_a buffers
		const int in_b = nh_sort_u64_u32(ctx, q->keys_a, q->keys_b, q->idx_a, q->idx_b, &q->ctl->count, q->hist, 0, 48);
		q->keys = in_b ? q->keys_b : q->keys_a;
		q->idx = in_b ? q->idx_b : q->idx_a;
		NH_LAUNCH(ctx, "q_tree", k_q_tree, nh_grid_for(C > 1u ? C - 1u : 1u, 256, 4096), 256, q->keys, C, q->nodes, q->parent, q->rchild, q->last, q->right_at, q->arrive,
		          q->top, q->ctl);
		if (C > 1u) NH_LAUNCH(ctx, "q_links", k_q_links, nh_grid_for(C - 1u, 256, 4096), 256, C, q->nodes, q->last, q->right_at);
		nh_query_boxes(ctx, W, C);
	}
	// (layers are by combined collider index: they outlive a build with the same two counts, whose tree needs the node words again)
	const bool same_world = q->built && q->n == C && q->nbox == colliders->boxes.count;
	q->built = true; q->n = C; q->nbox = colliders->boxes.count;
	if (q->layers_set && !same_world) q->layers_set = false;
	if (q->layers_set) nh_query_layer_pass(ctx);
	return NH_OK;
}

// Layer words of the colliders of the last build (header, "layer masks").  Observer like the build.
extern "C" int nh_query_set_layers(nh_context* ctx, const uint32_t* box_layers, const uint32_t* sphere_layers) {
	if (!ctx) return NH_ERR_INVALID;
	nh_QueryState* q = ctx->query;
	if (!q || !q->built) return NH_ERR_INVALID;
	if (((uintptr_t)box_layers | (uintptr_t)sphere_layers) & 3u) return NH_ERR_INVALID;
	if (!box_layers && !sphere_layers) { q->layers_set = false; return NH_OK; }
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	if (q->capacity > q->layer_capacity) {
		// (a growth waits for the stream first, as nh_query_reserve's does: a filtered call may still read the old words)
		NH_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
		if (q->layers) hipFree(q->layers);
		if (q->node_layers) hipFree(q->node_layers);
		q->layers = q->node_layers = nullptr;
		q->layer_capacity = 0; q->layers_set = false;
		NH_HIP_CHECK(ctx, hipMalloc((void**)&q->layers, sizeof(uint32_t) * (size_t)q->capacity));
		NH_HIP_CHECK(ctx, hipMalloc((void**)&q->node_layers, 2u * sizeof(uint32_t) * (size_t)q->capacity));
		q->layer_capacity = q->capacity;
	}
	const uint32_t nbox = q->nbox, nsph = q->n - q->nbox;
	if (nbox) {
		if (box_layers) NH_HIP_CHECK(ctx, hipMemcpyAsync(q->layers, box_layers, sizeof(uint32_t) * (size_t)nbox, hipMemcpyDeviceToDevice, ctx->stream));
		else NH_HIP_CHECK(ctx, hipMemsetAsync(q->layers, 0xff, sizeof(uint32_t) * (size_t)nbox, ctx->stream));
	}
	if (nsph) {
		if (sphere_layers) NH_HIP_CHECK(ctx, hipMemcpyAsync(q->layers + nbox, sphere_layers, sizeof(uint32_t) * (size_t)nsph, hipMemcpyDeviceToDevice, ctx->stream));
		else NH_HIP_CHECK(ctx, hipMemsetAsync(q->layers + nbox, 0xff, sizeof(uint32_t) * (size_t)nsph, ctx->stream));
	}
	q->layers_set = true;
	nh_query_layer_pass(ctx);
	return NH_OK;
}

// The filter every later query call reads (header, "layer masks").  Host state only: nothing is launched.
extern "C" int nh_query_filter(nh_context* ctx, uint32_t mode, uint32_t mask, const uint32_t* masks) {
	if (!ctx) return NH_ERR_INVALID;
	nh_QueryState* q = ctx->query;
	if (!q || !q->built) return NH_ERR_INVALID;
	if (mode != NH_FILTER_OFF && mode != NH_FILTER_UNIFORM && mode != NH_FILTER_PER_QUERY) return NH_ERR_INVALID;
	if (mode == NH_FILTER_PER_QUERY && (!masks || ((uintptr_t)masks & 3u))) return NH_ERR_INVALID;
	q->filter_mode = mode;
	q->filter_mask = mode == NH_FILTER_UNIFORM ? mask : 0u;
	q->filter_masks = mode == NH_FILTER_PER_QUERY ? masks : nullptr;
	return NH_OK;
}

// Diagnostic: whether layers are in force and the root's node word.  Waits for the stream.
extern "C" int nh_query_layer_info(nh_context* ctx, nh_QueryLayerInfo* out) {
	if (!ctx || !out) return NH_ERR_INVALID;
	nh_QueryState* q = ctx->query;
	if (!q || !q->built) return NH_ERR_INVALID;
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	uint32_t any = q->n ? 0xffffffffu : 0u;
	if (q->layers_set && q->n) NH_HIP_CHECK(ctx, hipMemcpyAsync(&any, q->node_layers, sizeof(any), hipMemcpyDeviceToHost, ctx->stream));
	NH_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	out->set = q->layers_set ? 1u : 0u;
	out->colliders = q->n;
	out->any_layers = any;
	out->reserved = 0u;
	return NH_OK;
}

// The tree of the last build with the boxes of the arrays given now (header: the contract).  Observer like the build; no allocation, no wait.
extern "C" int nh_query_refit(nh_context* ctx, const nh_BodyData* bodies, const nh_ColliderData* colliders) {
	if (!ctx || !bodies || !colliders) return NH_ERR_INVALID;
	nh_QueryState* q = ctx->query;
	if (!q || !q->built) return NH_ERR_INVALID;
	uint32_t C = 0;
	{ const int rc = nh_query_args(bodies, colliders, &C); if (rc) return rc; }
	// (the leaf order is by combined collider index: other counts are another world)
	if (colliders->boxes.count != q->nbox || C != q->n) return NH_ERR_INVALID;
	if (!C) return NH_OK;
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	nh_query_boxes(ctx, nh_query_world(bodies, colliders), C);
	return NH_OK;
}

// Diagnostics of the last build's tree (tools/refit_rates.py).  Waits for the stream.
extern "C" int nh_query_stats(nh_context* ctx, nh_QueryStats* out) {
	if (!ctx || !out) return NH_ERR_INVALID;
	nh_QueryState* q = ctx->query;
	if (!q || !q->built) return NH_ERR_INVALID;
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	nh_QCtl ctl;
	NH_HIP_CHECK(ctx, hipMemcpyAsync(&ctl, q->ctl, sizeof(ctl), hipMemcpyDeviceToHost, ctx->stream));
	NH_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	out->colliders = q->n;
	out->run_length = NH_Q_RUN;
	out->runs = (q->n + NH_Q_RUN - 1u) / NH_Q_RUN;
	out->top_nodes = q->n > NH_Q_RUN && ctl.top_n ? ctl.top_n - 1u : 0u;
	out->top_depth = q->n > NH_Q_RUN ? ctl.top_depth : 0u;
	return NH_OK;
}

// The four closest-hit casts: one record type and one kernel each, the same checks in the same order.
template <class Cast>
using nh_CastKernel = void (*)(const Cast*, uint32_t, nh_RayHit*, const nh_QNode*, const nh_QRec*, uint32_t, uint32_t, uint32_t, nh_QFilter);
template <class Cast>
static int nh_cast(nh_context* ctx, const char* label, nh_CastKernel<Cast> plain, nh_CastKernel<Cast> filtered, const Cast* casts, uint32_t count, nh_RayHit* hits,
                   uint32_t flags) {
	if (!ctx || !ctx->query || !ctx->query->built) return NH_ERR_INVALID;
	if (flags & ~(uint32_t)NH_RAY_ANY_HIT) return NH_ERR_INVALID;
	if (count == 0u) return NH_OK;
	if (!casts || !hits || (((uintptr_t)casts | (uintptr_t)hits) & 15u)) return NH_ERR_INVALID;    // (records are moved as 16-byte words)
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
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

extern "C" int nh_closest(nh_context* ctx, const nh_PointQuery* queries, uint32_t count, nh_PointHit* hits, uint32_t flags) {
	if (!ctx || !ctx->query || !ctx->query->built) return NH_ERR_INVALID;
	if (flags != 0u) return NH_ERR_INVALID;
	if (count == 0u) return NH_OK;
	if (!queries || !hits || (((uintptr_t)queries | (uintptr_t)hits) & 15u)) return NH_ERR_INVALID;    // (records are moved as 16-byte words)
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	nh_QueryState* q = ctx->query;
	bool on;
	const nh_QFilter F = nh_query_filter_of(q, &on);
	NH_LAUNCH(ctx, "q_closest", on ? k_q_closest<true> : k_q_closest<false>, nh_grid_for(count, 256, 1u << 20), 256, queries, count, hits, q->nodes, q->rec, q->keys,
	          q->ctl, q->n, q->nbox, F);
	return NH_OK;
}

// One launch with the lists' LDS sized by k (the table at k_q_closest_k); no allocation, no wait.
extern "C" int nh_closest_k(nh_context* ctx, const nh_PointQuery* queries, uint32_t count, uint32_t k, uint32_t* counts, nh_PointHit* hits, uint32_t flags) {
	if (!ctx || !ctx->query || !ctx->query->built) return NH_ERR_INVALID;
	if (flags != 0u || k == 0u || k > NH_CLOSEST_K_MAX || count >= (1u << 30)) return NH_ERR_INVALID;
	if (count == 0u) return NH_OK;
	if (!queries || !hits || (((uintptr_t)queries | (uintptr_t)hits) & 15u) || ((uintptr_t)counts & 3u)) return NH_ERR_INVALID;    // (records are moved as 16-byte words)
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	nh_QueryState* q = ctx->query;
	const uint32_t block = nh_q_nearest_block(k);
	if (ctx->timing) nh_timer_begin(ctx, "q_closest_k");
	bool on;
	const nh_QFilter F = nh_query_filter_of(q, &on);
	hipLaunchKernelGGL(on ? k_q_closest_k<true> : k_q_closest_k<false>, dim3(nh_grid_for(count, block, 1u << 20)), dim3(block), block * k * sizeof(nh_QNear), ctx->stream,
	                   queries, count, k, counts, hits, q->nodes, q->rec, q->keys, q->ctl, q->n, q->nbox, F);
	if (ctx->timing) nh_timer_end(ctx);
	return NH_OK;
}

// One launch, as nh_closest; no allocation, no wait.
extern "C" int nh_distance(nh_context* ctx, const nh_DistanceQuery* queries, uint32_t count, nh_PointHit* hits, uint32_t flags) {
	if (!ctx || !ctx->query || !ctx->query->built) return NH_ERR_INVALID;
	if (flags != 0u || count >= (1u << 30)) return NH_ERR_INVALID;
	if (count == 0u) return NH_OK;
	if (!queries || !hits || (((uintptr_t)queries | (uintptr_t)hits) & 15u)) return NH_ERR_INVALID;    // (records are moved as 16-byte words)
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
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
	void* old[] = { q->ov_keys_a, q->ov_keys_b, q->ov_vals_a, q->ov_vals_b };
	for (void* b : old) if (b) hipFree(b);
	q->ov_keys_a = q->ov_keys_b = nullptr; q->ov_vals_a = q->ov_vals_b = nullptr;
	q->ov_capacity = 0;
	NH_HIP_CHECK(ctx, hipMalloc((void**)&q->ov_keys_a, sizeof(uint64_t) * (size_t)cap));
	NH_HIP_CHECK(ctx, hipMalloc((void**)&q->ov_keys_b, sizeof(uint64_t) * (size_t)cap));
	NH_HIP_CHECK(ctx, hipMalloc((void**)&q->ov_vals_a, sizeof(uint32_t) * (size_t)cap));
	NH_HIP_CHECK(ctx, hipMalloc((void**)&q->ov_vals_b, sizeof(uint32_t) * (size_t)cap));
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

// The chain nh_overlap and nh_penetration share, from the argument checks to the sort: offsets are complete behind it, and for a list call (*list) the
// written prefix (ctl->ov_written records) lies sorted by (query, combined collider index) in the ov_*_b buffers (*in_b) or the ov_*_a ones.  Each
// entry point ends in its own gather.  `hits` is only checked here: records of either size are moved as 16-byte words.
static int nh_overlap_chain(nh_context* ctx, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets, const void* hits, uint32_t capacity,
                            uint32_t flags, bool* list_out, int* in_b, uint32_t* cbits_out) {
	*list_out = false;
	bool list = false;
	{ const int rc = nh_overlap_args(ctx, queries, count, offsets, hits, capacity, flags, &list); if (rc || count == 0u) return rc; }
	nh_QueryState* q = ctx->query;
	const uint32_t cbits = (uint32_t)nh_q_bits(q->n);
	*cbits_out = cbits;
	const uint32_t grid = nh_grid_for(count, 256, 1u << 20);
	bool on;
	const nh_QFilter F = nh_query_filter_of(q, &on);
	NH_LAUNCH(ctx, "q_overlap_count", (on ? k_q_overlap<false, false, true> : k_q_overlap<false, false, false>), grid, 256, queries, count, offsets, q->nodes, q->rec,
	          q->n, q->nbox, q->ctl, (uint64_t*)nullptr, (uint32_t*)nullptr, cbits, F);
	NH_LAUNCH(ctx, "q_overlap_count_capsule", (on ? k_q_overlap<false, true, true> : k_q_overlap<false, true, false>), grid, 256, queries, count, offsets, q->nodes, q->rec,
	          q->n, q->nbox, q->ctl, (uint64_t*)nullptr, (uint32_t*)nullptr, cbits, F);
	nh_overlap_offsets(ctx, offsets, count, capacity);
	if (!list) return NH_OK;
	NH_LAUNCH(ctx, "q_overlap_list", (on ? k_q_overlap<true, false, true> : k_q_overlap<true, false, false>), grid, 256, queries, count, offsets, q->nodes, q->rec,
	          q->n, q->nbox, q->ctl, q->ov_keys_a, q->ov_vals_a, cbits, F);
	NH_LAUNCH(ctx, "q_overlap_list_capsule", (on ? k_q_overlap<true, true, true> : k_q_overlap<true, true, false>), grid, 256, queries, count, offsets, q->nodes, q->rec,
	          q->n, q->nbox, q->ctl, q->ov_keys_a, q->ov_vals_a, cbits, F);
	const int bits = (((int)cbits + nh_q_bits(count)) + 7) / 8 * 8;
	*in_b = nh_sort_u64_u32(ctx, q->ov_keys_a, q->ov_keys_b, q->ov_vals_a, q->ov_vals_b, &q->ctl->ov_written, q->hist, 0, bits);
	*list_out = true;
	return NH_OK;
}

extern "C" int nh_overlap(nh_context* ctx, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets, nh_OverlapHit* hits, uint32_t capacity,
                          uint32_t flags) {
	bool list = false;
	int in_b = 0;
	uint32_t cbits = 0u;
	{ const int rc = nh_overlap_chain(ctx, queries, count, offsets, hits, capacity, flags, &list, &in_b, &cbits); if (rc || !list) return rc; }
	nh_QueryState* q = ctx->query;
	NH_LAUNCH(ctx, "q_overlap_gather", k_q_overlap_gather, nh_grid_for(capacity, 256, 4096), 256, in_b ? q->ov_vals_b : q->ov_vals_a, q->ctl, q->rec, q->n, q->nbox,
	          hits);
	return NH_OK;
}

// nh_overlap's chain with a gather that evaluates the pair function of each record (header: the same set, the same order, the same offsets).
extern "C" int nh_penetration(nh_context* ctx, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets, nh_PenetrationHit* hits, uint32_t capacity,
                              uint32_t flags) {
	bool list = false;
	int in_b = 0;
	uint32_t cbits = 0u;
	{ const int rc = nh_overlap_chain(ctx, queries, count, offsets, hits, capacity, flags, &list, &in_b, &cbits); if (rc || !list) return rc; }
	nh_QueryState* q = ctx->query;
	NH_LAUNCH(ctx, "q_penetration_gather", k_q_penetration_gather, nh_grid_for(capacity, 256, 1u << 20), 256, in_b ? q->ov_keys_b : q->ov_keys_a,
	          in_b ? q->ov_vals_b : q->ov_vals_a, q->ctl, q->rec, q->n, q->nbox, queries, count, cbits, hits);
	return NH_OK;
}

// The all-hits chain (the comment above k_q_castall): nh_overlap's argument rules, offsets and capacity contract, the casts' walk, the ordering by t.
// `label`: the timing labels' stem, q_<entry point without nh_>.
template <class Shape>
static int nh_castall(nh_context* ctx, const char* const label[3], const void* casts, uint32_t count, uint32_t* offsets, nh_RayHit* hits, uint32_t capacity,
                      uint32_t flags) {
	bool list = false;
	{ const int rc = nh_overlap_args(ctx, casts, count, offsets, hits, capacity, flags, &list); if (rc || count == 0u) return rc; }
	nh_QueryState* q = ctx->query;
	const float4* recs = static_cast<const float4*>(casts);
	const uint32_t cbits = (uint32_t)nh_q_bits(q->n);
	const int ibits = nh_q_bits(count);
	const bool one_sort = ibits + 32 + (int)cbits <= 64;
	const uint32_t grid = nh_grid_for(count, 256, 1u << 20);
	bool on;
	const nh_QFilter F = nh_query_filter_of(q, &on);
	NH_LAUNCH(ctx, label[0], (on ? k_q_castall<Shape, false, true> : k_q_castall<Shape, false, false>), grid, 256, recs, count, offsets, q->nodes, q->rec, q->n, q->nbox,
	          q->ctl, (uint64_t*)nullptr, (uint32_t*)nullptr, cbits, one_sort ? 1u : 0u, F);
	nh_overlap_offsets(ctx, offsets, count, capacity);
	if (!list) return NH_OK;
	NH_LAUNCH(ctx, label[1], (on ? k_q_castall<Shape, true, true> : k_q_castall<Shape, true, false>), grid, 256, recs, count, offsets, q->nodes, q->rec, q->n, q->nbox,
	          q->ctl, q->ov_keys_a, q->ov_vals_a, cbits, one_sort ? 1u : 0u, F);
	uint64_t* keys = q->ov_keys_a; uint64_t* keys_other = q->ov_keys_b;
	uint32_t* vals = q->ov_vals_a; uint32_t* vals_other = q->ov_vals_b;
	const uint32_t* m = &q->ctl->ov_written;
	if (nh_sort_u64_u32(ctx, keys, keys_other, vals, vals_other, m, q->hist, 0, one_sort ? (ibits + 32 + (int)cbits + 7) / 8 * 8 : ((int)cbits + 7) / 8 * 8)) {
		std::swap(keys, keys_other); std::swap(vals, vals_other);
	}
	if (!one_sort) {
		NH_LAUNCH(ctx, "q_castall_rekey", k_q_castall_rekey, nh_grid_for(capacity, 256, 4096), 256, keys, vals, q->ctl, cbits);
		if (nh_sort_u64_u32(ctx, keys, keys_other, vals, vals_other, m, q->hist, 0, (ibits + 32 + 7) / 8 * 8)) {
			std::swap(keys, keys_other); std::swap(vals, vals_other);
		}
	}
	NH_LAUNCH(ctx, label[2], (k_q_castall_gather<Shape>), nh_grid_for(capacity, 256, 1u << 20), 256, keys, vals, q->ctl, q->rec, q->n, q->nbox, recs, count,
	          one_sort ? 32u + cbits : 32u, hits);
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
	if (!ctx || !ctx->query || !ctx->query->built) return NH_ERR_INVALID;
	if (flags != 0u || k == 0u || k > NH_CAST_K_MAX || count >= (1u << 30)) return NH_ERR_INVALID;
	if (count == 0u) return NH_OK;
	if (!casts || !hits || (((uintptr_t)casts | (uintptr_t)hits) & 15u) || ((uintptr_t)counts & 3u)) return NH_ERR_INVALID;    // (records are moved as 16-byte words)
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	nh_QueryState* q = ctx->query;
	const uint32_t block = nh_q_nearest_block(k);
	if (ctx->timing) nh_timer_begin(ctx, label);
	bool on;
	const nh_QFilter F = nh_query_filter_of(q, &on);
	hipLaunchKernelGGL((on ? k_q_cast_k<Shape, true> : k_q_cast_k<Shape, false>), dim3(nh_grid_for(count, block, NH_Q_CAST_K_GRID)), dim3(block), block * k * sizeof(nh_QNear),
	                   ctx->stream, static_cast<const float4*>(casts), count, k, counts, hits, q->nodes, q->rec, q->n, q->nbox, F);
	if (ctx->timing) nh_timer_end(ctx);
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
