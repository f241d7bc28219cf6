// nh_query_build.hip -- the scene-query tree (nh_query_tree.h): nh_query_build (a linear BVH over every box and sphere collider, built from the current
// transforms), nh_query_refit (the same tree with the boxes of the current transforms), nh_query_set_layers (a word of layer bits per collider, and per node
// the OR of the words below it), nh_query_filter (the mask(s) every later query call walks under), the diagnostics, and the buffers all of them live in.
// include/nudge_hip.h, "scene queries" and "layer masks".  The queries that walk the tree are in nh_query.hip.
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
// Layer pass (behind nh_query_set_layers, and at the tail of a build while layers are set; never in a refit: the topology stands):
//   k_q_layers_runs / k_q_layers_top  the box pass's two climbs with a layer word in place of a box
#include "nh_query_tree.h"

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

// ---- the two climbs ---------------------------------------------------------------------------------------------------------------------------
// What a node holds of the leaves below it, bottom-up: a payload T with a merge() that does not depend on who arrives first, and a place P it lives in by
// node id.  The box pass carries the six floats of a box (fminf / fmaxf: a NaN leaf, a body that does not exist, drops out of its ancestors; the .w words
// of a node, child and escape links, stay as the build wrote them), the layer pass a layer word (OR).
struct nh_QBounds { float lo[3], hi[3]; };
__device__ __forceinline__ nh_QBounds nh_q_merge(nh_QBounds a, const nh_QBounds& b) {
	for (int k = 0; k < 3; ++k) { a.lo[k] = fminf(a.lo[k], b.lo[k]); a.hi[k] = fmaxf(a.hi[k], b.hi[k]); }
	return a;
}
__device__ __forceinline__ uint32_t nh_q_merge(uint32_t a, uint32_t b) { return a | b; }

struct nh_QNodeBoxes {
	nh_QNode* nodes;
	__device__ __forceinline__ nh_QBounds get(uint32_t id) const {
		const float4 a = nodes[id].a, b = nodes[id].b;
		return { { a.x, a.y, a.z }, { b.x, b.y, b.z } };
	}
	__device__ __forceinline__ void put(uint32_t id, const nh_QBounds& v) const {
		float* a = reinterpret_cast<float*>(&nodes[id].a);
		float* b = reinterpret_cast<float*>(&nodes[id].b);
		for (int k = 0; k < 3; ++k) { a[k] = v.lo[k]; b[k] = v.hi[k]; }
	}
};
struct nh_QNodeWords {
	uint32_t* words;
	__device__ __forceinline__ uint32_t get(uint32_t id) const { return words[id]; }
	__device__ __forceinline__ void put(uint32_t id, uint32_t v) const { words[id] = v; }
};

// Bottom phase.  Workgroup b owns leaves [b * NH_Q_RUN, (b + 1) * NH_Q_RUN) and the internal nodes whose range lies inside them (nh_query.h): LDS slot
// = node index - run start.  A slot holds the payloads of the node's two children, by side, and its arrival counter: a lane (leaf base + threadIdx.x, payload
// v, parent word pw; NH_Q_NONE for a lane without a leaf) puts its payload on its side, then counts itself in; the second to arrive reads the other side,
// merges and goes on with the parent, until the parent word says "top".  Every hand-off is inside the workgroup: LDS stores released and acquired at
// workgroup scope by the counter's atomic, no agent-scope fence, no global atomic.  The finished nodes leave through the slots after a barrier.
template <class T, class P>
__device__ __forceinline__ void nh_q_climb_run(const uint32_t* __restrict__ parent, uint32_t n, uint32_t pw, T v, P out) {
	__shared__ T child[NH_Q_RUN][2];
	__shared__ uint32_t arrived[NH_Q_RUN];
	__shared__ uint32_t up[NH_Q_RUN];            // parent words of the run's internal nodes
	const uint32_t base = blockIdx.x * NH_Q_RUN, s = threadIdx.x, j = base + s;
	arrived[s] = 0u;
	up[s] = j + 1u < n ? parent[j] : NH_Q_NONE;
	__syncthreads();
	while (!(pw & NH_Q_PARENT_TOP)) {
		const uint32_t slot = (pw & NH_Q_PARENT_ID) - base, side = (pw & NH_Q_PARENT_RIGHT) ? 1u : 0u;
		child[slot][side] = v;
		const uint32_t before = __hip_atomic_fetch_add(&arrived[slot], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
		if (before == 0u) break;
		v = nh_q_merge(v, child[slot][side ^ 1u]);
		pw = up[slot];
	}
	__syncthreads();
	if (arrived[s] == 2u) out.put(j, nh_q_merge(child[s][0], child[s][1]));
}

// Top phase: the nodes that cross a run boundary -- with B runs at most B - 2 have two crossing children, the rest are chains with one child finished
// below; few (nh_query_stats counts them) but deep.  The launch boundary has made the bottom phase's payloads visible.  ONE workgroup climbs from the entry
// list: a lane whose payload is in place counts itself in at the parent; the second to arrive merges its sibling's, writes the parent and goes on.
// All hand-offs are between waves of this one workgroup -- one CU, one L1, one L2 -- so the counter's atomic releases and acquires at WORKGROUP
// scope and nothing in the pass needs an agent-scope fence.  The second arriver leaves the counter at 0 for the next pass.  The counter's upper 24
// bits carry the first arriver's height, so that the root's lane knows the height of the top tree (the longest chain, for nh_query_stats: *depth,
// where the caller wants it).
#define NH_Q_TOP_BLOCK 1024
template <class P>
__device__ __forceinline__ void nh_q_climb_top(const uint32_t* __restrict__ top, uint32_t m, const nh_QNode* nodes, const uint32_t* __restrict__ parent,
                                               const uint32_t* __restrict__ rchild, uint32_t* arrive, P at, uint32_t* depth) {
	for (uint32_t e = threadIdx.x; e < m; e += NH_Q_TOP_BLOCK) {
		const uint32_t me = top[e];
		auto v = at.get(me);
		uint32_t height = 0u;
		uint32_t pw = parent[me];
		while (pw != NH_Q_NONE) {
			const uint32_t id = pw & NH_Q_PARENT_ID;
			const uint32_t before = __hip_atomic_fetch_add(&arrive[id], 1u | (height << 8), __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
			if ((before & 0xffu) == 0u) break;
			__hip_atomic_store(&arrive[id], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
			height = min(max(height, before >> 8) + 1u, 0xffffffu);
			const uint32_t other = (pw & NH_Q_PARENT_RIGHT) ? __float_as_uint(nodes[id].a.w) : rchild[id];
			v = nh_q_merge(v, at.get(other));
			at.put(id, v);
			pw = parent[id];
		}
		if (depth && pw == NH_Q_NONE) *depth = height;
	}
}

// ---- box pass -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NH_Q_RUN) void k_q_boxes_runs(nh_QWorld W, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ parent,
                                                           const uint32_t* __restrict__ right_at, uint32_t n, nh_QRec* __restrict__ rec, nh_QNode* __restrict__ nodes) {
	const uint32_t j = blockIdx.x * NH_Q_RUN + threadIdx.x;
	uint32_t pw = NH_Q_NONE;
	nh_QBounds box = { { 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f } };
	if (j < n) {
		const uint32_t c = idx[j];
		nh_QRec r;
		const nh_f3 e = nh_q_collider(W, c, r);
		rec[c] = r;
		const nh_f3 mn = nh_make3(r.a.x - e.x, r.a.y - e.y, r.a.z - e.z), mx = nh_make3(r.a.x + e.x, r.a.y + e.y, r.a.z + e.z);
		const float pad = nh_q_pad(mn, mx);      // (nh_query.h: the host's sweep rule rebuilds this box)
		box = { { mn.x - pad, mn.y - pad, mn.z - pad }, { mx.x + pad, mx.y + pad, mx.z + pad } };
		nh_QNode leaf;
		leaf.a = make_float4(box.lo[0], box.lo[1], box.lo[2], __uint_as_float(NH_Q_LEAF | c));
		leaf.b = make_float4(box.hi[0], box.hi[1], box.hi[2], __uint_as_float(j + 1u == n ? NH_Q_NONE : right_at[j]));
		nodes[n - 1u + j] = leaf;
		pw = parent[n - 1u + j];
	}
	nh_q_climb_run(parent, n, pw, box, nh_QNodeBoxes{ nodes });
}

__global__ __launch_bounds__(NH_Q_TOP_BLOCK) void k_q_boxes_top(const uint32_t* __restrict__ top, nh_QCtl* ctl, nh_QNode* nodes,
                                                                const uint32_t* __restrict__ parent, const uint32_t* __restrict__ rchild, uint32_t* arrive) {
	nh_q_climb_top(top, ctl->top_n, nodes, parent, rchild, arrive, nh_QNodeBoxes{ nodes }, &ctl->top_depth);
}

// ---- layer pass ------------------------------------------------------------------------------------------------------------------------------
// Per node, the OR of the layer words of the leaves below it.  It reads the sorted index, the parent words, rchild and the entry list of the last build, and
// the top phase the box pass's counters (0 between launches, left at 0; the height in them is not read).  Workgroup b gathers the words of its run's
// colliders into leaf order first.
__global__ __launch_bounds__(NH_Q_RUN) void k_q_layers_runs(const uint32_t* __restrict__ layers, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ parent,
                                                            uint32_t n, uint32_t* __restrict__ node_layers) {
	const uint32_t j = blockIdx.x * NH_Q_RUN + threadIdx.x;
	uint32_t pw = NH_Q_NONE, word = 0u;
	if (j < n) {
		word = layers[idx[j]];
		node_layers[n - 1u + j] = word;
		pw = parent[n - 1u + j];
	}
	nh_q_climb_run(parent, n, pw, word, nh_QNodeWords{ node_layers });
}

__global__ __launch_bounds__(NH_Q_TOP_BLOCK) void k_q_layers_top(const uint32_t* __restrict__ top, const nh_QCtl* __restrict__ ctl, const nh_QNode* __restrict__ nodes,
                                                                 const uint32_t* __restrict__ parent, const uint32_t* __restrict__ rchild, uint32_t* arrive,
                                                                 uint32_t* node_layers) {
	nh_q_climb_top(top, ctl->top_n, nodes, parent, rchild, arrive, nh_QNodeWords{ node_layers }, nullptr);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------
void nh_query_free(nh_context* ctx) {
	nh_QueryState* q = ctx->query;
	if (!q) return;
	void* bufs[] = { q->ctl, q->rec, q->keys_a, q->keys_b, q->idx_a, q->idx_b, q->hist, q->nodes, q->parent, q->rchild, q->last, q->right_at, q->arrive, q->top,
	                 q->ov_keys_a, q->ov_keys_b, q->ov_vals_a, q->ov_vals_b, q->layers, q->node_layers, q->rg_cursor, q->ev_scan, q->ev_ctl, q->sw_scan, q->sw_body };
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
	const size_t cap = C + C / 8u + 64u;
	NH_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
	q->capacity = 0; q->built = false; q->keys = nullptr; q->idx = nullptr;
	// (top: a node has at most one entry child per side, and a tree of n leaves at most n entries: every entry is the root of a disjoint subtree)
	{ int rc = nh_device_buffers(ctx, { { &q->rec, sizeof(nh_QRec) * cap }, { &q->keys_a, sizeof(uint64_t) * cap }, { &q->keys_b, sizeof(uint64_t) * cap },
	                                    { &q->idx_a, sizeof(uint32_t) * cap }, { &q->idx_b, sizeof(uint32_t) * cap }, { &q->nodes, 2u * sizeof(nh_QNode) * cap },
	                                    { &q->parent, 2u * sizeof(uint32_t) * cap }, { &q->rchild, sizeof(uint32_t) * cap }, { &q->last, sizeof(uint32_t) * cap },
	                                    { &q->right_at, sizeof(uint32_t) * cap }, { &q->arrive, sizeof(uint32_t) * cap }, { &q->top, sizeof(uint32_t) * cap } });
	  if (rc) return rc; }
	q->capacity = (uint32_t)cap;
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

// The layer pass over the tree of the last build: two launches, the second only where the tree has more than one run.
static void nh_query_layer_pass(nh_context* ctx) {
	nh_QueryState* q = ctx->query;
	const uint32_t C = q->n;
	if (!C) return;
	NH_LAUNCH(ctx, "q_layers_runs", k_q_layers_runs, (C + NH_Q_RUN - 1u) / NH_Q_RUN, NH_Q_RUN, q->layers, q->idx, q->parent, C, q->node_layers);
	if (C > NH_Q_RUN) NH_LAUNCH(ctx, "q_layers_top", k_q_layers_top, 1, NH_Q_TOP_BLOCK, q->top, q->ctl, q->nodes, q->parent, q->rchild, q->arrive, q->node_layers);
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
		q->layer_capacity = 0; q->layers_set = false;
		{ int rc = nh_device_buffers(ctx, { { &q->layers, sizeof(uint32_t) * (size_t)q->capacity }, { &q->node_layers, 2u * sizeof(uint32_t) * (size_t)q->capacity } });
		  if (rc) return rc; }
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
