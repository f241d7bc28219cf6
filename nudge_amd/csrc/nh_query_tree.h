// nh_query_tree.h -- the scene-query tree as the library's own translation units see it (private, device side): the records, the nodes, the control words
// and the context's query state.  nh_query_build.hip makes and owns all of it; nh_query.hip walks it.  The per-item arithmetic is in nh_query.h, which the
// tests' host oracles share; nothing here is theirs.
// Node ids: internal nodes 0 .. n-2 (root 0), leaf j (j-th collider in key order) n-1+j; with one collider the root is that leaf.
#pragma once
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

// words of nh_overlap_bodies / nh_overlap_events (zeroed at the head of every call): the length of the input's written prefix (the sort reads it) and of
// each output's (entered or the bodies' list, left)
struct nh_QEventCtl { uint32_t in_written, out_written[2], pad; };

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
	uint32_t rg_capacity;        // nh_region's cursors, by region of the caller's count: where the list pass is in each region's segment
	uint32_t* rg_cursor;
	uint32_t ev_capacity;        // nh_overlap_bodies' / nh_overlap_events' flag and scan words, by record of the input capacities' sum (ev_scan: that + 2 words)
	uint32_t* ev_scan;
	struct nh_QEventCtl* ev_ctl; // their control words (allocated with the first scratch)
	uint32_t sw_capacity;        // nh_sweep's flag and scan words, by collider of the tree (sw_scan: that + 1 word and the scan's slack)
	uint32_t* sw_scan;
	uint32_t sw_body_capacity;   // nh_sweep_limit's words, by body: (bits of the least limiting t, the entry that applies it); only the words a list names are ever set
	uint2* sw_body;
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
