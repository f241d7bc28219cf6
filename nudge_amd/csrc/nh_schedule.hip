// nh_schedule.hip -- the start of the solve order: nh_setup_contact_constraints and the kernels it launches itself -- the one-lane-per-body adjacency of the
// common case (k_adj_simple) and, in exact-order mode, the replay of the reference's batch scheduler (nudge.cpp:4206-4339) -- and the replay of a still step that
// owes that adjacency kernel (nh_still_abandon).  What the setup defers until the counters are on the host (general adjacency, classes, colours, levels) is
// launched by finish_setup beside the solvers it chooses between, and lives with them in nh_solve.hip.
#include "nh_internal.h"
#include "nh_solver.h"

// One lane per body.  A body that sits in exactly ONE collider pair, with the static world, and has <= 8 contacts -- the box on the
// ground -- needs no CSR build: its contacts are first .. first+d-1 (a pair's contacts are adjacent in tag order), recorded here in slot
// order as ONE word pair the solver reads next to the body state: simple[x] = (first contact, count | 3-bit offsets in slot order << 4 |
// body-is-"a" << 28).  Degrees come straight from nh_collide's counters: no scan, no adjacency array on this path (k_adj_from_simple
// writes the CSR form on demand).  Everything else is left PENDING for the general k_adj_fill / k_adj_sort, which do not even start
// when nothing is pending.
#define NH_FIRST_IS_A 0x80000000u        // in first_contact[]: the body plays "a" in its last pair (k_gather_contacts)
__global__ __launch_bounds__(256) void k_adj_simple(nh_DevState* __restrict__ st, uint32_t nbodies, uint32_t* __restrict__ deg, const unsigned long long* __restrict__ pair_counter,
                                                    const uint32_t* __restrict__ first_contact, const uint32_t* __restrict__ slot_key,
                                                    uint8_t* __restrict__ body_class, const nh_BodyProperties* __restrict__ props, nh_BodyMomentum* __restrict__ momentum,
                                                    uint2* __restrict__ simple, uint32_t* __restrict__ body_rec, uint32_t* __restrict__ body_pos, const uint32_t* __restrict__ sorted_idx) {
	// body_rec / body_pos (nh_internal.h, contact storage by slot): for a body of the one-pair class the record its contacts come from (| role) and that record's
	// place in the tag order -- what a still step's solver lane starts from; NH_BODY_REC_NONE for a body without contacts
	bool other = false, unstable = false;
	for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < nbodies; x += gridDim.x * blockDim.x) {
		if (x == 0) {
			body_class[0] = 0;
			momentum[0].unused0 = props[0].mass_inverse;             // the reference stashes mass_inverse in unused0 of EVERY body (nudge.cpp:4198)
			const nh_BodyMomentum m0 = momentum[0];
			const nh_BodyProperties p0 = props[0];
			st->static_inert = nh_is_inert(m0.velocity, m0.angular_velocity, p0.inertia_inverse, p0.mass_inverse) ? 1u : 0u;
			deg[0] = 0u;
			continue;
		}
		const unsigned long long pc = pair_counter[x];
		const uint32_t d = (uint32_t)pc;
		deg[x] = d;                                 // (the degrees as an array of their own: what the CSR scan reads, ensure_csr)
		uint32_t cls = NH_CLS_NONE;
		if (d) {
			const uint32_t inf = (uint32_t)(pc >> 32);
			if ((inf & 0xFFFFu) == 1u && (inf >> 16) == 0u && d <= 8u) {
				const uint32_t fc = first_contact[x];
				const uint32_t f = fc & ~NH_FIRST_IS_A;
				// contacts f .. f+d-1 in slot order (insertion sort in registers: a 4-entry network for the usual box on the ground, 8 otherwise)
				auto emit = [&](auto tag) {
					constexpr int W = decltype(tag)::value;
					uint32_t c[W], k[W];
#pragma unroll
					for (int q = 0; q < W; ++q) { c[q] = (uint32_t)q < d ? f + q : 0xFFFFFFFFu; k[q] = (uint32_t)q < d ? slot_key_of(c[q], slot_key) : 0xFFFFFFFFu; }
#pragma unroll
					for (int q = 1; q < W; ++q) {
#pragma unroll
						for (int j = q; j > 0; --j) {
							bool sw = (k[j] < k[j - 1]) || (k[j] == k[j - 1] && c[j] < c[j - 1]);
							uint32_t tc = sw ? c[j - 1] : c[j], tk = sw ? k[j - 1] : k[j];
							c[j - 1] = sw ? c[j] : c[j - 1]; k[j - 1] = sw ? k[j] : k[j - 1];
							c[j] = tc; k[j] = tk;
						}
					}
					uint32_t perm = 0;
#pragma unroll
					for (int q = 0; q < W; ++q) if ((uint32_t)q < d) perm |= (c[q] - f) << (3 * q);
					simple[x] = make_uint2(f, d | (perm << 4) | ((fc & NH_FIRST_IS_A) ? (1u << 28) : 0u));
					if (body_rec) {
						const uint32_t pos = first_contact[x + NH_DEG_STRIDE(nbodies)];
						body_pos[x] = pos;
						body_rec[x] = (sorted_idx ? sorted_idx[pos] : NH_BODY_REC_NONE) | ((fc & NH_FIRST_IS_A) ? NH_BODY_REC_IS_A : 0u);
					}
				};
				if (d <= 4u) emit(std::integral_constant<int, 4>()); else emit(std::integral_constant<int, 8>());
				cls = d <= 4u ? NH_CLS_STATIC4 : NH_CLS_STATIC8;
				if (cls == NH_CLS_STATIC8) st->has_static8 = 1;
			} else if (!slot_key && (inf >> 16) != 0u) {
				// default (colour) order and a dynamic partner: a general body, settled here -- its adjacency list is filled like a pending body's
				// (k_adj_fill) but needs neither the per-body sort by slot key nor the predecessor links of the exact order (k_adj_sort walks and
				// sorts every list it classifies: 0.5 ms in a pit of 4 M spheres that are ALL of this kind)
				cls = NH_CLS_GENERAL;
				st->has_pending = 1;
				momentum[x].unused0 = props[x].mass_inverse;         // (nudge.cpp:4198: the level-scheduled sweeps read it from there)
			} else {
				cls = NH_CLS_PENDING;
				st->has_pending = 1;
			}
		} else {
			momentum[x].unused0 = props[x].mass_inverse;
			if (body_rec) { body_rec[x] = NH_BODY_REC_NONE; body_pos[x] = 0u; }
		}
		body_class[x] = (uint8_t)cls;
		other |= cls != NH_CLS_STATIC4;
		unstable |= cls != NH_CLS_STATIC4 && cls != NH_CLS_NONE;
	}
	if (__builtin_amdgcn_ballot_w64(unstable) != 0 && nh_lane() == 0) st->has_unstable = 1u;
	// (one plain store per wave that has such a body: no counting)
	if (__builtin_amdgcn_ballot_w64(other) != 0 && nh_lane() == 0) st->has_other = 1u;
}

// ---- exact replay of the reference's greedy batch scheduler (nudge.cpp:4206-4339), one wave -------------------
#define GR_BUCKETS 16
#define GR_OPEN 64          // open (vacant) batches kept per bucket in LDS
// Exact-order mode, common case first.  When the scheduler below never meets a lane conflict, contact i ends up in batch
// (i / 128) * 16 + i % 16 (its bucket's batch completes with every eighth contact of the bucket, batches are emitted in that order,
// leftovers bucket by bucket).  The first conflict the scheduler can meet is two contacts of ONE such batch sharing a dynamic body, so if no
// batch of the closed form holds one, the closed form IS the schedule: checked here with one lane per batch; only otherwise the
// sequential replay runs (it is a single wave walking all contacts: milliseconds for tens of thousands).
__global__ __launch_bounds__(256) void k_order_check(nh_DevState* __restrict__ st, const nh_BodyPair* __restrict__ bodies, uint32_t* __restrict__ slot_key, uint32_t seq) {
	const uint32_t n = st->contacts;
	const uint32_t nbatch = ((n + 127u) / 128u) * 16u;
	for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < nbatch; t += gridDim.x * blockDim.x) {
		const uint32_t first = (t >> 4) * 128u + (t & 15u);
		uint32_t ca[8], cb[8];
		bool conflict = false;
#pragma unroll
		for (int k = 0; k < 8; ++k) {
			const uint32_t i = first + 16u * k;
			ca[k] = NH_NONE; cb[k] = NH_NONE;
			if (i < n) {
				const nh_BodyPair bp = bodies[i];
				ca[k] = bp.a ? bp.a : bp.b; cb[k] = bp.b ? bp.b : bp.a;      // dependencies on body 0 do not count (nudge.cpp:4238-4240)
				slot_key[i] = t;
#pragma unroll
				for (int j = 0; j < k; ++j) conflict |= ca[j] == ca[k] || cb[j] == ca[k] || ca[j] == cb[k] || cb[j] == cb[k];
			}
		}
		if (conflict) st->order_conflict = seq;
	}
}

// Open batches beyond the GR_OPEN kept in LDS spill to global memory (`spill_ab` / `spill_idx`: GR_BUCKETS x spill_cap x 8 entries from the
// arena): a dynamic hub body with thousands of contacts (a tray of boxes) makes every contact of a bucket conflict, so no batch completes
// and the open list grows with the contact count -- the reference sizes these arrays by contacts.count (nudge.cpp:4222-4223).
struct gr_store {
	uint2 (*lds_ab)[GR_OPEN + 1][8];
	uint32_t (*lds_idx)[GR_OPEN + 1][8];
	uint2* spill_ab; uint32_t* spill_idx; uint32_t spill_cap;
	__device__ __forceinline__ size_t at(uint32_t b, uint32_t j, uint32_t l) const { return ((size_t)b * spill_cap + (j - (GR_OPEN + 1u))) * 8u + l; }
	__device__ __forceinline__ uint2 ab(uint32_t b, uint32_t j, uint32_t l) const {
		if (j <= GR_OPEN) return lds_ab[b][j][l];
		const unsigned long long v = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(spill_ab + at(b, j, l)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
	}
	__device__ __forceinline__ void set_ab(uint32_t b, uint32_t j, uint32_t l, uint2 v) const {
		if (j <= GR_OPEN) lds_ab[b][j][l] = v;
		else __hip_atomic_store(reinterpret_cast<unsigned long long*>(spill_ab + at(b, j, l)), (unsigned long long)v.x | ((unsigned long long)v.y << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	__device__ __forceinline__ uint32_t idx(uint32_t b, uint32_t j, uint32_t l) const {
		return j <= GR_OPEN ? lds_idx[b][j][l] : __hip_atomic_load(spill_idx + at(b, j, l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	__device__ __forceinline__ void set_idx(uint32_t b, uint32_t j, uint32_t l, uint32_t v) const {
		if (j <= GR_OPEN) lds_idx[b][j][l] = v; else __hip_atomic_store(spill_idx + at(b, j, l), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
};

__global__ __launch_bounds__(64) void k_greedy_replay(nh_DevState* __restrict__ st, const nh_BodyPair* __restrict__ bodies, uint32_t* __restrict__ slot_key, uint32_t seq,
                                                      uint2* __restrict__ spill_ab, uint32_t* __restrict__ spill_idx, uint32_t spill_cap) {
	if (st->order_conflict != seq) return;          // k_order_check: the closed form it wrote is the schedule
	__shared__ uint2 pair_ab[GR_BUCKETS][GR_OPEN + 1][8];
	__shared__ uint32_t slot_idx[GR_BUCKETS][GR_OPEN + 1][8];
	__shared__ uint32_t vacancy[GR_BUCKETS];
	__shared__ uint32_t emitted;
	const gr_store S = { pair_ab, slot_idx, spill_ab, spill_idx, spill_cap };
	const uint32_t max_open = GR_OPEN + spill_cap;      // largest legal index of the all-invalid padding entry
	const uint32_t lane = threadIdx.x, sub = lane >> 3, ln = lane & 7;
	const uint32_t n = st->contacts;
	if (lane < GR_BUCKETS) { vacancy[lane] = 0; }
	if (lane == 0) emitted = 0;
	for (uint32_t k = lane; k < GR_BUCKETS * 8; k += 64) pair_ab[k >> 3][0][k & 7] = make_uint2(NH_NONE, NH_NONE);
	__syncthreads();
	for (uint32_t i = 0; i < n; ++i) {
		nh_BodyPair bp = bodies[i];
		uint32_t bucket = i % GR_BUCKETS;
		uint32_t ca = bp.a ? bp.a : bp.b, cb = bp.b ? bp.b : bp.a;     // ignore dependencies on body 0
		uint32_t vac = vacancy[bucket];
		// first open batch (or the all-invalid padding entry at index vac) without a conflicting lane
		uint32_t j = NH_NONE;
		for (uint32_t base = 0; j == NH_NONE; base += 8) {
			uint32_t jb = base + sub;
			bool in_range = jb <= vac;
			uint2 ab = in_range ? S.ab(bucket, jb, ln) : make_uint2(NH_NONE, NH_NONE);
			bool conflict = in_range && (ab.x == ca || ab.y == ca || ab.x == cb || ab.y == cb);
			unsigned long long bal = __ballot(conflict);
			unsigned long long rng = __ballot(in_range);
			for (uint32_t s = 0; s < 8; ++s) {
				bool ok = ((rng >> (s * 8)) & 1ull) && (((bal >> (s * 8)) & 0xffull) == 0ull);
				if (ok) { j = base + s; break; }
			}
		}
		// first free lane of that batch
		uint2 mine = S.ab(bucket, j, ln);
		unsigned long long freeb = __ballot(sub == 0 && mine.x == NH_NONE && mine.y == NH_NONE);
		uint32_t free_lane = (uint32_t)__ffsll((long long)(freeb & 0xffull)) - 1u;
		__syncthreads();
		if (lane == 0) {
			S.set_idx(bucket, j, free_lane, i);
			S.set_ab(bucket, j, free_lane, make_uint2(ca, cb));
		}
		__syncthreads();
		bool changed = false;
		if (j == vac) {
			vac = vac + 1;
			changed = true;
			if (vac > max_open) { if (lane == 0) st->error = NH_ERR_SCHEDULER_CAPACITY; return; }
		} else if (free_lane == 7) {
			// batch complete: emit it, move the last open batch into its place
			uint32_t e = emitted;
			if (lane < 8) slot_key[S.idx(bucket, j, lane)] = e;
			vac = vac - 1;
			__syncthreads();
			if (lane < 8) {
				S.set_ab(bucket, j, lane, S.ab(bucket, vac, lane));
				S.set_idx(bucket, j, lane, S.idx(bucket, vac, lane));
			}
			if (lane == 0) emitted = e + 1;
			changed = true;
		}
		__syncthreads();
		if (changed) {
			if (lane == 0) vacancy[bucket] = vac;
			if (lane < 8) S.set_ab(bucket, vac, lane, make_uint2(NH_NONE, NH_NONE));
		}
		__syncthreads();
	}
	// leftovers, bucket by bucket (nudge.cpp:4316-4337)
	uint32_t e = emitted;
	for (uint32_t b = 0; b < GR_BUCKETS; ++b) {
		uint32_t vac = vacancy[b];
		for (uint32_t j = 0; j < vac; ++j) {
			if (lane < 8) {
				uint2 ab = S.ab(b, j, lane);
				if (!(ab.x == NH_NONE && ab.y == NH_NONE)) slot_key[S.idx(b, j, lane)] = e;
			}
			++e;
		}
	}
}

static nh_ContactConstraintData* new_constraint_data(nh_context* ctx) {
	if (ctx->constraint_ring.empty()) { ctx->impulse_ring.resize(64, nullptr); ctx->constraint_ring.resize(64, nullptr); }
	uint32_t k = ctx->ring_pos % 64;
	if (!ctx->constraint_ring[k]) ctx->constraint_ring[k] = new nh_ContactConstraintData();
	return ctx->constraint_ring[k];
}

extern "C" int nh_setup_contact_constraints(nh_context* ctx, const nh_ActiveBodies* active_bodies, const nh_ContactData* contacts,
                                            const nh_BodyData* bodies, nh_ContactImpulseData* imp, nh_Arena* memory, nh_ContactConstraintData** out) {
	if (!ctx || !contacts || !bodies || !imp || !memory || !out) return NH_ERR_INVALID;
	{
		const nh_StillStep& ss = ctx->still;
		const bool in_sequence = ss.active && !ss.resolved && !ctx->pending && contacts->data == ss.lay_contacts.data && contacts->bodies == ss.lay_contacts.bodies &&
		                         bodies->momentum == ss.bodies.momentum && bodies->transforms == ss.bodies.transforms && bodies->count == ss.bodies.count && imp->ctx == ctx && !imp->consumed;
		int rc = nh_flush_pending(ctx, true, in_sequence); if (rc) return rc;
	}
	(void)active_bodies;
	nh_DevState* st = ctx->d_state;
	const uint32_t kcap = contacts->capacity;
	const uint32_t B = bodies->count;
	int err = NH_OK;
	nh_ContactConstraintData* d = new_constraint_data(ctx);
	d->rows = nh_arena_array<float>(memory, (size_t)kcap * 40, &err);
	d->states = nh_arena_array<float>(memory, (size_t)kcap * 4, &err);
	if (!ctx->deg || ctx->deg_capacity < NH_DEG_WORDS(B)) return NH_ERR_INVALID;      // nh_collide of this step sized and filled it
	// one setup per collide: the fill cursors and the contact layout below belong to the last nh_collide (header note 8)
	if (ctx->setup_seq == ctx->collide_seq) return NH_ERR_STALE_SETUP;
	if ((ctx->flags & NH_FLAG_SYNC_COUNTS) && contacts->count != ctx->h_state->contacts) return NH_ERR_STALE_SETUP;
	ctx->setup_seq = ctx->collide_seq;
	d->body_off = nh_arena_array<uint32_t>(memory, (size_t)B + 2u, &err);           // CSR offsets (scan of the degrees nh_collide counted)
	d->adj = nh_arena_array<uint32_t>(memory, (size_t)kcap * 2, &err);
	if (!ctx->lay_class || ctx->lay_body_capacity < B) return NH_ERR_INVALID;        // (sized by this step's nh_collide)
	d->body_class = ctx->lay_class;          // library-owned: a still step reads what the last full step's k_adj_simple left here
	d->simple = ctx->lay_simple;
	d->level_order = nh_arena_array<uint32_t>(memory, kcap, &err);
	d->gpair = nh_arena_array<uint2>(memory, kcap, &err);
	d->gstates = nh_arena_array<float4>(memory, kcap, &err);
	uint32_t* cursor = ctx->deg + NH_DEG_STRIDE(B);                                   // fill cursors (zeroed by nh_collide)
	uint32_t* pred_a = nh_arena_array<uint32_t>(memory, kcap, &err);
	uint32_t* pred_b = nh_arena_array<uint32_t>(memory, kcap, &err);
	uint32_t* level = nh_arena_array<uint32_t>(memory, kcap, &err);
	uint32_t* general_list = nh_arena_array<uint32_t>(memory, kcap, &err);
	uint32_t* slot_key = (ctx->flags & NH_FLAG_EXACT_ORDER) ? nh_arena_array<uint32_t>(memory, kcap, &err) : nullptr;
	uint32_t* tent = (ctx->flags & NH_FLAG_EXACT_ORDER) ? nullptr : nh_arena_array<uint32_t>(memory, kcap, &err);      // colouring: this round's picks
	// exact order: spill space of the scheduler replay's open batches (k_greedy_replay), at most 8192 per bucket = 12.6 MB
	const uint32_t spill_cap = slot_key ? (kcap / GR_BUCKETS + 1u < 8192u ? kcap / GR_BUCKETS + 1u : 8192u) : 0u;
	uint2* spill_ab = slot_key ? nh_arena_array<uint2>(memory, (size_t)GR_BUCKETS * spill_cap * 8u, &err) : nullptr;
	uint32_t* spill_idx = slot_key ? nh_arena_array<uint32_t>(memory, (size_t)GR_BUCKETS * spill_cap * 8u, &err) : nullptr;
	uint32_t* level_hist = nh_arena_array<uint32_t>(memory, 2 * (NH_MAX_LEVELS + 2), &err);       // [0, L+2): histogram -> offsets; [L+2, 2L+4): class has a full row
	uint32_t* level_cursor = nh_arena_array<uint32_t>(memory, NH_MAX_LEVELS + 2, &err);
	uint32_t* tmp = nh_arena_array<uint32_t>(memory, 2 * NH_SORT_GRID + 64, &err);
	if (err) return err;
	d->contact_capacity = kcap; d->body_count = B; d->bodies = contacts->bodies;
	d->contact_data = contacts->data; d->impulses = imp->data; d->general_list = general_list;
	d->levels = 0; d->general_contacts = 0;
	d->blk.active = false; d->blk.warm_pending = false; d->blk.local = false;

	// (degrees were counted by nh_collide while it laid the contacts out; their scan into CSR offsets waits until somebody needs it: ensure_csr)
	d->csr_ready = false;
	if (slot_key) {
		const uint32_t seq = ++ctx->order_seq ? ctx->order_seq : ++ctx->order_seq;       // never 0: tells this call's verdict from an older one
		NH_LAUNCH(ctx, "order_check", k_order_check, nh_grid_for(kcap / 8u + 16u, 256, 1024), 256, st, contacts->bodies, slot_key, seq);
		NH_LAUNCH(ctx, "greedy_replay", k_greedy_replay, 1, 64, st, contacts->bodies, slot_key, seq, spill_ab, spill_idx, spill_cap);
	}
	if (ctx->still.active && !ctx->still.resolved) ctx->still.setup_d = d;      // still step: classes and records are last step's (nh_still_abandon launches the kernel if it comes to that)
	else
	NH_LAUNCH(ctx, "adjacency_simple", k_adj_simple, nh_grid_for(B, 256, 4096), 256, st, B, ctx->deg, reinterpret_cast<const unsigned long long*>(ctx->deg + 2u * NH_DEG_STRIDE(B)), ctx->deg + 4u * NH_DEG_STRIDE(B), slot_key,
	          d->body_class, bodies->properties, bodies->momentum, d->simple, ctx->body_rec, ctx->body_pos, ctx->sort_seeded ? ctx->sort_sorted_idx : (const uint32_t*)nullptr);
	if (ctx->hint_capacity < B) {
		// library-owned, persistent across steps: per body, where its contacts started in the previous step's list (warm-start hint)
		ctx->hint_capacity = 0;
		{ int rc = nh_device_buffers(ctx, { { &ctx->hint, sizeof(uint32_t) * (size_t)B } }); if (rc) return rc; }
		NH_HIP_CHECK(ctx, hipMemsetAsync(ctx->hint, 0xFF, sizeof(uint32_t) * (size_t)B, ctx->stream));
		ctx->hint_capacity = B;
	}
	// No host round trip here.  The one-body path (lookup + rows + warm start) runs fused with the first sweeps, and everything that
	// needs the device counters is finished behind it (finish_setup), by nh_apply_impulses or by the next call that observes
	// momentum / impulses / counters (nh_flush_pending).
	d->cont.contacts = *contacts;
	d->cont.cursor = cursor; d->cont.pred_a = pred_a; d->cont.pred_b = pred_b; d->cont.level = level; d->cont.slot_key = slot_key;
	d->cont.level_hist = level_hist; d->cont.level_cursor = level_cursor; d->cont.tmp = tmp; d->cont.tent = tent;
	d->has_static8 = d->has_staticN = d->has_late = false; d->static_inert = false; d->general_lists = true;
	d->finish_pending = true;
	d->setup_pending = true; d->imp = imp; d->bodies_at_setup = *bodies;
	imp->consumed = true;
	ctx->pending = d;
	*out = d;
	return NH_OK;
}

// A still step that has not been confirmed, met by anything but the next call of the sample's order (or failed on the device): the step is launched again in full.
int nh_still_abandon(nh_context* ctx) {
	nh_StillStep& ss = ctx->still;
	if (!ss.active || ss.resolved || ss.replaying) return NH_OK;
	nh_ContactConstraintData* d = ss.setup_d;
	ss.setup_d = nullptr;
	int rc = nh_still_undo_drops(ctx);                    // (what this step's narrowphase dropped from the slot cache in sleepers form comes back first)
	if (rc) return rc;
	rc = nh_still_export_cache(ctx);                      // (the slot cache holds the last confirmed step's impulses: the full solver reads the caller's arrays)
	if (rc) return rc;
	ss.contacts_stale = false;                         // (the replay lays the dense list out itself)
	rc = nh_still_collide_again(ctx);
	if (rc) return rc;
	if (d) {
		// the adjacency kernel the still setup left out (default order only: still steps are not launched in exact-order mode)
		const uint32_t B = d->body_count;
		NH_LAUNCH(ctx, "adjacency_simple", k_adj_simple, nh_grid_for(B, 256, 4096), 256, ctx->d_state, B, ctx->deg, reinterpret_cast<const unsigned long long*>(ctx->deg + 2u * NH_DEG_STRIDE(B)),
		          ctx->deg + 4u * NH_DEG_STRIDE(B), (const uint32_t*)nullptr, d->body_class, d->bodies_at_setup.properties, d->bodies_at_setup.momentum, d->simple,
		          ctx->body_rec, ctx->body_pos, ctx->sort_seeded ? ctx->sort_sorted_idx : (const uint32_t*)nullptr);
	}
	return NH_OK;
}
