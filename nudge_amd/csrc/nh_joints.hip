// nh_joints.hip -- joints (include/nudge_hip.h, "joints"): ball, distance and hinge joints between the calls of the call-by-call ABI.  The per-item
// logic is nh_joint.h's, which the host oracle compiles as well; here are the schedule -- the caller's list order turned into dependency levels per BIN -- and
// the two kernels that replay that order in parallel, one workgroup per bin, a workgroup barrier between two levels.
//   k_j_init          one lane per joint and per body: levels 0, order the identity, the owner words NH_NONE; its first lane clears the four status words
//   k_j_offsets       one lane per cut point: the offsets' rules and the assembly size, OR-ed into status[0]
//   k_j_owner<0>      one lane per joint: counts the valid ones; a min over bin numbers into the owner words of its dynamic bodies
//   k_j_owner<1>      ... compares: a body whose owner is another bin raises NH_JOINT_ERR_SHARED_BODY
//   k_j_levels        one workgroup per bin, all in LDS: the span's body pairs, each joint's predecessors by a backward scan, levels by relaxation rounds between
//                     barriers until nothing changes, the order by rank counting
//   k_j_mark          one lane per entry of the active list: one flag byte per body
//   k_j_setup         one workgroup per bin walks the levels (0 first: the invalid joints): a lane builds its joint's rows into the solve record, warm-starts them
//   k_j_sweep         the same walk, `iterations` times in one launch: a lane loads the head, the two momentum records and row by row 80 bytes, stores 16 per row,
//                     the momentum and, after the last sweep, the joint's 32 bytes of accumulated impulses
//   k_j_connections   one lane per joint: its body pair, or (0, 0)
// Nothing is taken on trust from device memory: every span is clamped to the list and to NH_JOINT_SPAN_MAX, every entry of `order` must lie in its span, every level
// is clamped to the span's size (the barrier count is uniform and bounded), every body index is compared with bodies->count before it is used.
#include "nh_internal.h"
#include "nh_joint.h"

static_assert(sizeof(nh_Joint) == 64 && sizeof(nh_JointImpulse) == 32 && sizeof(nh_JointParams) == 16, "the joint records of the header");
static_assert(sizeof(nh_JRow) == 80 && sizeof(nh_JHead) == 32 && sizeof(nh_JSolve) == 432, "the solve record: 27 16-byte words");
#define NH_J_PER_LANE ((NH_JOINT_SPAN_MAX + 255u) / 256u)          // a lane's share of a span: 5 joints

// library-owned scratch (nh_context::joints) and which setup the solve records belong to
struct nh_JointState {
	nh_JSolve* solve; uint32_t solve_capacity;
	uint32_t* owner; uint8_t* live; uint32_t body_capacity;
	bool prepared; uint32_t prepared_bodies;                     // nh_joints_prepare has run; its bodies_count (nh_joint_connections' validity)
	bool setup_ok; uint32_t setup_seq, setup_count;              // an nh_joints_setup of `setup_count` joints ran in nh_collide number `setup_seq`, no nh_joints_prepare since
};

void nh_joints_free(nh_context* ctx) {
	nh_JointState* s = ctx->joints;
	if (!s) return;
	void* bufs[] = { s->solve, s->owner, s->live };
	for (void* b : bufs) if (b) hipFree(b);
	delete s;
	ctx->joints = nullptr;
}

// ---- loaders: 16-byte accesses of the records ------------------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ T nh_j_load(const void* base, size_t index) {
	static_assert(sizeof(T) % 16 == 0, "whole 16-byte words");
	union { uint4 q[sizeof(T) / 16]; T r; } u;
	const uint4* src = reinterpret_cast<const uint4*>(base) + (sizeof(T) / 16) * index;
#pragma unroll
	for (uint32_t k = 0; k < sizeof(T) / 16; ++k) u.q[k] = src[k];
	return u.r;
}
template <class T>
__device__ __forceinline__ void nh_j_store(void* base, size_t index, const T& r) {
	static_assert(sizeof(T) % 16 == 0, "whole 16-byte words");
	union { uint4 q[sizeof(T) / 16]; T r; } u;
	u.r = r;
	uint4* dst = reinterpret_cast<uint4*>(base) + (sizeof(T) / 16) * index;
#pragma unroll
	for (uint32_t k = 0; k < sizeof(T) / 16; ++k) dst[k] = u.q[k];
}

// what validity reads of joint j: the first 16 bytes and p[0], p[1]
__device__ __forceinline__ bool nh_j_valid_at(const nh_Joint* joints, uint32_t j, uint32_t body_count, uint32_t* a, uint32_t* b) {
	const uint4* src = reinterpret_cast<const uint4*>(joints) + 4u * (size_t)j;
	const uint4 h = src[0], t = src[2];
	*a = h.x; *b = h.y;
	return nh_j_valid(h.x, h.y, h.z, h.w, __uint_as_float(t.z), __uint_as_float(t.w), body_count);
}

// the span of bin w, clamped: [s, s + n)
__device__ __forceinline__ void nh_j_span(const uint32_t* offsets, uint32_t A, uint32_t count, uint32_t w, uint32_t* s, uint32_t* n) {
	const uint32_t b = nh_j_span_begin(offsets, A, count, w), e = nh_j_span_begin(offsets, A, count, w + 1u);
	*s = b;
	*n = e > b ? min(e - b, (uint32_t)NH_JOINT_SPAN_MAX) : 0u;
}

// ---- prepare -----------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_j_init(uint32_t count, uint32_t body_count, uint32_t* __restrict__ status, uint32_t* __restrict__ levels,
                                                 uint32_t* __restrict__ order, uint32_t* __restrict__ owner) {
	const uint32_t n = max(count, body_count);
	if (blockIdx.x == 0 && threadIdx.x < 4u) status[threadIdx.x] = 0u;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		if (i < count) { levels[i] = 0u; order[i] = i; }
		if (i < body_count) owner[i] = NH_NONE;
	}
}

__global__ __launch_bounds__(256) void k_j_offsets(const uint32_t* __restrict__ offsets, uint32_t A, uint32_t count, uint32_t* status) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= A; i += gridDim.x * blockDim.x) {
		const uint32_t o = nh_j_offset(offsets, count, i);
		uint32_t bits = 0u;
		if (i == 0u && o != 0u) bits |= NH_JOINT_ERR_OFFSETS;
		if (i == A && o != count) bits |= NH_JOINT_ERR_OFFSETS;
		if (i < A) {
			const uint32_t o1 = nh_j_offset(offsets, count, i + 1u);
			if (o1 < o) bits |= NH_JOINT_ERR_OFFSETS;
			else if (o1 - o > NH_JOINT_ASSEMBLY_MAX) bits |= NH_JOINT_ERR_ASSEMBLY_SIZE;
		}
		if (bits) atomicOr(&status[0], bits);
	}
}

template <int PASS>
__global__ __launch_bounds__(256) void k_j_owner(const nh_Joint* __restrict__ joints, uint32_t count, const uint32_t* __restrict__ offsets, uint32_t A,
                                                  uint32_t body_count, uint32_t* owner, uint32_t* status) {
	const bool binned = !(status[0] & NH_JOINT_ERR_OFFSETS);          // (this bit is k_j_offsets': final before either pass starts)
	for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < count; j += gridDim.x * blockDim.x) {
		uint32_t a, b;
		if (!nh_j_valid_at(joints, j, body_count, &a, &b)) continue;
		if (PASS == 0) atomicAdd(&status[1], 1u);
		if (!binned) continue;
		const uint32_t bin = nh_j_bin_of(offsets, A, count, j);
		if (PASS == 0) {
			if (a) atomicMin(&owner[a], bin);
			if (b) atomicMin(&owner[b], bin);
		} else if ((a && owner[a] != bin) || (b && owner[b] != bin)) atomicOr(&status[0], (uint32_t)NH_JOINT_ERR_SHARED_BODY);
	}
}

__global__ __launch_bounds__(256) void k_j_levels(const nh_Joint* __restrict__ joints, uint32_t count, const uint32_t* __restrict__ offsets, uint32_t A,
                                                   uint32_t body_count, uint32_t* status, uint32_t* __restrict__ levels, uint32_t* __restrict__ order) {
	__shared__ uint32_t sa[NH_JOINT_SPAN_MAX + 1u], sb[NH_JOINT_SPAN_MAX + 1u], lvl[NH_JOINT_SPAN_MAX + 1u];
	__shared__ int pa[NH_JOINT_SPAN_MAX + 1u], pb[NH_JOINT_SPAN_MAX + 1u];
	__shared__ uint32_t s_changed, s_max;
	if (status[0] != 0u) return;          // (final: every kernel that writes it has finished; uniform)
	uint32_t s, n;
	nh_j_span(offsets, A, count, blockIdx.x, &s, &n);
	if (n == 0u) return;                  // (uniform)
	const uint32_t tid = threadIdx.x;
	if (tid == 0u) { atomicAdd(&status[3], 1u); s_max = 0u; }
	for (uint32_t p = tid; p < n; p += 256u) {
		uint32_t a, b;
		const bool ok = nh_j_valid_at(joints, s + p, body_count, &a, &b);
		sa[p] = ok ? a : 0u; sb[p] = ok ? b : 0u;          // (a valid joint names at least one dynamic body: (0, 0) marks the invalid ones)
		lvl[p] = 0u;
	}
	__syncthreads();
	// predecessors: the last earlier joint of the span that names the body (an invalid joint names nobody)
	for (uint32_t p = tid; p < n; p += 256u) {
		const uint32_t a = sa[p], b = sb[p];
		int qa = -1, qb = -1;
		for (int q = (int)p - 1; q >= 0 && ((a && qa < 0) || (b && qb < 0)); --q) {
			const uint32_t xa = sa[q], xb = sb[q];
			if (a && qa < 0 && (xa == a || xb == a)) qa = q;
			if (b && qb < 0 && (xa == b || xb == b)) qb = q;
		}
		pa[p] = qa; pb[p] = qb;
	}
	// levels: a joint takes its level in the round after its predecessors have theirs (a level is written once, and read as 0 or as what it is)
	for (;;) {
		if (tid == 0u) s_changed = 0u;
		__syncthreads();
		for (uint32_t p = tid; p < n; p += 256u) {
			if (!(sa[p] | sb[p]) || lvl[p]) continue;
			const int qa = pa[p], qb = pb[p];
			const uint32_t la = qa >= 0 ? lvl[qa] : 0u, lb = qb >= 0 ? lvl[qb] : 0u;
			if ((qa >= 0 && !la) || (qb >= 0 && !lb)) continue;
			lvl[p] = 1u + max(la, lb);
			s_changed = 1u;
		}
		__syncthreads();
		const bool again = s_changed != 0u;
		__syncthreads();
		if (!again) break;
	}
	// the order: rank by (level, index)
	for (uint32_t p = tid; p < n; p += 256u) {
		const uint32_t l = lvl[p];
		uint32_t rank = 0u;
		for (uint32_t q = 0u; q < n; ++q) { const uint32_t lq = lvl[q]; rank += (lq < l || (lq == l && q < p)) ? 1u : 0u; }
		levels[s + p] = l;
		order[s + rank] = s + p;
		atomicMax(&s_max, l);
	}
	__syncthreads();
	if (tid == 0u) atomicMax(&status[2], s_max);
}

// ---- setup and sweeps --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_j_mark(const nh_DevState* __restrict__ st, const uint32_t* __restrict__ active, uint32_t capacity, uint8_t* __restrict__ live,
                                                 uint32_t body_count) {
	const uint32_t n = min(st->active, capacity);
	for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
		const uint32_t i = active[k];
		if (i < body_count) live[i] = 1u;
	}
}

struct nh_JBodies { const nh_Transform* transforms; const nh_BodyProperties* properties; nh_BodyMomentum* momentum; uint32_t count; };

__device__ __forceinline__ nh_JSide nh_j_side_at(const nh_JBodies& bd, uint32_t body) {
	const nh_Transform t = nh_j_load<nh_Transform>(bd.transforms, body);
	const nh_BodyProperties pr = nh_j_load<nh_BodyProperties>(bd.properties, body);
	return nh_j_side(body, t, pr);
}

// a lane's share of its bin's span: the joints order[s + tid + 256 c] and their levels; the span's highest level (at most its size) in *top
__device__ __forceinline__ void nh_j_share(uint32_t s, uint32_t n, const uint32_t* __restrict__ levels, const uint32_t* __restrict__ order,
                                           uint32_t (&myj)[NH_J_PER_LANE], uint32_t (&myl)[NH_J_PER_LANE], uint32_t* top) {
	uint32_t t = 0u;
#pragma unroll
	for (uint32_t c = 0u; c < NH_J_PER_LANE; ++c) {
		const uint32_t k = threadIdx.x + 256u * c;
		myj[c] = NH_NONE; myl[c] = 0u;
		if (k < n) {
			const uint32_t j = order[s + k];
			if (j >= s && j - s < n) { myj[c] = j; myl[c] = min(levels[j], n); t = max(t, myl[c]); }
		}
	}
	atomicMax(top, t);
}

__device__ __forceinline__ void nh_j_setup_one(const nh_Joint* __restrict__ joints, uint32_t jx, const nh_JBodies& bd, const uint8_t* __restrict__ live,
                                               const nh_JointParams& pm, const nh_JointImpulse* __restrict__ impulses, nh_JSolve* __restrict__ solve) {
	const nh_Joint j = nh_j_load<nh_Joint>(joints, jx);
	nh_JHead h = { j.a, j.b, 0u, j.type, 0.0f, 0.0f, { 0.0f, 0.0f } };
	uint4* rec = reinterpret_cast<uint4*>(solve + jx);
	const bool is_live = nh_j_valid(j, bd.count) && ((j.a && live[j.a]) || (j.b && live[j.b]));
	if (!is_live) { nh_j_store(rec, 0, h); return; }
	const nh_JSide A = nh_j_side_at(bd, j.a), B = nh_j_side_at(bd, j.b);
	const nh_JFrame f = nh_j_frame(j, A, B);
	const nh_JointImpulse imp = nh_j_load<nh_JointImpulse>(impulses, jx);
	nh_JMom ma = j.a ? nh_j_load<nh_JMom>(bd.momentum, j.a) : nh_j_zero_mom();
	nh_JMom mb = j.b ? nh_j_load<nh_JMom>(bd.momentum, j.b) : nh_j_zero_mom();
	const uint32_t rows = nh_j_rows(j.type);
	for (uint32_t k = 0u; k < rows; ++k) {
		bool dead;
		nh_JRow r = nh_j_row(j, k, f, A, B, pm, &dead);
		r.acc = dead ? 0.0f : pm.warm * imp.row[k];
		nh_j_push(r, nh_j_linear(j.type, k), r.acc, A.mi, B.mi, ma, mb);
		nh_j_store(rec + 2u + 5u * k, 0, r);
	}
	if (j.a) nh_j_store(bd.momentum, j.a, ma);
	if (j.b) nh_j_store(bd.momentum, j.b, mb);
	h.rows = rows; h.mi_a = A.mi; h.mi_b = B.mi;
	nh_j_store(rec, 0, h);
}

__global__ __launch_bounds__(256) void k_j_setup(const nh_Joint* __restrict__ joints, uint32_t count, const uint32_t* __restrict__ offsets, uint32_t A,
                                                  const uint32_t* __restrict__ status, const uint32_t* __restrict__ levels, const uint32_t* __restrict__ order,
                                                  nh_JBodies bd, const uint8_t* __restrict__ live, nh_JointParams pm,
                                                  const nh_JointImpulse* __restrict__ impulses, nh_JSolve* __restrict__ solve) {
	__shared__ uint32_t s_top;
	if (status[0] != 0u) return;
	uint32_t s, n;
	nh_j_span(offsets, A, count, blockIdx.x, &s, &n);
	if (n == 0u) return;
	if (threadIdx.x == 0u) s_top = 0u;
	__syncthreads();
	uint32_t myj[NH_J_PER_LANE], myl[NH_J_PER_LANE];
	nh_j_share(s, n, levels, order, myj, myl, &s_top);
	__syncthreads();
	const uint32_t top = s_top;
	for (uint32_t L = 0u; L <= top; ++L) {
#pragma unroll
		for (uint32_t c = 0u; c < NH_J_PER_LANE; ++c)
			if (myj[c] != NH_NONE && myl[c] == L) nh_j_setup_one(joints, myj[c], bd, live, pm, impulses, solve);
		__syncthreads();          // level L's momentum is written before level L + 1 reads it
	}
}

__device__ __forceinline__ void nh_j_sweep_one(uint32_t jx, const nh_JBodies& bd, nh_JSolve* solve, nh_JointImpulse* impulses, bool last) {
	uint4* rec = reinterpret_cast<uint4*>(solve + jx);
	const nh_JHead h = nh_j_load<nh_JHead>(rec, 0);
	const uint32_t rows = min(h.rows, (uint32_t)NH_JOINT_ROWS_MAX);
	if (rows == 0u || h.a >= bd.count || h.b >= bd.count) return;          // not live this step
	nh_JMom ma = h.a ? nh_j_load<nh_JMom>(bd.momentum, h.a) : nh_j_zero_mom();
	nh_JMom mb = h.b ? nh_j_load<nh_JMom>(bd.momentum, h.b) : nh_j_zero_mom();
	nh_JointImpulse out;
	for (uint32_t k = 0u; k < 6u; ++k) out.row[k] = 0.0f;
	out.reserved[0] = out.reserved[1] = 0u;
	for (uint32_t k = 0u; k < rows; ++k) {
		nh_JRow r = nh_j_load<nh_JRow>(rec + 2u + 5u * k, 0);
		nh_j_visit(r, nh_j_linear(h.type, k), h.mi_a, h.mi_b, ma, mb);
		rec[2u + 5u * k + 4u] = make_uint4(__float_as_uint(r.wb[0]), __float_as_uint(r.wb[1]), __float_as_uint(r.wb[2]), __float_as_uint(r.acc));
		out.row[k] = r.acc;
	}
	if (h.a) nh_j_store(bd.momentum, h.a, ma);
	if (h.b) nh_j_store(bd.momentum, h.b, mb);
	if (last) nh_j_store(impulses, jx, out);
}

__global__ __launch_bounds__(256) void k_j_sweep(uint32_t count, const uint32_t* __restrict__ offsets, uint32_t A, const uint32_t* __restrict__ status,
                                                  const uint32_t* __restrict__ levels, const uint32_t* __restrict__ order, nh_JBodies bd, nh_JSolve* solve,
                                                  nh_JointImpulse* impulses, uint32_t iterations) {
	__shared__ uint32_t s_top;
	if (status[0] != 0u) return;
	uint32_t s, n;
	nh_j_span(offsets, A, count, blockIdx.x, &s, &n);
	if (n == 0u) return;
	if (threadIdx.x == 0u) s_top = 0u;
	__syncthreads();
	uint32_t myj[NH_J_PER_LANE], myl[NH_J_PER_LANE];
	nh_j_share(s, n, levels, order, myj, myl, &s_top);
	__syncthreads();
	const uint32_t top = s_top;
	for (uint32_t it = 0u; it < iterations; ++it)
		for (uint32_t L = 1u; L <= top; ++L) {
#pragma unroll
			for (uint32_t c = 0u; c < NH_J_PER_LANE; ++c)
				if (myj[c] != NH_NONE && myl[c] == L) nh_j_sweep_one(myj[c], bd, solve, impulses, it + 1u == iterations);
			__syncthreads();
		}
}

__global__ __launch_bounds__(256) void k_j_connections(const nh_Joint* __restrict__ joints, uint32_t count, uint32_t body_count, nh_BodyPair* __restrict__ out) {
	for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < count; j += gridDim.x * blockDim.x) {
		uint32_t a, b;
		const bool ok = nh_j_valid_at(joints, j, body_count, &a, &b);
		out[j] = nh_BodyPair{ ok ? a : 0u, ok ? b : 0u };
	}
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------------------
// The scratch for `joints` joints and `bodies` bodies; a growth waits for the stream first (an earlier call may still use the old buffers).  Solve records that
// move are void: the setup they came from no longer counts.
static int nh_j_reserve(nh_context* ctx, uint32_t joints, uint32_t bodies) {
	if (!ctx->joints) ctx->joints = new nh_JointState();
	nh_JointState* s = ctx->joints;
	if (joints > s->solve_capacity) {
		NH_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
		s->solve_capacity = 0; s->setup_ok = false;
		{ int rc = nh_device_buffers(ctx, { { &s->solve, sizeof(nh_JSolve) * (size_t)joints } }); if (rc) return rc; }
		s->solve_capacity = joints;
	}
	if (bodies > s->body_capacity) {
		NH_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
		s->body_capacity = 0;
		{ int rc = nh_device_buffers(ctx, { { &s->owner, sizeof(uint32_t) * (size_t)bodies }, { &s->live, (size_t)bodies } }); if (rc) return rc; }
		s->body_capacity = bodies;
	}
	return NH_OK;
}

static bool nh_j_list_ok(const nh_JointList* l) {
	return l && !(!l->joints && l->count) && !((uintptr_t)l->joints & 15u) && !((uintptr_t)l->offsets & 3u) && l->count < 0x80000000u && l->assemblies < 0x80000000u;
}
static bool nh_j_plan_ok(const nh_JointPlan* p, uint32_t count) {
	return p && p->status && p->levels && p->order && !(((uintptr_t)p->status | (uintptr_t)p->levels | (uintptr_t)p->order) & 3u) && p->capacity >= count;
}
static bool nh_j_bodies_ok(const nh_BodyData* b) { return b && !(b->count && (!b->transforms || !b->properties || !b->momentum)); }
static bool nh_j_param_ok(float x) { return (nh_asuint(x) & 0x7f800000u) != 0x7f800000u && x >= 0.0f; }

extern "C" int nh_joints_prepare(nh_context* ctx, uint32_t bodies_count, const nh_JointList* list, const nh_JointPlan* plan) {
	if (!ctx || !nh_j_list_ok(list) || !nh_j_plan_ok(plan, list->count)) return NH_ERR_INVALID;
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	{ const int rc = nh_j_reserve(ctx, 0u, bodies_count); if (rc) return rc; }
	nh_JointState* s = ctx->joints;
	s->prepared = true; s->prepared_bodies = bodies_count; s->setup_ok = false;
	const uint32_t n = list->count, A = nh_j_assemblies(list->offsets, list->assemblies);
	NH_LAUNCH(ctx, "j_owner", k_j_init, nh_grid_for(n > bodies_count ? n : bodies_count, 256, 4096), 256, n, bodies_count, plan->status, plan->levels, plan->order, s->owner);
	if (n == 0u) return NH_OK;
	NH_LAUNCH(ctx, "j_owner", k_j_offsets, nh_grid_for((uint64_t)A + 1u, 256, 4096), 256, list->offsets, A, n, plan->status);
	NH_LAUNCH(ctx, "j_owner", k_j_owner<0>, nh_grid_for(n, 256, 4096), 256, list->joints, n, list->offsets, A, bodies_count, s->owner, plan->status);
	NH_LAUNCH(ctx, "j_owner", k_j_owner<1>, nh_grid_for(n, 256, 4096), 256, list->joints, n, list->offsets, A, bodies_count, s->owner, plan->status);
	NH_LAUNCH(ctx, "j_levels", k_j_levels, nh_j_bins(n), 256, list->joints, n, list->offsets, A, bodies_count, plan->status, plan->levels, plan->order);
	return NH_OK;
}

extern "C" int nh_joints_setup(nh_context* ctx, const nh_ActiveBodies* active_bodies, const nh_BodyData* bodies, const nh_JointList* list, const nh_JointPlan* plan,
                               const nh_JointParams* params, const nh_JointImpulse* impulses) {
	if (!ctx || !active_bodies || !nh_j_bodies_ok(bodies) || !nh_j_list_ok(list) || !nh_j_plan_ok(plan, list->count) || !params) return NH_ERR_INVALID;
	if ((!impulses && list->count) || ((uintptr_t)impulses & 15u) || ((uintptr_t)active_bodies->indices & 3u)) return NH_ERR_INVALID;
	if (!nh_j_param_ok(params->time_step) || !nh_j_param_ok(params->baumgarte) || !nh_j_param_ok(params->max_bias) || !nh_j_param_ok(params->warm) || params->warm > 1.0f)
		return NH_ERR_INVALID;
	{ int rc = nh_flush_pending(ctx); if (rc) return rc; }          // momentum is written: whatever was deferred comes first, a still step becomes a full one
	if (list->count == 0u) return NH_OK;
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	{ const int rc = nh_j_reserve(ctx, list->count, bodies->count); if (rc) return rc; }
	nh_JointState* s = ctx->joints;
	if (bodies->count) {
		NH_HIP_CHECK(ctx, hipMemsetAsync(s->live, 0, bodies->count, ctx->stream));
		if (active_bodies->indices && active_bodies->capacity)
			NH_LAUNCH(ctx, "j_setup", k_j_mark, nh_grid_for(bodies->count, 256, 2048), 256, ctx->d_state, active_bodies->indices, active_bodies->capacity, s->live, bodies->count);
	}
	const nh_JBodies bd{ bodies->transforms, bodies->properties, bodies->momentum, bodies->count };
	NH_LAUNCH(ctx, "j_setup", k_j_setup, nh_j_bins(list->count), 256, list->joints, list->count, list->offsets, nh_j_assemblies(list->offsets, list->assemblies),
	          plan->status, plan->levels, plan->order, bd, s->live, *params, impulses, s->solve);
	s->setup_ok = true; s->setup_seq = ctx->collide_seq; s->setup_count = list->count;
	return NH_OK;
}

extern "C" int nh_joints_apply(nh_context* ctx, const nh_BodyData* bodies, const nh_JointList* list, const nh_JointPlan* plan, nh_JointImpulse* impulses,
                               uint32_t iterations) {
	if (!ctx || !nh_j_bodies_ok(bodies) || !nh_j_list_ok(list) || !nh_j_plan_ok(plan, list->count) || iterations == 0u) return NH_ERR_INVALID;
	if ((!impulses && list->count) || ((uintptr_t)impulses & 15u)) return NH_ERR_INVALID;
	{ int rc = nh_flush_pending(ctx); if (rc) return rc; }
	if (list->count == 0u) return NH_OK;
	nh_JointState* s = ctx->joints;
	if (!s || !s->setup_ok || s->setup_seq != ctx->collide_seq || s->setup_count != list->count) return NH_ERR_STALE_SETUP;
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	const nh_JBodies bd{ bodies->transforms, bodies->properties, bodies->momentum, bodies->count };
	NH_LAUNCH(ctx, "j_sweep", k_j_sweep, nh_j_bins(list->count), 256, list->count, list->offsets, nh_j_assemblies(list->offsets, list->assemblies), plan->status,
	          plan->levels, plan->order, bd, s->solve, impulses, iterations);
	return NH_OK;
}

extern "C" int nh_joint_connections(nh_context* ctx, const nh_JointList* list, nh_BodyPair* out) {
	if (!ctx || !nh_j_list_ok(list) || (!out && list->count) || ((uintptr_t)out & 7u)) return NH_ERR_INVALID;
	if (!ctx->joints || !ctx->joints->prepared) return NH_ERR_INVALID;
	if (list->count == 0u) return NH_OK;
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	NH_LAUNCH(ctx, "j_connections", k_j_connections, nh_grid_for(list->count, 256, 4096), 256, list->joints, list->count, ctx->joints->prepared_bodies, out);
	return NH_OK;
}
