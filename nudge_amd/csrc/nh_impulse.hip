// nh_impulse.hip -- body impulses (include/nudge_hip.h, "body impulses"): a list of impulse records summed per body and either written out
// (nh_impulse_sums) or added to the bodies' momentum (nh_body_impulses), and the two generators of such lists.  The per-item logic is nh_impulse.h's, which
// the host oracle compiles as well; here are the flags, the scans, the sort and the output rules around it -- nh_contact_pairs' chain with the body index
// as the key.  Kernel boundaries are the only hand-offs and no atomic decides where a sum goes: the bytes are a function of the input alone.
//   k_bi_run_flag     one lane per record: 1 where a run starts (a valid record whose body differs from the record's before it), and the list's length
//                     -- the device count clamped to the capacity -- for everything behind it
//   nh_scan_u32       in place: a run head's scan word is its run's index, the total the number of runs
//   k_bi_runs         one lane per run head walks its run with two 16-byte loads per record and writes ONE 32-byte partial nh_ImpulseSum, the run's key
//                     (its body) and its index as the value
//   nh_sort_u64_u32   STABLE, over only the 8-bit passes bits(bodies->count - 1) need: the runs of a body end up adjacent and in list order
//   k_bi_body_flag    1 where a body starts in the sorted keys;  nh_scan_u32: a body head's word is its record's position
//   k_bi_sums         one lane per body head merges its runs in order and writes the record with two 16-byte stores -- iff all records fit; its first
//                     lane writes the count
//   k_bi_apply        the same merge; then one 32-byte transform, one 16-byte property and two 16-byte momentum words loaded, two 16-byte words
//                     stored and, with the wake flag, one byte
//   k_bi_blast        one lane per record of a hit list: its segment by binary search, its body's position, one record out
//   k_bi_touch        one lane per touch slot: one record out
// Every record index a kernel reads is below the list's capacity, every run index below the number of records, every body index below bodies->count,
// every position k_bi_sums writes below the output's count, which is then at most its capacity -- whatever the device words hold.
#include "nh_internal.h"
#include "nh_impulse.h"

struct nh_BiCtl { uint32_t n, runs, bodies, pad; };

// library-owned scratch (nh_context::impulses), all by the record capacity: the run sums, keys and values, the flags and their scan
struct nh_ImpulseState {
	nh_BiCtl* ctl; uint32_t* hist;
	uint32_t* scan; nh_ImpulseSum* part; uint64_t* keys_a; uint64_t* keys_b; uint32_t* vals_a; uint32_t* vals_b; uint32_t capacity;
};

void nh_impulses_free(nh_context* ctx) {
	nh_ImpulseState* s = ctx->impulses;
	if (!s) return;
	void* bufs[] = { s->ctl, s->hist, s->scan, s->part, s->keys_a, s->keys_b, s->vals_a, s->vals_b };
	for (void* b : bufs) if (b) hipFree(b);
	delete s;
	ctx->impulses = nullptr;
}

// ---- loaders: 16-byte loads of the 32-byte records -----------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ T nh_bi_load32(const void* base, size_t index) {
	static_assert(sizeof(T) == 32, "a 32-byte record");
	union { uint4 q[2]; T r; } u;
	const uint4* src = reinterpret_cast<const uint4*>(base) + 2u * index;
	u.q[0] = src[0]; u.q[1] = src[1];
	return u.r;
}
template <class T>
__device__ __forceinline__ void nh_bi_store32(void* base, size_t index, const T& r) {
	static_assert(sizeof(T) == 32, "a 32-byte record");
	union { uint4 q[2]; T r; } u;
	u.r = r;
	uint4* dst = reinterpret_cast<uint4*>(base) + 2u * index;
	dst[0] = u.q[0]; dst[1] = u.q[1];
}

struct nh_BiLoad {
	const nh_BodyImpulse* records; const nh_Transform* transforms; const nh_ImpulseSum* parts;
	__device__ __forceinline__ uint32_t body(uint32_t i) const { return records[i].body; }
	__device__ __forceinline__ nh_BodyImpulse record(uint32_t i) const { return nh_bi_load32<nh_BodyImpulse>(records, i); }
	__device__ __forceinline__ nh_f3 position(uint32_t b) const {
		const float4 p = *reinterpret_cast<const float4*>(transforms + b);
		return nh_make3(p.x, p.y, p.z);
	}
	__device__ __forceinline__ nh_ImpulseSum part(uint32_t r) const { return nh_bi_load32<nh_ImpulseSum>(parts, r); }
};

__device__ __forceinline__ uint32_t nh_bi_count(const uint32_t* count, uint32_t capacity) {
	if (!count) return capacity;
	const uint32_t c = *count;
	return c < capacity ? c : capacity;
}

// ---- the chain -------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bi_run_flag(nh_BiLoad ld, const uint32_t* __restrict__ count, uint32_t capacity, uint32_t body_count,
                                                      nh_BiCtl* __restrict__ ctl, uint32_t* __restrict__ scan) {
	const uint32_t n = nh_bi_count(count, capacity);
	if (blockIdx.x == 0 && threadIdx.x == 0) ctl->n = n;
	for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w <= n; w += (uint64_t)gridDim.x * blockDim.x)
		scan[w] = w < n && nh_bi_run_head(ld, body_count, (uint32_t)w) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_bi_runs(nh_BiLoad ld, const nh_BiCtl* __restrict__ ctl, uint32_t capacity, const uint32_t* __restrict__ scan,
                                                  nh_ImpulseSum* __restrict__ part, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
	const uint32_t n = min(ctl->n, capacity);
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const uint32_t r = scan[i];
		if (scan[i + 1u] == r || r >= n) continue;          // not a run head
		const nh_ImpulseSum s = nh_bi_run(ld, n, i);
		nh_bi_store32(part, r, s);
		keys[r] = s.body;
		vals[r] = r;
	}
}

__global__ __launch_bounds__(256) void k_bi_body_flag(const uint64_t* __restrict__ keys, const nh_BiCtl* __restrict__ ctl, uint32_t capacity,
                                                       uint32_t* __restrict__ scan) {
	const uint32_t runs = min(ctl->runs, capacity);
	for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w <= runs; w += (uint64_t)gridDim.x * blockDim.x)
		scan[w] = w < runs && (w == 0u || keys[w] != keys[w - 1u]) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_bi_sums(nh_BiLoad ld, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                  const uint32_t* __restrict__ scan, const nh_BiCtl* __restrict__ ctl, uint32_t capacity,
                                                  uint32_t* __restrict__ out_count, nh_ImpulseSum* __restrict__ out, uint32_t out_capacity) {
	const uint32_t runs = min(ctl->runs, capacity), bodies = ctl->bodies;
	if (blockIdx.x == 0 && threadIdx.x == 0) *out_count = bodies;
	if (!out || bodies > out_capacity) return;          // all or none
	for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < runs; w += gridDim.x * blockDim.x) {
		const uint32_t at = scan[w];
		if (scan[w + 1u] == at || at >= bodies) continue;          // not a body head
		nh_bi_store32(out, at, nh_bi_merge(ld, keys, vals, runs, w));
	}
}

template <bool WAKE>
__global__ __launch_bounds__(256) void k_bi_apply(nh_BiLoad ld, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                   const uint32_t* __restrict__ scan, const nh_BiCtl* __restrict__ ctl, uint32_t capacity,
                                                   const nh_BodyProperties* __restrict__ properties, nh_BodyMomentum* __restrict__ momentum,
                                                   uint8_t* __restrict__ idle, uint32_t body_count) {
	const uint32_t runs = min(ctl->runs, capacity);
	for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < runs; w += gridDim.x * blockDim.x) {
		if (scan[w + 1u] == scan[w]) continue;          // not a body head
		const nh_ImpulseSum s = nh_bi_merge(ld, keys, vals, runs, w);
		if (!nh_bi_valid(s.body, body_count)) continue;          // (a run's body is valid by the flag kernel's test: no index is taken on trust)
		const nh_Transform t = nh_bi_load32<nh_Transform>(ld.transforms, s.body);
		const float4 p = *reinterpret_cast<const float4*>(properties + s.body);
		const nh_BodyProperties pr = { { p.x, p.y, p.z }, p.w };
		float4* m = reinterpret_cast<float4*>(momentum + s.body);
		float4 v = m[0], a = m[1];          // (.w: unused0 / unused1, stored back as loaded)
		nh_bi_apply(&v.x, &a.x, t.rotation, pr, s);
		m[0] = v; m[1] = a;
		if (WAKE) idle[s.body] = 0u;
	}
}

// ---- the generators --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bi_blast(nh_BiLoad ld, uint32_t body_count, const nh_Blast* __restrict__ blasts, uint32_t count,
                                                   const uint32_t* __restrict__ offsets, const uint4* __restrict__ hits, uint32_t capacity,
                                                   nh_BodyImpulse* __restrict__ out) {
	const uint32_t n = min(offsets[count], capacity);
	for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
		const nh_Blast b = nh_bi_load32<nh_Blast>(blasts, nh_bi_segment(offsets, count, j));
		nh_bi_store32(out, j, nh_bi_blast(ld, b, hits[j].x, body_count));
	}
}

__global__ __launch_bounds__(256) void k_bi_touch(const nh_Push* __restrict__ pushes, uint32_t count, uint32_t k, const uint32_t* __restrict__ counts,
                                                   const nh_Touch* __restrict__ touches, nh_BodyImpulse* __restrict__ out) {
	const uint64_t slots = (uint64_t)count * k;
	for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < slots; w += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t i = (uint32_t)(w / k), j = (uint32_t)(w - (uint64_t)i * k);
		nh_BodyImpulse o = nh_bi_nobody();
		if (j < min(counts[i], k)) {
			union { uint4 q[4]; nh_Touch t; } u;
			const uint4* src = reinterpret_cast<const uint4*>(touches) + 4u * w;
			u.q[0] = src[0]; u.q[1] = src[1]; u.q[2] = src[2]; u.q[3] = src[3];
			const uint4 pq = *reinterpret_cast<const uint4*>(pushes + i);
			const nh_Push p = { __uint_as_float(pq.x), __uint_as_float(pq.y), pq.z, pq.w };
			o = nh_bi_touch(p, u.t);
		}
		nh_bi_store32(out, w, o);
	}
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------------
// The scratch for `records` records; a growth waits for the stream first (an earlier call may still read the old buffers) and happens only when the
// capacity exceeds every earlier one.
static int nh_bi_reserve(nh_context* ctx, uint32_t records) {
	if (!ctx->impulses) ctx->impulses = new nh_ImpulseState();
	nh_ImpulseState* s = ctx->impulses;
	if (!s->ctl) {
		NH_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
		{ int rc = nh_device_buffers(ctx, { { &s->ctl, sizeof(nh_BiCtl), true }, { &s->hist, sizeof(uint32_t) * (256u * NH_SORT_GRID + 512u) } }); if (rc) return rc; }
	}
	if (records > s->capacity) {
		NH_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
		s->capacity = 0;
		const size_t c = records;
		{ int rc = nh_device_buffers(ctx, { { &s->scan, sizeof(uint32_t) * (c + 2u + 16u) }, { &s->part, sizeof(nh_ImpulseSum) * c }, { &s->keys_a, sizeof(uint64_t) * c },
		                                    { &s->keys_b, sizeof(uint64_t) * c }, { &s->vals_a, sizeof(uint32_t) * c }, { &s->vals_b, sizeof(uint32_t) * c } }); if (rc) return rc; }
		s->capacity = records;
	}
	return NH_OK;
}

static bool nh_bi_list_ok(const nh_ImpulseList* l) {
	return l && !(!l->records && l->capacity) && !((uintptr_t)l->records & 15u) && !((uintptr_t)l->count & 3u) && l->capacity < 0x80000000u;
}

static bool nh_bi_sumlist_ok(const nh_ImpulseSumList* l) {
	return l && l->count && !((uintptr_t)l->count & 3u) && !(!l->sums && l->capacity) && !((uintptr_t)l->sums & 15u) && l->capacity < 0x80000000u;
}

// the chain up to the scan of the body heads, behind the argument checks (in.capacity > 0): the sorted keys and values for the kernel that ends it
struct nh_BiSorted { nh_BiLoad ld; const uint64_t* keys; const uint32_t* vals; uint32_t grid; };

static int nh_bi_pipeline(nh_context* ctx, const nh_BodyData* bodies, const nh_ImpulseList& in, nh_BiSorted* out) {
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	{ const int rc = nh_bi_reserve(ctx, in.capacity); if (rc) return rc; }
	nh_ImpulseState* s = ctx->impulses;
	const uint32_t grid = nh_grid_for((uint64_t)in.capacity + 1u, 256, 1u << 16);
	const nh_BiLoad ld{ in.records, bodies->transforms, s->part };
	NH_LAUNCH(ctx, "bi_run_flag", k_bi_run_flag, grid, 256, ld, in.count, in.capacity, bodies->count, s->ctl, s->scan);
	nh_scan_u32(ctx, s->scan, s->scan, &s->ctl->n, 1u, s->hist, &s->ctl->runs);
	NH_LAUNCH(ctx, "bi_runs", k_bi_runs, grid, 256, ld, s->ctl, in.capacity, s->scan, s->part, s->keys_a, s->vals_a);
	const int in_b = nh_sort_u64_u32(ctx, s->keys_a, s->keys_b, s->vals_a, s->vals_b, &s->ctl->runs, s->hist, 0, nh_bi_sort_bits(nh_bi_bits(bodies->count)));
	const uint64_t* keys = in_b ? s->keys_b : s->keys_a;
	NH_LAUNCH(ctx, "bi_body_flag", k_bi_body_flag, grid, 256, keys, s->ctl, in.capacity, s->scan);
	nh_scan_u32(ctx, s->scan, s->scan, &s->ctl->runs, 1u, s->hist, &s->ctl->bodies);
	*out = nh_BiSorted{ ld, keys, in_b ? s->vals_b : s->vals_a, grid };
	return NH_OK;
}

extern "C" int nh_impulse_sums(nh_context* ctx, const nh_BodyData* bodies, const nh_ImpulseList* in, const nh_ImpulseSumList* out, uint32_t flags) {
	if (!ctx || flags || !bodies || !nh_bi_list_ok(in) || !nh_bi_sumlist_ok(out)) return NH_ERR_INVALID;
	if (bodies->count && !bodies->transforms) return NH_ERR_INVALID;
	if (in->capacity == 0u) {          // no record can be read: no body
		NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
		NH_HIP_CHECK(ctx, hipMemsetAsync(out->count, 0, sizeof(uint32_t), ctx->stream));
		return NH_OK;
	}
	nh_BiSorted so;
	{ const int rc = nh_bi_pipeline(ctx, bodies, *in, &so); if (rc) return rc; }
	NH_LAUNCH(ctx, "bi_sums", k_bi_sums, so.grid, 256, so.ld, so.keys, so.vals, ctx->impulses->scan, ctx->impulses->ctl, in->capacity, out->count,
	          out->capacity ? out->sums : (nh_ImpulseSum*)nullptr, out->capacity);
	return NH_OK;
}

extern "C" int nh_body_impulses(nh_context* ctx, const nh_BodyData* bodies, const nh_ImpulseList* in, uint32_t flags) {
	if (!ctx || (flags & ~(uint32_t)NH_IMPULSE_WAKE) || !bodies || !nh_bi_list_ok(in)) return NH_ERR_INVALID;
	if (bodies->count && (!bodies->transforms || !bodies->properties || !bodies->momentum || !bodies->idle_counters)) return NH_ERR_INVALID;
	{ int rc = nh_flush_pending(ctx); if (rc) return rc; }          // momentum is written: whatever was deferred comes first
	if (in->capacity == 0u) return NH_OK;
	// idle counters are rewritten from outside the step; whether anybody was asleep is known only on the device
	if (flags & NH_IMPULSE_WAKE) { int rc = nh_bodies_changed(ctx); if (rc) return rc; }
	nh_BiSorted so;
	{ const int rc = nh_bi_pipeline(ctx, bodies, *in, &so); if (rc) return rc; }
	nh_ImpulseState* s = ctx->impulses;
	if (flags & NH_IMPULSE_WAKE)
		NH_LAUNCH(ctx, "bi_apply", k_bi_apply<true>, so.grid, 256, so.ld, so.keys, so.vals, s->scan, s->ctl, in->capacity, bodies->properties, bodies->momentum,
		          bodies->idle_counters, bodies->count);
	else
		NH_LAUNCH(ctx, "bi_apply", k_bi_apply<false>, so.grid, 256, so.ld, so.keys, so.vals, s->scan, s->ctl, in->capacity, bodies->properties, bodies->momentum,
		          bodies->idle_counters, bodies->count);
	return NH_OK;
}

extern "C" int nh_blast_impulses(nh_context* ctx, const nh_BodyData* bodies, const nh_Blast* blasts, uint32_t count, const nh_HitList* hits,
                                 nh_BodyImpulse* out, uint32_t flags) {
	if (!ctx || flags || !bodies || !hits || (bodies->count && !bodies->transforms)) return NH_ERR_INVALID;
	if (hits->capacity >= 0x80000000u || ((uintptr_t)blasts & 15u) || ((uintptr_t)hits->offsets & 3u) || ((uintptr_t)hits->hits & 15u) || ((uintptr_t)out & 15u)) return NH_ERR_INVALID;
	if (count && (!blasts || !hits->offsets)) return NH_ERR_INVALID;
	if (count && hits->capacity && (!hits->hits || !out)) return NH_ERR_INVALID;
	if (count == 0u || hits->capacity == 0u) return NH_OK;          // no record can be read: none is written
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	const nh_BiLoad ld{ nullptr, bodies->transforms, nullptr };
	NH_LAUNCH(ctx, "bi_blast", k_bi_blast, nh_grid_for(hits->capacity, 256, 1u << 16), 256, ld, bodies->count, blasts, count, hits->offsets,
	          reinterpret_cast<const uint4*>(hits->hits), hits->capacity, out);
	return NH_OK;
}

extern "C" int nh_touch_impulses(nh_context* ctx, const nh_Push* pushes, uint32_t count, uint32_t k, const uint32_t* counts, const nh_Touch* touches,
                                 nh_BodyImpulse* out, uint32_t flags) {
	if (!ctx || flags) return NH_ERR_INVALID;
	if (((uintptr_t)pushes & 15u) || ((uintptr_t)counts & 3u) || ((uintptr_t)touches & 15u) || ((uintptr_t)out & 15u)) return NH_ERR_INVALID;
	if ((uint64_t)count * k >= 0x80000000ull) return NH_ERR_INVALID;
	if (count && k && (!pushes || !counts || !touches || !out)) return NH_ERR_INVALID;
	if (count == 0u || k == 0u) return NH_OK;
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	NH_LAUNCH(ctx, "bi_touch", k_bi_touch, nh_grid_for((uint64_t)count * k, 256, 1u << 16), 256, pushes, count, k, counts, touches, out);
	return NH_OK;
}
