// nh_contact_events.hip -- contact events (include/nudge_hip.h, "contact events"): one record per touching body pair out of a contact
// list, and the difference of two such lists.  The per-item logic is nh_contact_events.h's, which the host oracle compiles as well; here are the
// flags, the scans, the sort and the compaction around it.  Kernel boundaries are the only hand-offs and no atomic decides where a record goes: the
// bytes are a function of the input alone.
//   nh_contact_pairs    k_cp_run_flag    one lane per contact: 1 where a run starts (its (lo, hi) differs from the contact's before it), and the
//                                        list's length -- the device count clamped to the capacity -- for everything behind it
//                       nh_scan_u32      in place: a run head's scan word is its run's index, the total the number of runs
//                       k_cp_runs        one lane per run head walks its run (with the step-bound call: finds each contact's cache entry first) and
//                                        writes ONE partial record, the run's key lo << bits | hi and its index as the value
//                       nh_sort_u64_u32  STABLE, over only the passes 2 x bits need: the runs of a pair end up adjacent and in list order
//                       k_cp_pair_flag   1 where a pair starts in the sorted keys;  nh_scan_u32: a pair head's word is its record's position
//                       k_cp_merge       one lane per pair head merges its runs in order and writes the 64-byte record with four 16-byte stores --
//                                        iff all records fit; its first lane writes the count
//   nh_contact_events   k_cp_ev_flag     one lane per record of cur, then of prev: 1 where its (lo, hi) is not in the other list (binary search)
//                       nh_scan_u32      over both ranges at once, each with a closing 0 word
//                       k_cp_ev_compact  the counts; a flagged record is copied whole iff its output takes all of its records
// Every contact index a kernel reads is below the list's capacity, every run index below the number of contacts, every position it writes below the
// output's count, which is then at most its capacity -- whatever the device words hold.
#include "nh_internal.h"
#include "nh_contact_events.h"

struct nh_CpCtl { uint32_t n, runs, pairs, ev_cur, ev_prev, ev_words, pad[2]; };

// library-owned scratch (nh_context::contact_events): by contact capacity the run records, keys and values; by words the flags and their scan
struct nh_CpState {
	nh_CpCtl* ctl; uint32_t* hist;
	uint32_t* scan; uint32_t scan_capacity;
	nh_ContactPair* part; uint64_t* keys_a; uint64_t* keys_b; uint32_t* vals_a; uint32_t* vals_b; uint32_t contact_capacity;
};

void nh_contact_events_free(nh_context* ctx) {
	nh_CpState* s = ctx->contact_events;
	if (!s) return;
	void* bufs[] = { s->ctl, s->hist, s->scan, s->part, s->keys_a, s->keys_b, s->vals_a, s->vals_b };
	for (void* b : bufs) if (b) hipFree(b);
	delete s;
	ctx->contact_events = nullptr;
}

// ---- loaders: 16-byte loads of the 32-byte contact, the 16-byte impulse and the 64-byte record ----------------------------------------------------
__device__ __forceinline__ nh_ContactPair nh_cp_record(const uint4* records, uint32_t r) {
	union { uint4 q[4]; nh_ContactPair p; } u;
	const uint4* src = records + 4u * (size_t)r;
	u.q[0] = src[0]; u.q[1] = src[1]; u.q[2] = src[2]; u.q[3] = src[3];
	return u.p;
}

struct nh_CpCache { const uint64_t* tags; const uint32_t* features; const uint64_t* ctags; const uint32_t* cfeatures; const float4* cdata; uint32_t m; };

template <bool LOOKUP>
struct nh_CpLoad {
	const float4* data; const uint2* bodies; const float4* impulses; const uint4* parts; nh_CpCache cache;
	__device__ __forceinline__ nh_Contact contact(uint32_t j) const {
		const float4 a = data[2u * (size_t)j], b = data[2u * (size_t)j + 1u];
		return nh_Contact{ { a.x, a.y, a.z }, a.w, { b.x, b.y, b.z }, b.w };
	}
	__device__ __forceinline__ nh_BodyPair pair(uint32_t j) const { const uint2 p = bodies[j]; return nh_BodyPair{ p.x, p.y }; }
	__device__ __forceinline__ nh_f3 impulse(uint32_t j) const {
		if (LOOKUP) {
			const uint32_t at = nh_cp_cache_find(cache.ctags, cache.cfeatures, cache.m, j, cache.tags[j], cache.features[j]);
			if (at == NH_CP_NONE) return nh_make3(0.0f, 0.0f, 0.0f);
			const float4 v = cache.cdata[at];
			return nh_make3(v.x, v.y, v.z);
		}
		if (!impulses) return nh_make3(0.0f, 0.0f, 0.0f);
		const float4 v = impulses[j];
		return nh_make3(v.x, v.y, v.z);
	}
	__device__ __forceinline__ nh_ContactPair part(uint32_t r) const { return nh_cp_record(parts, r); }
};

__device__ __forceinline__ void nh_cp_store(nh_ContactPair* dst, const nh_ContactPair& r) {
	union { uint4 q[4]; nh_ContactPair p; } u;
	u.p = r;
	uint4* d = reinterpret_cast<uint4*>(dst);
	d[0] = u.q[0]; d[1] = u.q[1]; d[2] = u.q[2]; d[3] = u.q[3];
}

__device__ __forceinline__ uint32_t nh_cp_count(const uint32_t* count, uint32_t capacity) {
	if (!count) return capacity;
	const uint32_t c = *count;
	return c < capacity ? c : capacity;
}

// ---- nh_contact_pairs ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cp_run_flag(const uint2* __restrict__ bodies, const uint32_t* __restrict__ count, uint32_t capacity,
                                                      nh_CpCtl* __restrict__ ctl, uint32_t* __restrict__ scan) {
	const uint32_t n = nh_cp_count(count, capacity);
	if (blockIdx.x == 0 && threadIdx.x == 0) ctl->n = n;
	for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w <= n; w += (uint64_t)gridDim.x * blockDim.x) {
		uint32_t f = 0u;
		if (w < n) {
			const uint32_t i = (uint32_t)w;
			if (i == 0u) f = 1u;
			else {
				const uint2 p = bodies[i], q = bodies[i - 1u];
				f = nh_cp_pair(nh_BodyPair{ p.x, p.y }) != nh_cp_pair(nh_BodyPair{ q.x, q.y }) ? 1u : 0u;
			}
		}
		scan[w] = f;
	}
}

template <bool LOOKUP>
__global__ __launch_bounds__(256) void k_cp_runs(nh_CpLoad<LOOKUP> ld, const uint32_t* __restrict__ cache_count, uint32_t cache_capacity,
                                                  const nh_CpCtl* __restrict__ ctl, const uint32_t* __restrict__ scan, uint32_t bits,
                                                  nh_ContactPair* __restrict__ part, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
	const uint32_t n = ctl->n;
	if (LOOKUP) ld.cache.m = nh_cp_count(cache_count, cache_capacity);
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const uint32_t r = scan[i];
		if (scan[i + 1u] == r || r >= n) continue;          // not a run head
		const nh_ContactPair rec = nh_cp_run(ld, n, i);
		nh_cp_store(part + r, rec);
		keys[r] = nh_cp_key(((uint64_t)rec.lo << 32) | rec.hi, bits);
		vals[r] = r;
	}
}

__global__ __launch_bounds__(256) void k_cp_pair_flag(const uint64_t* __restrict__ keys, const nh_CpCtl* __restrict__ ctl, uint32_t capacity,
                                                       uint32_t* __restrict__ scan) {
	const uint32_t runs = min(ctl->runs, capacity);
	for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w <= runs; w += (uint64_t)gridDim.x * blockDim.x)
		scan[w] = w < runs && (w == 0u || keys[w] != keys[w - 1u]) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_cp_merge(nh_CpLoad<false> ld, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                   const uint32_t* __restrict__ scan, const nh_CpCtl* __restrict__ ctl, uint32_t capacity,
                                                   uint32_t* __restrict__ out_count, nh_ContactPair* __restrict__ out, uint32_t out_capacity) {
	const uint32_t runs = min(ctl->runs, capacity), pairs = ctl->pairs;
	if (blockIdx.x == 0 && threadIdx.x == 0) *out_count = pairs;
	if (!out || pairs > out_capacity) return;          // all or none
	for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < runs; w += gridDim.x * blockDim.x) {
		const uint32_t at = scan[w];
		if (scan[w + 1u] == at || at >= pairs) continue;          // not a pair head
		nh_cp_store(out + at, nh_cp_merge(ld, keys, vals, runs, w));
	}
}

// ---- nh_contact_events ---------------------------------------------------------------------------------------------------------------------------
struct nh_CpPairs { const uint32_t* count; const nh_ContactPair* pairs; uint32_t capacity; };

// the lengths both kernels go by: 0 and 0 where an input is absent (its count exceeds its capacity)
__device__ __forceinline__ void nh_cp_ev_lengths(const nh_CpPairs& cur, const nh_CpPairs& prev, bool has_prev, uint32_t& cn, uint32_t& pn) {
	cn = *cur.count; pn = has_prev ? *prev.count : 0u;
	if (cn > cur.capacity || pn > prev.capacity) { cn = 0u; pn = 0u; }
}

__global__ __launch_bounds__(256) void k_cp_ev_flag(nh_CpPairs cur, nh_CpPairs prev, bool has_prev, nh_CpCtl* __restrict__ ctl, uint32_t* __restrict__ scan) {
	uint32_t cn, pn;
	nh_cp_ev_lengths(cur, prev, has_prev, cn, pn);
	const uint64_t words = (uint64_t)cn + pn + 2u;
	if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->ev_cur = cn; ctl->ev_prev = pn; ctl->ev_words = (uint32_t)words; }
	for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (uint64_t)gridDim.x * blockDim.x) {
		uint32_t f = 0u;
		if (w < cn) {
			const uint2 k = *reinterpret_cast<const uint2*>(cur.pairs + w);
			f = !has_prev || !nh_cp_find(prev.pairs, pn, k.x, k.y) ? 1u : 0u;
		} else if (w > cn && w - cn - 1u < pn) {
			const uint2 k = *reinterpret_cast<const uint2*>(prev.pairs + (w - cn - 1u));
			f = nh_cp_find(cur.pairs, cn, k.x, k.y) ? 0u : 1u;
		}
		scan[w] = f;
	}
}

__global__ __launch_bounds__(256) void k_cp_ev_compact(nh_CpPairs cur, nh_CpPairs prev, const uint32_t* __restrict__ scan, const nh_CpCtl* __restrict__ ctl,
                                                        uint32_t* __restrict__ began_count, nh_ContactPair* __restrict__ began, uint32_t began_capacity,
                                                        uint32_t* __restrict__ ended_count, nh_ContactPair* __restrict__ ended, uint32_t ended_capacity) {
	const uint32_t cn = min(ctl->ev_cur, cur.capacity), pn = min(ctl->ev_prev, prev.capacity);
	const uint32_t base = scan[cn + 1u], nb = scan[cn], ne = scan[cn + 1u + pn] - base;
	if (blockIdx.x == 0 && threadIdx.x == 0) { *began_count = nb; *ended_count = ne; }
	const bool write_b = began && nb <= began_capacity, write_e = ended && ne <= ended_capacity;
	if (!write_b && !write_e) return;
	const uint64_t words = (uint64_t)cn + pn + 1u;          // (the last word closes the scan)
	for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t at = scan[w];
		if (scan[w + 1u] == at || w == cn) continue;
		if (w < cn) { if (write_b && at < nb) nh_cp_store(began + at, nh_cp_record(reinterpret_cast<const uint4*>(cur.pairs), (uint32_t)w)); }
		else if (write_e && at - base < ne) nh_cp_store(ended + (at - base), nh_cp_record(reinterpret_cast<const uint4*>(prev.pairs), (uint32_t)(w - cn - 1u)));
	}
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------------
// The scratch for `contacts` contacts and `words` flag words; a growth waits for the stream first (an earlier call may still read the old buffers) and
// happens only when a capacity exceeds every earlier one.
static int nh_cp_reserve(nh_context* ctx, uint32_t contacts, uint64_t words) {
	if (!ctx->contact_events) ctx->contact_events = new nh_CpState();
	nh_CpState* s = ctx->contact_events;
	if (!s->ctl) {
		NH_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
		{ int rc = nh_device_buffers(ctx, { { &s->ctl, sizeof(nh_CpCtl), true }, { &s->hist, sizeof(uint32_t) * (256u * NH_SORT_GRID + 512u) } }); if (rc) return rc; }
	}
	if (words > s->scan_capacity) {
		NH_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
		s->scan_capacity = 0;
		{ int rc = nh_device_buffers(ctx, { { &s->scan, sizeof(uint32_t) * ((size_t)words + 16u) } }); if (rc) return rc; }
		s->scan_capacity = (uint32_t)words;
	}
	if (contacts > s->contact_capacity) {
		NH_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
		s->contact_capacity = 0;
		const size_t c = contacts;
		{ int rc = nh_device_buffers(ctx, { { &s->part, sizeof(nh_ContactPair) * c }, { &s->keys_a, sizeof(uint64_t) * c }, { &s->keys_b, sizeof(uint64_t) * c },
		                                    { &s->vals_a, sizeof(uint32_t) * c }, { &s->vals_b, sizeof(uint32_t) * c } }); if (rc) return rc; }
		s->contact_capacity = contacts;
	}
	return NH_OK;
}

static bool nh_cp_pairlist_ok(const nh_PairList* l) {
	return l && l->count && !((uintptr_t)l->count & 3u) && !(!l->pairs && l->capacity) && !((uintptr_t)l->pairs & 15u) && l->capacity < 0x80000000u;
}

// the pipeline behind the argument checks: `in` with its arrays in place (impulses unused where `cache` is given: the step-bound call)
static int nh_cp_pipeline(nh_context* ctx, const nh_ContactList& in, const nh_CpCache* cache, const uint32_t* cache_count, uint32_t cache_capacity, const nh_PairList* out) {
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	if (in.capacity == 0u) {          // no contact can be read: no pair
		NH_HIP_CHECK(ctx, hipMemsetAsync(out->count, 0, sizeof(uint32_t), ctx->stream));
		return NH_OK;
	}
	{ const int rc = nh_cp_reserve(ctx, in.capacity, (uint64_t)in.capacity + 2u); if (rc) return rc; }
	nh_CpState* s = ctx->contact_events;
	const uint32_t bits = nh_cp_bits(in.body_count), grid = nh_grid_for((uint64_t)in.capacity + 1u, 256, 1u << 16);
	nh_CpLoad<false> ld{ reinterpret_cast<const float4*>(in.data), reinterpret_cast<const uint2*>(in.bodies), reinterpret_cast<const float4*>(in.impulses),
	                     reinterpret_cast<const uint4*>(s->part), {} };
	NH_LAUNCH(ctx, "cp_run_flag", k_cp_run_flag, grid, 256, ld.bodies, in.count, in.capacity, s->ctl, s->scan);
	nh_scan_u32(ctx, s->scan, s->scan, &s->ctl->n, 1u, s->hist, &s->ctl->runs);
	if (cache) {
		nh_CpLoad<true> lk{ ld.data, ld.bodies, nullptr, ld.parts, *cache };
		NH_LAUNCH(ctx, "cp_runs_lookup", k_cp_runs<true>, grid, 256, lk, cache_count, cache_capacity, s->ctl, s->scan, bits, s->part, s->keys_a, s->vals_a);
	} else
		NH_LAUNCH(ctx, "cp_runs", k_cp_runs<false>, grid, 256, ld, (const uint32_t*)nullptr, 0u, s->ctl, s->scan, bits, s->part, s->keys_a, s->vals_a);
	const int in_b = nh_sort_u64_u32(ctx, s->keys_a, s->keys_b, s->vals_a, s->vals_b, &s->ctl->runs, s->hist, 0, nh_cp_sort_bits(bits));
	const uint64_t* keys = in_b ? s->keys_b : s->keys_a;
	NH_LAUNCH(ctx, "cp_pair_flag", k_cp_pair_flag, grid, 256, keys, s->ctl, in.capacity, s->scan);
	nh_scan_u32(ctx, s->scan, s->scan, &s->ctl->runs, 1u, s->hist, &s->ctl->pairs);
	NH_LAUNCH(ctx, "cp_merge", k_cp_merge, grid, 256, ld, keys, in_b ? s->vals_b : s->vals_a, s->scan, s->ctl, in.capacity, out->count,
	          out->capacity ? out->pairs : (nh_ContactPair*)nullptr, out->capacity);
	return NH_OK;
}

extern "C" int nh_contact_pairs(nh_context* ctx, const nh_ContactList* in, const nh_PairList* out, uint32_t flags) {
	if (!ctx || flags || !in || !nh_cp_pairlist_ok(out)) return NH_ERR_INVALID;
	if (in->capacity >= 0x80000000u || ((uintptr_t)in->count & 3u)) return NH_ERR_INVALID;
	if (in->capacity && (!in->data || !in->bodies)) return NH_ERR_INVALID;
	if (((uintptr_t)in->data & 15u) || ((uintptr_t)in->bodies & 7u) || ((uintptr_t)in->impulses & 15u)) return NH_ERR_INVALID;
	return nh_cp_pipeline(ctx, *in, nullptr, nullptr, 0u, out);
}

extern "C" int nh_step_contact_pairs(nh_context* ctx, const nh_ContactData* contacts, const nh_ContactCache* cache, uint32_t body_count,
                                     const nh_PairList* out, uint32_t flags) {
	if (!ctx || flags || !contacts || !cache || !nh_cp_pairlist_ok(out)) return NH_ERR_INVALID;
	if (contacts->capacity >= 0x80000000u || cache->capacity >= 0x80000000u) return NH_ERR_INVALID;
	if (contacts->capacity && (!contacts->data || !contacts->bodies || !contacts->tags || !contacts->features)) return NH_ERR_INVALID;
	if (cache->capacity && (!cache->tags || !cache->features || !cache->data)) return NH_ERR_INVALID;
	if (((uintptr_t)contacts->data & 15u) || ((uintptr_t)contacts->bodies & 7u) || ((uintptr_t)cache->data & 15u)) return NH_ERR_INVALID;
	{ const int rc = nh_export_views(ctx, NH_VIEW_CONTACTS | NH_VIEW_CACHE); if (rc) return rc; }
	const nh_ContactList in{ contacts->data, contacts->bodies, nullptr, &ctx->d_state->contacts, contacts->capacity, body_count };
	const nh_CpCache look{ contacts->tags, contacts->features, cache->tags, cache->features, reinterpret_cast<const float4*>(cache->data), 0u };
	return nh_cp_pipeline(ctx, in, &look, &ctx->d_state->cache, cache->capacity, out);
}

extern "C" int nh_contact_events(nh_context* ctx, const nh_PairList* prev, const nh_PairList* cur, const nh_PairList* began, const nh_PairList* ended,
                                 uint32_t flags) {
	if (!ctx || flags || !nh_cp_pairlist_ok(cur) || !nh_cp_pairlist_ok(began) || !nh_cp_pairlist_ok(ended) || (prev && !nh_cp_pairlist_ok(prev))) return NH_ERR_INVALID;
	const uint64_t words = (uint64_t)cur->capacity + (prev ? prev->capacity : 0u) + 2u;
	if (words > 0xfffffff0ull) return NH_ERR_INVALID;          // (the scan counts its words in 32 bits)
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	{ const int rc = nh_cp_reserve(ctx, 0u, words); if (rc) return rc; }
	nh_CpState* s = ctx->contact_events;
	const nh_CpPairs C{ cur->count, cur->pairs, cur->capacity }, P{ prev ? prev->count : nullptr, prev ? prev->pairs : nullptr, prev ? prev->capacity : 0u };
	const uint32_t grid = nh_grid_for(words, 256, 1u << 16);
	NH_LAUNCH(ctx, "cp_ev_flag", k_cp_ev_flag, grid, 256, C, P, prev != nullptr, s->ctl, s->scan);
	nh_scan_u32(ctx, s->scan, s->scan, &s->ctl->ev_words, 0u, s->hist, nullptr);
	NH_LAUNCH(ctx, "cp_ev_compact", k_cp_ev_compact, grid, 256, C, P, s->scan, s->ctl, began->count, began->capacity ? began->pairs : (nh_ContactPair*)nullptr,
	          began->capacity, ended->count, ended->capacity ? ended->pairs : (nh_ContactPair*)nullptr, ended->capacity);
	return NH_OK;
}
