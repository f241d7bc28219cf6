// nh_cache.hip -- the impulse cache: the warm-start lookup, the entries kept aside for sleeping pairs, the write-back (reference nudge.cpp:4021-4158),
// and the cache between its two homes -- the caller's arrays in tag order and the slots a still step keeps (nh_internal.h, contact storage by slot).
#include "nh_internal.h"

// ---- read_cached_impulses (nudge.cpp:4021-4108) ------------------------------------------------------------------
// contacts are already in tag order, so the reference's merge-join becomes one binary search per contact.
__global__ __launch_bounds__(256) void k_cache_lookup(const nh_DevState* __restrict__ st, const uint64_t* __restrict__ tags, const uint32_t* __restrict__ features,
                                                      const uint64_t* __restrict__ ctags, const uint32_t* __restrict__ cfeatures, const nh_CachedContactImpulse* __restrict__ cdata,
                                                      nh_CachedContactImpulse* __restrict__ out, const nh_BodyPair* __restrict__ bodies, const uint8_t* __restrict__ body_class) {
	uint32_t n = st->contacts, m = st->cache;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		if (body_class) {
			// only contacts of the >8-contact one-body class and of the level-scheduled path read their warm start from `out`; the
			// fused one-body solver looks its own up and may already have put its SOLVED impulses there
			const nh_BodyPair p = bodies[i];
			const uint32_t ca = p.a ? body_class[p.a] : 0u, cb = p.b ? body_class[p.b] : 0u;
			if (ca != NH_CLS_GENERAL && cb != NH_CLS_GENERAL && ca != NH_CLS_STATICN && cb != NH_CLS_STATICN) continue;
		}
		uint64_t t = tags[i]; uint32_t f = features[i];
		uint32_t lo = 0, hi = m;
		// steady state: the cache is last step's contact list, so the entry usually sits at the same index
		if (i < m && ctags[i] == t && cfeatures[i] == f) { lo = i; hi = i; }
		while (lo < hi) { uint32_t mid = (lo + hi) >> 1; if (tag_less(ctags[mid], cfeatures[mid], t, f)) lo = mid + 1; else hi = mid; }
		nh_CachedContactImpulse r = { { 0.0f, 0.0f, 0.0f }, 0.0f };
		if (lo < m && ctags[lo] == t && cfeatures[lo] == f) r = cdata[lo];
		out[i] = r;
	}
}

// ... over a LIST of contacts: the general ones of a world in which they are few (k_contact_class: `general_list`, st->general_contacts of them) -- two bodies touching among a
// million that rest on the ground cost the lookup 43 us of reading every contact's bodies and classes to find them
__global__ __launch_bounds__(256) void k_cache_lookup_listed(const nh_DevState* __restrict__ st, const uint32_t* __restrict__ list, const uint64_t* __restrict__ tags, const uint32_t* __restrict__ features,
                                                             const uint64_t* __restrict__ ctags, const uint32_t* __restrict__ cfeatures, const nh_CachedContactImpulse* __restrict__ cdata,
                                                             nh_CachedContactImpulse* __restrict__ out) {
	const uint32_t n = st->contacts, m = st->cache, g = st->general_contacts;
	for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < g; j += gridDim.x * blockDim.x) {
		const uint32_t i = list[j];
		if (i >= n) continue;
		const uint64_t t = tags[i]; const uint32_t f = features[i];
		uint32_t lo = 0, hi = m;
		if (i < m && ctags[i] == t && cfeatures[i] == f) { lo = i; hi = i; }
		while (lo < hi) { uint32_t mid = (lo + hi) >> 1; if (tag_less(ctags[mid], cfeatures[mid], t, f)) lo = mid + 1; else hi = mid; }
		nh_CachedContactImpulse r = { { 0.0f, 0.0f, 0.0f }, 0.0f };
		if (lo < m && ctags[lo] == t && cfeatures[lo] == f) r = cdata[lo];
		out[i] = r;
	}
}

// cached impulses of sleeping pairs are kept aside (nudge.cpp:4064-4101)
__global__ __launch_bounds__(256) void k_cull_flags(const nh_DevState* __restrict__ st, const uint64_t* __restrict__ ctags, const uint64_t* __restrict__ sleeping, uint32_t* __restrict__ flags) {
	uint32_t m = st->cache, ns = st->sleeping;
	if (blockIdx.x == 0 && threadIdx.x == 0) flags[m] = 0;       // sentinel so that scan[m] = number of culled entries
	if (ns == 0) return;                                         // nothing sleeps: the scan and the write below are skipped on the device
	for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
		uint64_t t = ctags[j];
		uint32_t lo = 0, hi = ns;
		while (lo < hi) { uint32_t mid = (lo + hi) >> 1; if (sleeping[mid] < t) lo = mid + 1; else hi = mid; }
		flags[j] = (lo < ns && sleeping[lo] == t) ? 1u : 0u;
	}
}

__global__ __launch_bounds__(256) void k_cull_write(const nh_DevState* __restrict__ st, const uint32_t* __restrict__ flags_in, const uint32_t* __restrict__ scan,
                                                    const uint64_t* __restrict__ ctags, const uint32_t* __restrict__ cfeatures, const nh_CachedContactImpulse* __restrict__ cdata,
                                                    uint64_t* __restrict__ otags, uint32_t* __restrict__ ofeatures, nh_CachedContactImpulse* __restrict__ odata) {
	uint32_t m = st->cache;
	if (st->sleeping == 0) return;
	for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
		// flags were scanned in place into `scan`; an entry is culled iff scan[j+1] != scan[j]
		uint32_t p = scan[j], q = scan[j + 1];
		if (q != p) { otags[p] = ctags[j]; ofeatures[p] = cfeatures[j]; odata[p] = cdata[j]; }
		(void)flags_in;
	}
}

// ---- write_cached_impulses (nudge.cpp:4110-4158): merge of two sorted runs by rank -------------------------------
__global__ __launch_bounds__(256) void k_write_cache(nh_DevState* __restrict__ st, const uint64_t* __restrict__ tags, const uint32_t* __restrict__ features, const nh_CachedContactImpulse* __restrict__ imp,
                                                     const uint64_t* __restrict__ ktags, const uint32_t* __restrict__ kfeatures, const nh_CachedContactImpulse* __restrict__ kdata,
                                                     uint64_t* __restrict__ otags, uint32_t* __restrict__ ofeatures, nh_CachedContactImpulse* __restrict__ odata, uint32_t capacity) {
	uint32_t n = st->contacts, m = st->culled;
	uint32_t total = n + m;
	if (total > capacity) { if (blockIdx.x == 0 && threadIdx.x == 0) { st->error = NH_ERR_CACHE_CAPACITY; st->cache = 0; } return; }
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
		if (i < n) {
			// contact i goes after every culled entry with key <= its key ("if (a < b) contact else culled")
			uint64_t t = tags[i]; uint32_t f = features[i];
			uint32_t lo = 0, hi = m;
			while (lo < hi) { uint32_t mid = (lo + hi) >> 1; if (!tag_less(t, f, ktags[mid], kfeatures[mid])) lo = mid + 1; else hi = mid; }
			uint32_t pos = i + lo;
			otags[pos] = t; ofeatures[pos] = f; odata[pos] = imp[i];
		} else {
			uint32_t j = i - n;
			uint64_t t = ktags[j]; uint32_t f = kfeatures[j];
			uint32_t lo = 0, hi = n;
			while (lo < hi) { uint32_t mid = (lo + hi) >> 1; if (tag_less(tags[mid], features[mid], t, f)) lo = mid + 1; else hi = mid; }
			uint32_t pos = j + lo;
			otags[pos] = t; ofeatures[pos] = f; odata[pos] = kdata[j];
		}
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) st->cache = total;
}

// ---- the contact cache between its two homes: the caller's arrays (tag order) and the slots (nh_internal.h, contact storage by slot) ------------------------
// full step -> slots: the solved impulse and feature word of dense contact c go to the raw slot c came from (k_gather_contacts recorded it), every record's count
__global__ __launch_bounds__(256) void k_cache_to_slots(const nh_DevState* __restrict__ st, const uint32_t* __restrict__ dense_slot, const nh_CachedContactImpulse* __restrict__ imp,
                                                        const uint32_t* __restrict__ features, const nh_Record* __restrict__ rec, float4* __restrict__ sc_imp, uint32_t* __restrict__ sc_feat,
                                                        uint32_t* __restrict__ sc_count) {
	const uint32_t n = st->contacts, nrec = st->records;
	for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
		const uint32_t slot = dense_slot[c];
		sc_imp[slot] = *reinterpret_cast<const float4*>(imp + c);
		sc_feat[slot] = features[c];
	}
	for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nrec; r += gridDim.x * blockDim.x) { const uint32_t k = rec[r].count; sc_count[r] = (k & NH_REC_SLEEPING) ? 0u : k; }
}

// entries kept aside for sleeping pairs (the culled arrays of this step's nh_ContactImpulseData: tag order, st->culled of them) -> the slots of the pairs' records.  A
// record is found by its key -- a sleeping record's key is the pair's word, which is what the cache tag equals for every entry that was kept (k_cull_flags) -- in the
// tag order of the layout; an entry's place among its record's slots is its place in the run of equal tags (the entries are ranked by feature word, like the slots' export)
__global__ __launch_bounds__(256) void k_culled_to_slots(const nh_DevState* __restrict__ st, const uint64_t* __restrict__ ctags, const uint32_t* __restrict__ cfeatures,
                                                         const nh_CachedContactImpulse* __restrict__ cdata, const uint64_t* __restrict__ sorted_keys, const uint32_t* __restrict__ sorted_idx,
                                                         const nh_Record* __restrict__ rec, uint32_t pair_cap, float4* __restrict__ sc_imp, uint32_t* __restrict__ sc_feat, uint32_t* __restrict__ sc_count) {
	const uint32_t n = st->culled, nrec = st->records, n_bb = min(st->pairs, pair_cap);
	for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
		const uint64_t t = ctags[j];
		uint32_t k = 0;                                   // place in the run of equal tags
		while (k < 4u && j > k && ctags[j - 1u - k] == t) ++k;
		uint32_t lo = 0, hi = nrec;
		while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (sorted_keys[mid] < t) lo = mid + 1u; else hi = mid; }
		if (lo >= nrec || sorted_keys[lo] != t) continue;
		const uint32_t ri = sorted_idx[lo];
		if (!(rec[ri].count & NH_REC_SLEEPING)) continue;
		const bool sph = ri >= n_bb;
		if (k >= (sph ? 1u : 4u)) continue;
		const uint32_t base = sph ? 4u * n_bb + (ri - n_bb) : 4u * ri;
		sc_imp[base + k] = *reinterpret_cast<const float4*>(cdata + j);
		sc_feat[base + k] = cfeatures[j];
		if (j + 1u >= n || ctags[j + 1u] != t) sc_count[ri] = k + 1u;          // (the last entry of the run knows how many there are)
	}
}

// slots -> the caller's cache arrays, in tag order: counts in tag order (scanned by the host's launch in between), then the entries ranked by feature word
__global__ __launch_bounds__(256) void k_slot_counts_sorted(const nh_DevState* __restrict__ st, const uint32_t* __restrict__ sorted_idx, const uint32_t* __restrict__ sc_count, uint32_t* __restrict__ out) {
	const uint32_t nrec = st->records;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= nrec; i += gridDim.x * blockDim.x) out[i] = i < nrec ? min(sc_count[sorted_idx[i]], 4u) : 0u;
}

__global__ __launch_bounds__(256) void k_slots_to_cache(nh_DevState* __restrict__ st, const uint32_t* __restrict__ sorted_idx, const uint64_t* __restrict__ sorted_keys, const uint32_t* __restrict__ cnt,
                                                        const uint32_t* __restrict__ start, const float4* __restrict__ sc_imp, const uint32_t* __restrict__ sc_feat, uint32_t pair_cap,
                                                        uint64_t* __restrict__ otags, uint32_t* __restrict__ ofeatures, nh_CachedContactImpulse* __restrict__ odata, uint32_t capacity) {
	const uint32_t nrec = st->records, n_bb = min(st->pairs, pair_cap);
	if (blockIdx.x == 0 && threadIdx.x == 0) { const uint32_t total = start[nrec]; if (total > capacity) { st->error = NH_ERR_CACHE_CAPACITY; st->cache = 0u; } else st->cache = total; }
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nrec; i += gridDim.x * blockDim.x) {
		// two dependent round trips: the record's place and count, then its four slots' feature words and impulses at once (a record of a pair with a sphere owns one
		// slot: the other three loads fall into the neighbours' slots and are not used)
		const uint32_t k = min(cnt[i], 4u), ri = sorted_idx[i], first = start[i];
		const uint64_t key = sorted_keys[i];
		const uint32_t base = ri < n_bb ? 4u * ri : 4u * n_bb + (ri - n_bb);
		uint32_t f[4]; float4 w[4];
#pragma unroll
		for (int j = 0; j < 4; ++j) { f[j] = sc_feat[base + j]; w[j] = sc_imp[base + j]; }
		if (!k || first + k > capacity) continue;
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			if ((uint32_t)j < k) {
				uint32_t r = 0;
#pragma unroll
				for (int q = 0; q < 4; ++q) r += ((uint32_t)q < k && (f[q] < f[j] || (f[q] == f[j] && q < j))) ? 1u : 0u;
				otags[first + r] = key; ofeatures[first + r] = f[j];
				*reinterpret_cast<float4*>(odata + first + r) = w[j];
			}
		}
	}
}

// Sleepers form: the slot-cache counts a still narrowphase dropped in a step that did not happen (nh_internal.h: sc_undo) come back.  Called wherever a still step is
// given up -- failed on the device (still_forget_failed), or left by the caller between its nh_collide and its solver (nh_still_abandon) -- BEFORE the slot cache goes
// home to the caller's arrays, which is what the full replay warm-starts from.  Notes of confirmed steps (numbers <= confirmed_seq) are simply cleared.
__global__ __launch_bounds__(256) void k_sleep_undo(uint64_t* __restrict__ sc_undo, uint32_t* __restrict__ sc_count, uint32_t n, uint32_t confirmed_seq) {
	for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
		const uint64_t u = sc_undo[r];
		if (u == 0ull) continue;
		if ((uint32_t)(u >> 32) > confirmed_seq) sc_count[r] = (uint32_t)u;
		sc_undo[r] = 0ull;
	}
}

static nh_ContactImpulseData* new_impulse_data(nh_context* ctx) {
	if (ctx->impulse_ring.empty()) { ctx->impulse_ring.resize(64, nullptr); ctx->constraint_ring.resize(64, nullptr); }
	uint32_t k = ctx->ring_pos % 64;
	if (!ctx->impulse_ring[k]) ctx->impulse_ring[k] = new nh_ContactImpulseData();
	return ctx->impulse_ring[k];
}

// cached impulses of sleeping pairs are kept aside (nudge.cpp:4064-4101); skipped entirely when nothing sleeps (culled = 0 since nh_collide)
void nh_run_cull(nh_context* ctx, nh_ContactImpulseData* d, uint32_t sleeping_on_host) {
	if (!d->cull_pending) return;
	d->cull_pending = false;
	if (sleeping_on_host == 0) return;
	nh_DevState* st = ctx->d_state;
	const uint32_t ccap = d->cache_capacity;
	NH_LAUNCH(ctx, "cull_flags", k_cull_flags, nh_grid_for(ccap, 256, 4096), 256, st, d->ctags, d->sleeping_pairs, d->cull_flags);
	nh_scan_u32(ctx, d->cull_flags, d->cull_flags, &st->cache, 1, d->cull_tmp, &st->culled, &st->sleeping);   // +1: the sentinel, so scan[j+1] exists for every j
	NH_LAUNCH(ctx, "cull_write", k_cull_write, nh_grid_for(ccap, 256, 4096), 256, st, d->cull_flags, d->cull_flags, d->ctags, d->cfeatures, d->cdata,
	          d->culled_tags, d->culled_features, d->culled_data);
}

extern "C" int nh_read_cached_impulses(nh_context* ctx, const nh_ContactCache* cache, const nh_ContactData* contacts, nh_Arena* memory, nh_ContactImpulseData** out) {
	if (!ctx || !cache || !contacts || !memory || !out) return NH_ERR_INVALID;
	{
		// still step: only on the cache and the contact list it was launched for
		const nh_StillStep& ss = ctx->still;
		const bool in_sequence = ss.active && !ss.resolved && !ctx->pending && cache->tags == ss.cache_tags && cache->features == ss.cache_features && cache->data == ss.cache_data &&
		                         cache->capacity == ss.cache_capacity && contacts->data == ss.lay_contacts.data && contacts->tags == ss.lay_contacts.tags;
		int rc = nh_flush_pending(ctx, true, in_sequence); if (rc) return rc;
	}
	const uint32_t kcap = contacts->capacity, ccap = cache->capacity;
	int err = NH_OK;
	ctx->ring_pos++;
	nh_ContactImpulseData* d = new_impulse_data(ctx);
	d->data = nh_arena_array<nh_CachedContactImpulse>(memory, kcap, &err);
	d->culled_tags = nh_arena_array<uint64_t>(memory, ccap, &err);
	d->culled_features = nh_arena_array<uint32_t>(memory, ccap, &err);
	d->culled_data = nh_arena_array<nh_CachedContactImpulse>(memory, ccap, &err);
	d->capacity = kcap; d->culled_capacity = ccap;
	// culling of cached impulses of sleeping pairs (nudge.cpp:4064-4101) only has work when something sleeps; the scratch for it is
	// reserved here, the kernels run once the host knows the sleeping-pair count (nh_run_cull)
	d->cull_flags = nh_arena_array<uint32_t>(memory, ccap + 1, &err);
	d->cull_tmp = nh_arena_array<uint32_t>(memory, 2 * NH_SORT_GRID + 64, &err);
	if (err) return err;
	// the per-contact lookup is deferred: bodies on the one-body path fetch their impulses inside the fused solver kernel, and
	// nh_materialize_lookup() fills d->data for everything else (only if such contacts exist, which setup learns)
	d->lookup_pending = true; d->ctx = ctx; d->consumed = false;
	d->tags = contacts->tags; d->features = contacts->features;
	d->ctags = cache->tags; d->cfeatures = cache->features; d->cdata = cache->data;
	d->cull_pending = contacts->sleeping_pairs != nullptr;
	d->sleeping_pairs = contacts->sleeping_pairs;
	d->cache_capacity = ccap;
	if (d->cull_pending && (ctx->flags & NH_FLAG_SYNC_COUNTS)) {
		// reference semantics: nh_collide has just synchronised, the count is on the host
		nh_run_cull(ctx, d, ctx->h_state->sleeping);
	}
	*out = d;
	return NH_OK;
}

// `bodies` / `body_class` given: restrict to the contacts that read their warm start from d->data (see k_cache_lookup)
// (`general_list`, `general`: the contacts that read their warm start from d->data are the listed general ones and nothing else -- no body of the rare many-contact class -- and
// they are few: the lookup walks the list)
void nh_materialize_lookup(nh_context* ctx, nh_ContactImpulseData* d, const nh_BodyPair* bodies, const uint8_t* body_class, const uint32_t* general_list, uint32_t general) {
	if (!d->lookup_pending) return;
	d->lookup_pending = false;
	if (general_list && general != 0u && (uint64_t)general * 16u < d->capacity && !ctx->no_listed_lookup) {
		NH_LAUNCH(ctx, "cache_lookup_listed", k_cache_lookup_listed, nh_grid_for(general, 256, 4096), 256, ctx->d_state, general_list, d->tags, d->features, d->ctags, d->cfeatures, d->cdata, d->data);
		return;
	}
	NH_LAUNCH(ctx, "cache_lookup", k_cache_lookup, nh_grid_for(d->capacity, 256, 16384), 256, ctx->d_state, d->tags, d->features, d->ctags, d->cfeatures, d->cdata, d->data, bodies, body_class);
}

extern "C" const nh_CachedContactImpulse* nh_contact_impulses_device(const nh_ContactImpulseData* d) {
	if (!d) return nullptr;
	nh_ContactImpulseData* m = const_cast<nh_ContactImpulseData*>(d);
	if (m->ctx) {
		// before the solver has run this holds the warm-start impulses, afterwards the solved ones: make either visible
		if (m->ctx->pending) nh_flush_pending(m->ctx);
		else if (!m->consumed) nh_materialize_lookup(m->ctx, m);
		nh_StillStep& ss = m->ctx->still;
		if (ss.active && ss.resolved && m->consumed && m->cdata == ss.cache_data) {
			// a still step: the solved impulses live in the slot cache; in tag order they are what the exported cache holds (nothing is culled in a still step)
			if (nh_still_sync_outputs(m->ctx, NH_VIEW_CACHE) == NH_OK)
				hipMemcpyAsync(m->data, ss.cache.data, sizeof(nh_CachedContactImpulse) * (size_t)(m->capacity < ss.cache.capacity ? m->capacity : ss.cache.capacity), hipMemcpyDeviceToDevice, m->ctx->stream);
		}
	}
	return d->data;
}

extern "C" int nh_write_cached_impulses(nh_context* ctx, nh_ContactCache* cache, const nh_ContactData* contacts, nh_ContactImpulseData* imp) {
	if (!ctx || !cache || !contacts || !imp) return NH_ERR_INVALID;
	{ int rc = nh_flush_pending(ctx); if (rc) return rc; }
	{
		nh_StillStep& ss = ctx->still;
		// a still step that went through: the solver has written every contact's impulse into its cache entry, tags and features are last step's -- nothing to do
		if (ss.active && ss.resolved && cache->data == ss.cache_data && imp->ctx == ctx && imp->consumed) return NH_OK;
		// a full step: afterwards the cache IS this step's contact list when nothing was culled (the round trip has told) -- what the next still step relies on
		// (sleepers form: entries kept aside for sleeping pairs are part of such a cache -- they go to the slots of their records below)
		ss.cache_ok = imp->consumed && !imp->cull_pending && !(ctx->flags & NH_FLAG_SYNC_COUNTS) && ((ctx->h_state->sleeping == 0u && ctx->h_state->culled == 0u) || !ss.no_local) &&
		              contacts->data == ss.lay_contacts.data && contacts->tags == ss.lay_contacts.tags;
		ss.cache_tags = cache->tags; ss.cache_features = cache->features; ss.cache_data = cache->data; ss.cache_capacity = cache->capacity;
		ss.cache = *cache;
		ss.slots_current = false;
	}
	if (!imp->consumed) nh_materialize_lookup(ctx, imp);      // no setup ran on this handle: the cache is rewritten from the looked-up impulses
	if (imp->cull_pending) {
		nh_Counts c;
		int rc = nh_read_counts(ctx, &c);
		if (rc) return rc;
		nh_run_cull(ctx, imp, c.sleeping_pairs);
	}
	nh_DevState* st = ctx->d_state;
	NH_LAUNCH(ctx, "write_cache", k_write_cache, nh_grid_for((uint64_t)contacts->capacity + cache->capacity, 256, 4096), 256, st,
	          contacts->tags, contacts->features, imp->data, imp->culled_tags, imp->culled_features, imp->culled_data,
	          cache->tags, cache->features, cache->data, cache->capacity);
	if (ctx->still.ok_next && ctx->still.cache_ok && !ctx->still.disabled && (ctx->flags & NH_FLAG_FUSED_STEP) && ctx->sort_seeded) {
		// the next step may be a still one: the cache goes to the slots as well (solved impulse + feature word to the raw slot each contact came from)
		NH_LAUNCH(ctx, "cache_to_slots", k_cache_to_slots, nh_grid_for(contacts->capacity, 256, 4096), 256, st, ctx->dense_slot, imp->data, contacts->features, ctx->rec,
		          ctx->sc_imp, ctx->sc_feat, ctx->sc_count);
		// (the entries kept aside for sleeping pairs, nudge.cpp:4064-4101: to the slots of the pairs' records -- a step in sleepers form keeps them there)
		// (the host's mirror knows the step's sleeping pairs from the round trip; how many entries were kept aside is counted on the device after it: the kernel reads that)
		if (ctx->h_state->sleeping)
			NH_LAUNCH(ctx, "culled_to_slots", k_culled_to_slots, nh_grid_for(imp->culled_capacity, 256, 2048), 256, st, imp->culled_tags, imp->culled_features, imp->culled_data, ctx->sort_sorted_keys,
			          ctx->sort_sorted_idx, ctx->rec, ctx->lay_capacity, ctx->sc_imp, ctx->sc_feat, ctx->sc_count);
		ctx->still.slots_current = true;
	}
	if (ctx->flags & NH_FLAG_SYNC_COUNTS) {
		nh_Counts c;
		int rc = nh_read_counts(ctx, &c);
		if (rc) return rc;
		cache->count = c.cache;
		if (c.error) return (int)c.error;
	}
	return NH_OK;
}

int nh_still_undo_drops(nh_context* ctx) {
	nh_StillStep& ss = ctx->still;
	if (!ss.undo_dirty || !ctx->sc_undo || !ctx->lay_capacity) return NH_OK;
	ss.undo_dirty = false;
	NH_LAUNCH(ctx, "sleep_undo", k_sleep_undo, nh_grid_for(ctx->lay_capacity, 256, 2048), 256, ctx->sc_undo, ctx->sc_count, ctx->lay_capacity, ss.confirmed_seq);
	return NH_OK;
}

int nh_still_export_cache(nh_context* ctx) {
	nh_StillStep& ss = ctx->still;
	if (!ss.cache_stale) return NH_OK;
	ss.cache_stale = false;
	nh_DevState* st = ctx->d_state;
	const uint32_t P = ctx->lay_capacity;
	// (scratch: the tag-order starts of the dense VIEW are this step's -- a failed still step may already have overwritten them -- so the cache gets its own scan;
	// dense_slot is free between two full steps)
	uint32_t* tmp_cnt = ctx->exp_cnt; uint32_t* tmp_start = ctx->exp_start;
	NH_LAUNCH(ctx, "slot_counts", k_slot_counts_sorted, nh_grid_for(P, 256, 2048), 256, st, ctx->sort_sorted_idx, ctx->sc_count, tmp_cnt);
	nh_scan_u32(ctx, tmp_cnt, tmp_start, &st->records, 1, ctx->exp_scan_tmp, nullptr);
	NH_LAUNCH(ctx, "slots_to_cache", k_slots_to_cache, nh_grid_for(P, 256, 4096), 256, st, ctx->sort_sorted_idx, ctx->sort_sorted_keys, tmp_cnt, tmp_start, ctx->sc_imp, ctx->sc_feat, P,
	          ss.cache.tags, ss.cache.features, ss.cache.data, ss.cache.capacity);
	return NH_OK;
}
