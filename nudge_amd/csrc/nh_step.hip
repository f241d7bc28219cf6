// nh_step.hip -- nh_step, the sample's sub-step loop as one entry point, with the verdicts of its still steps; and the views a still step owes the caller
// (nh_export_views: dense contact list, cache, active list, sleeping pairs).
#include "nh_internal.h"
#include <atomic>
#include <chrono>
#include <string.h>

// LOCAL speculation (nh_internal.h): every round trip -- a full step's, a still step's verdict -- tells whether somebody left its inflated box in that step; the
// movers form of the still step stays on for 16 steps after the last one who did
void nh_still_note_movers(nh_context* ctx, const nh_DevState* h, uint32_t seq) {          // `seq`: the nh_collide the counters belong to (0: a full step's round trip)
	nh_StillStep& ss = ctx->still;
	// (a still step in sleepers form that found NOBODY awake: the next step is a full one -- two of those in a row start the asleep steps, which cost nothing)
	if (ss.sleepers && h->active == 0u) ss.ok_next = false;
	// (sleepers ahead: how long has the sleeping set stood still?  Counted over confirmed still steps -- `seq` != 0 -- by the active count they report)
	if (seq != 0u) { if (h->active == ss.sleep_last_active) { if (ss.sleep_stable < 0xffffu) ss.sleep_stable++; } else { ss.sleep_stable = 0u; ss.sleep_last_active = h->active; } }
	// (... counted by k_pair_owned in the nh_collide numbered pair_owned_seq: counters of an earlier step, or of a full step -- which voids the count -- say nothing)
	if (ss.pair_owned_seq != 0u && seq >= ss.pair_owned_seq) { if (h->pair_unowned > ctx->pair_list_capacity) ss.pair_world_bad = true; else { ss.pair_world_ok = true; ss.pair_listed = h->pair_unowned; } }         // (pair ahead: some kept pair is nobody's -- k_pair_owned; the step that relied on it has failed itself)
	if (h->ahead_multi) ss.ahead_world_bad = true;          // (xform ahead: some body carries several colliders -- k_ahead_check; the step that relied on the map has failed itself)
	if (h->fat_inserts != ss.seen_inserts) ss.movers_left = 16u;
	else if (ss.movers_left) ss.movers_left--;
	ss.seen_inserts = h->fat_inserts; ss.seen_rebuilds = h->fat_rebuilds;
}

// ---- views of a world with sleepers (nh_internal.h, "SLEEPERS form"): the list of sleeping pairs and the active list, as a full step would have written them -------
__global__ __launch_bounds__(256) void k_view_sleep_keys(const nh_DevState* __restrict__ st, const nh_Record* __restrict__ rec, const uint64_t* __restrict__ rec_key, uint64_t* __restrict__ out) {
	const uint32_t n = st->records;
	for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) out[r] = (rec[r].count & NH_REC_SLEEPING) ? rec_key[r] : ~0ull;      // (a sleeping record carries the pair's word)
}
__global__ __launch_bounds__(256) void k_view_sleep_copy(nh_DevState* __restrict__ st, const uint64_t* __restrict__ sorted, uint64_t* __restrict__ out, uint32_t capacity) {
	const uint32_t n = st->sleeping;
	if (n > capacity) { if (blockIdx.x == 0 && threadIdx.x == 0) st->error = NH_ERR_CONTACT_CAPACITY; return; }
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = sorted[i];
}
__global__ __launch_bounds__(256) void k_view_awake_flags(const uint8_t* __restrict__ awake, uint32_t nbodies, uint32_t* __restrict__ flags) {
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= nbodies; i += gridDim.x * blockDim.x) flags[i] = (i >= 1u && i < nbodies && awake[i]) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_view_active_write(nh_DevState* __restrict__ st, const uint8_t* __restrict__ awake, const uint32_t* __restrict__ scan, uint32_t nbodies,
                                                           uint32_t* __restrict__ indices, uint32_t capacity) {
	for (uint32_t i = 1u + blockIdx.x * blockDim.x + threadIdx.x; i < nbodies; i += gridDim.x * blockDim.x) {
		if (!awake[i]) continue;
		const uint32_t at = scan[i];
		if (at < capacity) indices[at] = i; else st->error = NH_ERR_ACTIVE_CAPACITY;
	}
}

static int still_view_sleepers(nh_context* ctx, uint32_t what) {
	nh_StillStep& ss = ctx->still;
	nh_DevState* st = ctx->d_state;
	if (what & NH_VIEW_CONTACTS) {
		// sleeping pairs in ascending order (nudge.cpp:4008): the words of the sleeping records, sorted -- every other record sorts behind them
		const uint32_t P = ctx->lay_capacity;
		if (ss.lay_contacts.sleeping_pairs) {
			if (ctx->exp_sleep_capacity < P) {
				ctx->exp_sleep_capacity = 0;
				{ int rc = nh_device_buffers(ctx, { { &ctx->exp_sleep_a, sizeof(uint64_t) * (size_t)P + 64u }, { &ctx->exp_sleep_b, sizeof(uint64_t) * (size_t)P + 64u },
				                                    { &ctx->exp_sleep_hist, sizeof(uint32_t) * (256u * NH_SORT_GRID + 512u) } }); if (rc) return rc; }
				ctx->exp_sleep_capacity = P;
			}
			NH_LAUNCH(ctx, "view_sleep_keys", k_view_sleep_keys, nh_grid_for(P, 256, 2048), 256, st, ctx->rec, ctx->sort_keys_by_position, ctx->exp_sleep_a);
			uint64_t* a = ctx->exp_sleep_a; uint64_t* b = ctx->exp_sleep_b;
			int bits = (int)ctx->tag_bits; if (bits < 1) bits = 1; if (bits > 32) bits = 32;
			const int top = ((bits + 7) / 8) * 8;
			if (nh_sort_u64(ctx, a, b, &st->records, ctx->exp_sleep_hist, 0, top)) { uint64_t* t = a; a = b; b = t; }
			if (nh_sort_u64(ctx, a, b, &st->records, ctx->exp_sleep_hist, 32, 32 + top)) { uint64_t* t = a; a = b; b = t; }
			NH_LAUNCH(ctx, "view_sleep_copy", k_view_sleep_copy, nh_grid_for(P, 256, 1024), 256, st, a, ss.lay_contacts.sleeping_pairs, ss.lay_contacts.capacity);
		}
	}
	if ((what & NH_VIEW_ACTIVE) && ss.lay_active && ctx->still_awake) {
		const uint32_t B = ss.lay_bodies.count;
		if (ctx->exp_flags_capacity < B + 2u) {
			ctx->exp_flags_capacity = 0;
			{ int rc = nh_device_buffers(ctx, { { &ctx->exp_flags, sizeof(uint32_t) * ((size_t)B + 66u) } }); if (rc) return rc; }
			ctx->exp_flags_capacity = B + 2u;
		}
		NH_LAUNCH(ctx, "view_awake_flags", k_view_awake_flags, nh_grid_for(B, 256, 2048), 256, ctx->still_awake, B, ctx->exp_flags);
		nh_scan_u32(ctx, ctx->exp_flags, ctx->exp_flags, &st->pad0 /* always 0 */, B, ctx->exp_scan_tmp, nullptr);
		NH_LAUNCH(ctx, "view_active_write", k_view_active_write, nh_grid_for(B, 256, 2048), 256, st, ctx->still_awake, ctx->exp_flags, B, const_cast<uint32_t*>(ss.lay_active), ss.lay_active_capacity);
	}
	return NH_OK;
}

int nh_still_sync_outputs(nh_context* ctx, uint32_t what) {
	nh_StillStep& ss = ctx->still;
	if (ss.active && !ss.resolved) return NH_OK;          // (an unconfirmed still step is abandoned by the caller first: nh_flush_pending)
	int rc = NH_OK;
	if (what & NH_VIEW_CACHE) rc = nh_still_export_cache(ctx);
	if (rc) return rc;
	if ((what & NH_VIEW_CONTACTS) && ss.contacts_stale) { ss.contacts_stale = false; rc = nh_still_view_contacts(ctx); if (!rc && ss.views_sleepers) rc = still_view_sleepers(ctx, NH_VIEW_CONTACTS); ss.sleep_pairs_current = true; }
	else if ((what & NH_VIEW_CONTACTS) && ss.views_sleepers && !ss.sleep_pairs_current) { rc = still_view_sleepers(ctx, NH_VIEW_CONTACTS); ss.sleep_pairs_current = true; }
	if (rc) return rc;
	if ((what & NH_VIEW_ACTIVE) && ss.views_sleepers && !ss.active_current) { rc = still_view_sleepers(ctx, NH_VIEW_ACTIVE); ss.active_current = true; }
	return rc;
}

extern "C" int nh_export_views(nh_context* ctx, uint32_t what) {
	if (!ctx || (what & ~(uint32_t)NH_VIEW_ALL)) return NH_ERR_INVALID;          // (NH_VIEW_ALL = contacts | cache | active)
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	{ int rc = nh_flush_pending(ctx, true); if (rc) return rc; }
	return nh_still_sync_outputs(ctx, what);
}

// ---- nh_step: the sample's sub-step loop (example/main.cpp:274-328) as one entry point ----------------------------------------------------------------------
// The eight calls, `steps` times.  Besides sparing the caller eight crossings of the ABI per step, the library -- driving the call order itself -- may look at a still
// step's verdict one step late (nh_internal.h: nh_StillStep::pipelined), so that neither the host nor the GPU ever waits for the other inside the loop; a failed
// still step and the one launched behind it (both did nothing) are simply run again.  On return every step is confirmed.
// A still step that reports itself (nh_solve.hip: nh_FusedStep::host_counters) leaves its counters and, behind them, its number in the pinned ring slot as its solver STARTS --
// everything a still step can fail on was decided by then -- and NO event is recorded behind that solver (nh_StillStep::verdict.event): the host spins on the number,
// acquires, and reads the counters from the slot.  A launch that never ran writes no number: every 256 spins the host looks at the clock, and once the wait has lasted
// longer than any healthy step of a small world (2 ms) at the stream as well -- not before: a query puts a packet of its own behind the launch the host has just
// enqueued (measured: with a query every 256 spins the 5.9 us gap behind the solver is back, profiles/r10_steady_step_ab.log); a step longer than 2 ms pays at most that one.  0 = the number is there; 1 = the stream has drained and one more look did not find it; 2 = the runtime reports an error (ctx->last_hip_error).
int nh_still_await_number(nh_context* ctx) {
	nh_StillStep& ss = ctx->still;
	volatile const uint32_t* const flag = reinterpret_cast<volatile const uint32_t*>(ss.h_ring[ss.verdict.slot]) + NH_COUNTER_WORDS;
	std::chrono::steady_clock::time_point t0;
	for (uint32_t spins = 0; ; ++spins) {
		if (*flag == ss.verdict.seq) break;
		if ((spins & 255u) == 255u) {
			const auto now = std::chrono::steady_clock::now();
			if (spins == 255u) t0 = now;
			else if (now - t0 > std::chrono::milliseconds(2)) {
				const hipError_t q = hipStreamQuery(ctx->stream);
				if (q == hipSuccess) { if (*flag == ss.verdict.seq) break; return 1; }
				if (q != hipErrorNotReady) { ctx->last_hip_error = (int)q; return 2; }
			}
		}
		__builtin_ia32_pause();
	}
	std::atomic_thread_fence(std::memory_order_acquire);
	ctx->early_reads++;
	return 0;
}

int nh_still_verdict_now(nh_context* ctx) {
	// the pending verdict, waited for: 0 confirmed, 1 failed, 2 the runtime reports an error (ctx->last_hip_error)
	nh_StillStep& ss = ctx->still;
	if (!ss.verdict.pending) return 0;
	const nh_DevState* h = ss.h_ring[ss.verdict.slot];
	if (ss.verdict.event) {
		// (a counter copy by the runtime, the halo split or option "no_early_counts": the event behind the solver says the slot is complete)
		const hipError_t e = hipEventSynchronize(ss.ev_ring[ss.verdict.slot]);
		if (e != hipSuccess) { ss.verdict.pending = false; ctx->last_hip_error = (int)e; return 2; }
	} else {
		const int w = nh_still_await_number(ctx);
		if (w) { ss.verdict.pending = false; return w; }
	}
	ss.verdict.pending = false;
	if (h->still_failed_seq >= ss.verdict.seq || h->error) return 1;
	ss.confirmed_seq = ss.verdict.seq;
	memcpy(ctx->h_state, h, NH_COUNTER_WORDS * sizeof(uint32_t));
	if (!ctx->idle_unknown) { ctx->idle_bound = (int)h->max_idle[ss.verdict.parity]; ctx->idle_bound_mark = ss.verdict.collide_mark; }
	nh_still_note_movers(ctx, h, ss.verdict.seq);
	return 0;
}

// after a failed still step: nothing of it (or of the step launched behind it) has happened; the next nh_collide is a full one
static int still_forget_failed(nh_context* ctx, bool advanced, uint32_t voided) {
	nh_StillStep& ss = ctx->still;
	ss.verdict.pending = false;
	ss.active = false; ss.resolved = false; ss.setup_d = nullptr; ss.ok_next = false; ss.ahead_ready = false; ss.own_current = false;
	ss.note_failure();
	if (ss.sleepers) {
		// (sleepers ahead: somebody fell asleep, most likely.  One sleeper now and then costs the form eight steps; failures in quick succession -- a world dozing off in a
		// trickle -- double that up to 64)
		if (ss.sleep_backoff_len < 8u || ss.sleep_run >= 32u) ss.sleep_backoff_len = 8u; else if (ss.sleep_backoff_len < 64u) ss.sleep_backoff_len *= 2u;
		ss.sleep_backoff = ss.sleep_backoff_len; ss.sleep_stable = 0u; ss.sleep_run = 0u;
	}
	ss.failed += voided;                               // (still steps launched that did not happen: the failed one, and the one launched behind it if it got that far)
	ctx->pending = nullptr;
	ctx->grav.pending = false; ctx->grav.rest_pending = false; ctx->adv.done = false;
	ctx->after_collide = false; ctx->gravity_may_overlap = false;
	if (advanced && ctx->advance_count) ctx->advance_count--;          // (the failed step's nh_advance was counted: the sleep prediction counts real ones)
	if (advanced) nh_stream_void_advance(ctx);          // (... and so does the state stream; a frame taken at that nh_advance shows the state BEFORE the step: it is withdrawn)
	{ int rc = nh_still_undo_drops(ctx); if (rc) return rc; }          // (sleepers form: slot-cache counts the voided steps' narrowphases dropped)
	return nh_still_export_cache(ctx);                                 // (the slot cache holds the last step that DID happen: the full solver reads the caller's arrays)
}

static bool same_bodies_arrays(const nh_BodyData& a, const nh_BodyData& b) {
	return a.transforms == b.transforms && a.properties == b.properties && a.momentum == b.momentum && a.idle_counters == b.idle_counters && a.count == b.count;
}
static bool same_collider_arrays(const nh_ColliderData& a, const nh_ColliderData& b) {
	return a.boxes.tags == b.boxes.tags && a.boxes.data == b.boxes.data && a.boxes.transforms == b.boxes.transforms && a.boxes.count == b.boxes.count &&
	       a.spheres.tags == b.spheres.tags && a.spheres.data == b.spheres.data && a.spheres.transforms == b.spheres.transforms && a.spheres.count == b.spheres.count;
}

extern "C" int nh_step(nh_context* ctx, const nh_StepArgs* a, uint32_t steps) {
	if (!ctx || !a || !a->active_bodies || !a->contacts || !a->bodies || !a->colliders || !a->contact_cache) return NH_ERR_INVALID;
	NH_HIP_CHECK(ctx, hipSetDevice(ctx->device));
	nh_StillStep& ss = ctx->still;
	if (!ss.h_ring[0] && !ss.ring_failed) {
		for (int k = 0; k < 2; ++k) {
			if (hipHostMalloc((void**)&ss.h_ring[k], sizeof(nh_DevState), 0) != hipSuccess || hipEventCreateWithFlags(&ss.ev_ring[k], hipEventDisableTiming) != hipSuccess) { ss.ring_failed = true; break; }
			memset(ss.h_ring[k], 0, sizeof(nh_DevState));
		}
		if (ss.ring_failed) {
			// whatever was created goes back, both slots end empty, and the loop runs with the verdict inside every step from now on (no retry per call)
			for (int k = 0; k < 2; ++k) {
				if (ss.h_ring[k]) { (void)hipHostFree(ss.h_ring[k]); ss.h_ring[k] = nullptr; }
				if (ss.ev_ring[k]) { (void)hipEventDestroy(ss.ev_ring[k]); ss.ev_ring[k] = nullptr; }
			}
		}
	}
	// (per-kernel timing of EVERY launch collects its events at the step's round trip; timing restricted to one kernel -- nh_set_timing_filter: two events per step, what
	// bench.py keeps on during its timed region -- leaves the loop as it is: the events are collected when the call's last verdict has been waited for)
	ss.pipelined = ss.h_ring[0] != nullptr && (ctx->flags & NH_FLAG_FUSED_STEP) && !(ctx->flags & (NH_FLAG_SYNC_COUNTS | NH_FLAG_EXACT_ORDER)) && !ss.disabled &&
	               !(ctx->timing && ctx->timing_filter.empty()) &&
	               !ctx->step_hook;          // (nh_partition_step: what a step sends to the neighbours must be a step that HAPPENED -- its verdict is looked at inside the step)
	ss.verdict.pending = false;
	ss.ahead_map_ok = false; ss.ahead_ready = false;          // (xform ahead, nh_internal.h: nothing carries over from another call -- the caller may have changed anything in between)
	int result = NH_OK;
	uint32_t i = 0;
	while (i < steps || ss.verdict.pending) {
		if (i >= steps) {
			// the last step's verdict, waited for; a failure sends the loop back one step
			const int v = nh_still_verdict_now(ctx);
			if (v == 0) break;
			if (v == 2) { result = NH_ERR_HIP; break; }
			{ int rc = still_forget_failed(ctx, true, 1u); if (rc) { result = rc; break; } }
			i -= 1;
			continue;
		}
		// A world asleep (nh_internal.h: nh_AsleepState): two full steps in a row were its fixed point.  ONE check per call that nothing the caller owns has changed since
		// -- and the remaining steps of this call are done: nothing inside the library wakes a world in which nobody is awake.
		// (never inside nh_partition_step: the neighbours expect this rank's halo before every sub-step, whether anything moves here or not)
		if (ctx->asleep.streak >= 2u && !ctx->asleep.disabled && !ctx->step_hook && !ss.verdict.pending && !ctx->pending && (ctx->flags & NH_FLAG_FUSED_STEP) && !(ctx->flags & NH_FLAG_SYNC_COUNTS) && !ctx->timing &&
		    same_bodies_arrays(*a->bodies, ss.lay_bodies) && same_collider_arrays(*a->colliders, ss.lay_colliders) && a->contacts->data == ss.lay_contacts.data && a->contacts->tags == ss.lay_contacts.tags &&
		    a->contacts->sleeping_pairs == ss.lay_contacts.sleeping_pairs && a->active_bodies->indices == ss.lay_active && a->contact_cache->data == ss.cache_data && a->contact_cache->tags == ss.cache_tags && a->contact_cache->features == ss.cache_features) {
			const int v = nh_asleep_verify(ctx, a->bodies, a->colliders);
			if (v < 0) { result = -v; break; }
			if (v == 0) { ss.sleep_backoff = ss.sleep_backoff > steps - i ? ss.sleep_backoff - (steps - i) : 0u; ctx->asleep.steps += steps - i; if (ctx->stream_state.every) ctx->stream_state.advances += steps - i; i = steps; continue; }          // (no frames: nothing moves)
			ctx->asleep.streak = 0;
		}
		int rc;
		if (ctx->step_hook && (rc = ctx->step_hook(ctx, ctx->step_hook_user, i))) { result = rc; break; }
		ss.more_steps = i + 1u < steps; ss.steps_left = steps - 1u - i; ss.substep = i;
		nh_Arena temporary = a->arena;
		nh_ContactImpulseData* imp = nullptr;
		nh_ContactConstraintData* con = nullptr;
		if ((rc = nh_collide(ctx, a->active_bodies, a->contacts, a->bodies, a->colliders, a->body_connections, temporary)) ||
		    (rc = nh_apply_gravity_damping(ctx, a->active_bodies, a->bodies, a->time_step, a->gravity, a->damping_rate)) ||
		    (rc = nh_read_cached_impulses(ctx, a->contact_cache, a->contacts, &temporary, &imp)) ||
		    (rc = nh_setup_contact_constraints(ctx, a->active_bodies, a->contacts, a->bodies, imp, &temporary, &con)) ||
		    (rc = nh_apply_impulses(ctx, con, a->bodies, a->iterations))) {
			if (rc == NH_INTERNAL_STILL_FAILED && i > 0) {
				// the still step before this one failed: neither it nor this one has happened
				{ int rc2 = still_forget_failed(ctx, true, ctx->still.active ? 2u : 1u); if (rc2) { result = rc2; break; } }
				i -= 1;
				continue;
			}
			result = rc == NH_INTERNAL_STILL_FAILED ? NH_ERR_INVALID : rc;
			break;
		}
		if ((rc = nh_update_cached_impulses(ctx, con, imp)) || (rc = nh_write_cached_impulses(ctx, a->contact_cache, a->contacts, imp)) ||
		    (rc = nh_advance(ctx, a->active_bodies, a->bodies, a->time_step))) { result = rc; break; }
		++i;
	}
	ss.pipelined = false; ss.more_steps = false; ss.ahead_ready = false; ss.ahead_map_ok = false; ss.steps_left = 0u; ss.substep = 0u; ss.own_current = false;
	if (result && ss.verdict.pending) { if (ss.verdict.event) hipEventSynchronize(ss.ev_ring[ss.verdict.slot]); else hipStreamSynchronize(ctx->stream); ss.verdict.pending = false; }          // (no event behind a solver that reports itself: the stream)
	return result;
}
