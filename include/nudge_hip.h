/*
 * nudge_hip.h -- C ABI of the MI355X-native stepping engine (libnudge_hip.so).
 *
 * This is the drop-in boundary for the hot path of rasmusbarr/nudge:
 *     collide -> [gravity] -> read_cached_impulses -> setup_contact_constraints
 *             -> apply_impulses x N -> update_cached_impulses -> write_cached_impulses -> advance
 * Each entry point below replaces the reference function cited next to it (reference nudge.h:134-146,
 * implemented in reference nudge.cpp:3000-4926) and keeps its argument meaning.  Differences, all forced
 * by the device boundary or by scale, are:
 *
 *   1. Every array pointer inside the structs is DEVICE memory (hipMalloc'ed by the caller, or carved out
 *      of a torch tensor): the caller still owns every array; per-step scratch and the device side of the
 *      two opaque result objects come out of the caller's `nh_Arena` (device memory) with
 *      the reference's bump semantics (nudge.h:29-32, nudge.cpp:990-1055): `nh_collide` takes the arena
 *      BY VALUE (scratch is dead on return), the two `Arena*` functions ADVANCE it.
 *      What the library DOES allocate itself (hipMalloc, freed by nh_destroy; all of it state that must survive from one
 *      step to the next, which the by-value arena cannot hold): the counter block (~5 KB device + a pinned host mirror);
 *      per body 4 B of warm-start hint and 16 B of contact degree / adjacency bookkeeping (grown to the largest
 *      `bodies->count` seen); the splitters and bucket counters of the tag sort (16 B per 1024 broadphase pairs of
 *      capacity); the broadphase's kept pair list (16 B per pair of pair capacity: twice the capacity in 8-byte pairs) and one
 *      inflated box per collider (32 B) -- nh_collide re-tests the kept pairs instead of searching the grid while no collider
 *      has left its box, and re-inserts the few that have (new box, new pairs) from the grid of its last search, which it keeps as well:
 *      per collider 32 B of cell-sorted boxes + 9 B of book-keeping, 4 B per grid cell (4 cells per collider, 2^16 .. 2^24); the contact records' keys by position and the tag order of the last sort (20 B per pair of capacity) --
 *      the sort is skipped while no record changes its key; a side stream and two events; two small host-side rings of opaque-object descriptors.
 *   2. Indices are widened: body indices and collider tags are 32-bit (the reference packs them in 16 bits:
 *      nudge.h:68-71, 86, 93, 126 and asserts <= 8192 colliders at nudge.cpp:3010).  A contact's identity
 *      is therefore split in two words: `tags[i]`  = a_tag | (uint64_t)b_tag << 32   (reference: high 32
 *      bits of its u64 tag, a16 | b16 << 16) and `features[i]` = the reference's low 32 feature bits.
 *      Ordering everywhere is the reference's: by b_tag, then a_tag, then feature.
 *   3. Functions return an error code (NH_OK = 0) instead of assert()-aborting (nudge.cpp:1000, 3010, 4118).
 *   4. Counts are produced on the device.  With NH_FLAG_SYNC_COUNTS (default) the host-visible `count`
 *      fields are filled in before the call returns, as in the reference; without it the calls only enqueue
 *      work on the context's stream and `nh_read_counts` fetches the numbers when the host wants them.
 *   5. `contacts->data/bodies/tags/features` are returned in TAG ORDER (the order the reference's solver
 *      consumes them in, nudge.cpp:4027-4044), not in narrowphase emission order: same set, canonical order.
 *   6. The caller-side gravity/damping loop of the sample app (example/main.cpp:290-305) runs over
 *      host-invisible memory here, so it is offered as `nh_apply_gravity_damping`.
 *   7. Deferred execution.  `nh_read_cached_impulses` and `nh_setup_contact_constraints` may postpone part of their
 *      work (the per-contact cache lookup; row build + warm start of bodies that only touch the static world) and
 *      run it fused with the first `nh_apply_impulses`, so that a constraint row lives only in registers; the one host
 *      round trip of a step (device counters) is also taken there, behind the solver kernel it has just launched.  Every
 *      entry point of this library that reads or writes momentum, impulses or counters first completes pending
 *      work, and so does `nh_synchronize`: through the API the reference's call-by-call semantics are kept.  Only
 *      foreign kernels enqueued on the stream BETWEEN setup and the first apply would see momentum without the
 *      warm start; call `nh_synchronize` (or any entry point) first if you need that.
 *
 *   8. The solver consumes the contact list as nh_collide laid it out (tag order, per-body degrees, adjacency seeds).
 *      Contacts appended by the caller after nh_collide (the reference allows that: "Custom contacts can be added here",
 *      example/main.cpp:287) are announced with `nh_append_contacts`, which merges them into that order and counts the per-body
 *      bookkeeping again; fields of existing contacts (friction, penetration ...) may simply be edited in place.
 *      One nh_setup_contact_constraints per nh_collide (a second one returns NH_ERR_STALE_SETUP).
 *
 *   9. Still steps (NH_FLAG_FUSED_STEP without NH_FLAG_SYNC_COUNTS / NH_FLAG_EXACT_ORDER).  A world at rest on static geometry repeats itself: the same pairs at
 *      the same places of the kept pair list, the same tag order, nearly the same contacts.  When a step ended in that state the library launches the NEXT one
 *      speculatively as a "still" step: transforms + AABBs, the narrowphase straight from the kept pair list into the pairs' own contact slots (library-owned),
 *      the fused solver reading those slots and a slot-indexed copy of the warm-start cache -- three kernels that CHECK everything they rely on (nobody outside
 *      its inflated box or asleep, every collider pair with the key it had, at most four contacts per body, all of them against the inert static world) instead
 *      of the ~25 launches that would find it out again.  A pair that gains or loses a contact is listed and the places of the contacts behind it shift (the
 *      solver order of nudge.cpp:4206-4339 is a function of a contact's dense tag-order index, which stays exact).  A failed check is reported with the step's
 *      one host round trip before anything irreversible has been written, and the step is run again in full from nh_collide's arguments: results are
 *      bit-identical to a library that never speculates (option "no_still"), which the tests check.
 *      Since round 5 two of those checks no longer fail the step (LOCAL speculation; option "no_local_still" restores them): a small collider outside its inflated box is
 *      given a new box and re-inserted into the kept pair list by the step itself (its pair with the ground it left keeps its record: taking off, flying and coming down
 *      again are still steps), and a body asleep in a set of its own (no overlapping AABB of another dynamic body, no user connections in the world) is left alone -- its
 *      pairs are sleeping pairs, its cached impulses are kept aside by the reference's rule (nudge.cpp:3669-3703, 4064-4101).  What still ends in a full step: a first
 *      contact with a collider the body was not resting on, two dynamic bodies touching, sets of several bodies with a sleeper among them, a rebuild of the kept list.
 *      Inside ONE nh_step call -- where the caller cannot touch anything between two sub-steps -- a still step in which nobody moves and nobody can be asleep also does
 *      the next sub-step's first kernel ("xform ahead"; option "no_xform_ahead"): the solver lane that has just advanced a body writes its collider's world transform
 *      and AABB, tests it against the inflated box and gathers the scene bounds, so that the next sub-step starts at the narrowphase; what the lane finds wanting fails
 *      THAT sub-step, which is run again in full.  Only for worlds whose dynamic bodies carry one collider each (checked on the device once per call).
 *      nh_Counts.ahead_steps counts the sub-steps that started that way.  (Round 6: the lane also evaluates its body's own collider pair for the next sub-step -- "pair ahead",
 *      nh_Counts.pair_steps: such a sub-step starts at the solver -- and while the set of sleeping bodies stands still a world WITH sleepers is stepped the same way, its
 *      sleepers part of the static world for those sub-steps ("sleepers ahead"; options "no_pair_ahead", "no_sleeper_ahead").)
 *      The caller's dense contact list (contacts->data / bodies / tags / features, contacts->sleeping_pairs), active list and contact cache are VIEWS under this regime: they are
 *      brought up to date by nh_export_views (what: NH_VIEW_CONTACTS, NH_VIEW_CACHE, NH_VIEW_ACTIVE), by nh_append_contacts, and by any step that does not qualify -- not by
 *      every step, and not by the cheap observers: nh_read_counts returns the counters and nh_synchronize waits for the stream, neither exports anything (the
 *      sample reads active_bodies.count every sub-step, example/main.cpp:293: that must not cost two passes over the contacts).  Call nh_export_views and then
 *      nh_synchronize before reading the arrays from the device yourself.  (BREAKING for hosts written against rounds 1-4, where nh_synchronize / nh_read_counts
 *      exported the views: nh_set_option(ctx, "sync_exports_views", 1) restores that contract at its old price; INTEGRATION.md.)  Any entry point outside the sample's
 *      call order between nh_collide and nh_apply_impulses turns a still step into a full one first, so everything it observes is what a full step
 *      produces.  nh_Counts.still_steps / still_replays count them.
 *      The scene queries (nh_query_build, nh_query_refit, nh_raycast, nh_spherecast, nh_raycast_all, nh_spherecast_all, nh_boxcast_all, nh_capsulecast_all, nh_raycast_k, nh_spherecast_k, nh_boxcast_k, nh_capsulecast_k, nh_boxcast, nh_capsulecast, nh_overlap, nh_penetration, nh_overlap_wide, nh_penetration_wide, nh_region, nh_sense, nh_sense_rays, nh_sweep, nh_closest, nh_closest_k, nh_distance, nh_move, nh_recover, nh_walk, nh_boxmove, nh_boxwalk, nh_move_touched, nh_boxmove_touched, nh_walk_touched, nh_boxwalk_touched, nh_query_set_layers, nh_query_filter, nh_query_layer_info) are not entry points of the step in this sense: they neither export nor settle nor turn a still step into a
 *      full one, and they do not count -- see "scene queries" below.
 *      nh_body_impulses and nh_sweep_limit WRITE momentum from outside the step: they complete pending work first and, without NH_IMPULSE_WAKE, leave speculation to
 *      the checks above -- see "body impulses" and "fast bodies" below.
 *      nh_joints_setup and nh_joints_apply ARE entry points of the step in this sense: they complete pending work, and a pending still step becomes a full one
 *      first -- see "joints" below.  nh_joints_prepare and nh_joint_connections touch nothing of the step.
 *
 * Threading: one context = one HIP stream = one world at a time; no global mutable state.
 */
#ifndef NUDGE_HIP_H
#define NUDGE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes ------------------------------------------------------------------------------- */
enum {
	NH_OK = 0,
	NH_ERR_INVALID = 1,          /* bad argument */
	NH_ERR_NO_DEVICE = 2,        /* no HIP device / runtime error */
	NH_ERR_ARENA = 3,            /* arena exhausted            (reference: assert nudge.cpp:1000-1039) */
	NH_ERR_CONTACT_CAPACITY = 4, /* contacts->capacity exceeded (reference: unchecked overflow)         */
	NH_ERR_CACHE_CAPACITY = 5,   /* contact_cache->capacity     (reference: assert nudge.cpp:4118)      */
	NH_ERR_ACTIVE_CAPACITY = 6,  /* active_bodies->capacity     (reference: unchecked overflow)         */
	NH_ERR_PAIR_CAPACITY = 7,    /* broadphase pair buffer: nh_set_pair_capacity (default contacts->capacity / 2 + 1024;
	                                AABB-overlap pairs can outnumber contacts in dense scenes: size it from the colliders) */
	NH_ERR_HIP = 8,              /* a HIP call failed; see nh_last_hip_error                            */
	NH_ERR_SCHEDULER_CAPACITY = 9, /* NH_FLAG_EXACT_ORDER only: the replay of the reference's greedy batch scheduler ran out of open
	                                batches (more than ~130,000 contacts on ONE dynamic body; the reference sizes this by
	                                contacts.count, nudge.cpp:4222-4223)                                  */
	NH_ERR_STALE_HINT = 11,      /* idle_counters were changed behind the library's back (see nh_bodies_changed): a body was asleep in a step
	                                for which the host had ruled that out                                 */
	NH_ERR_STALE_SETUP = 10      /* nh_setup_contact_constraints called twice for one nh_collide, or contacts->count changed in
	                                between: the solver's inputs are laid out by nh_collide (note 8)         */
};

/* ---- context flags ----------------------------------------------------------------------------- */
enum {
	NH_FLAG_SYNC_COUNTS = 1u,    /* fill host-side count fields before returning (reference semantics)   */
	NH_FLAG_SINGLE_APPLY = 4u,   /* the caller promises ONE nh_apply_impulses(..., iterations) per nh_setup_contact_constraints (the whole
	                                iteration loop of example/main.cpp:313-318 in one call): the per-contact solver states that only a
	                                further nh_apply_impulses call would read are then not written (16 B per contact per step); a
	                                second call for the same setup returns NH_ERR_INVALID.  Entry points that complete a deferred setup
	                                before the first apply (nh_read_counts, nh_synchronize ...) keep the states: the apply after them works */
	NH_FLAG_FUSED_STEP = 8u,     /* implies NH_FLAG_SINGLE_APPLY.  The caller promises the call order of the sample's step (example/main.cpp:286-330):
	                                nh_collide, nh_apply_gravity_damping(dt), nh_read_cached_impulses, nh_setup_contact_constraints, one
	                                nh_apply_impulses, nh_update_cached_impulses, nh_write_cached_impulses, nh_advance(dt), and does not touch body
	                                state in between.  Gravity / damping and the advance of the bodies whose only contacts are with the inert
	                                static world then happen inside their solver kernel (same arithmetic, two passes over the body state less);
	                                every other body goes through the ordinary kernels.  Any other entry point in between settles the pending
	                                gravity first; nh_advance with a different time step than gravity was given returns NH_ERR_INVALID -- a broken
	                                promise, found after the solver has moved its bodies by gravity's step: do not continue that world       */
	NH_FLAG_EXACT_ORDER = 2u     /* solver visits contacts in the reference's greedy batch order, replayed
	                                exactly on the device (nudge.cpp:4206-4339); default is the closed-form
	                                round-robin order, identical whenever the greedy scheduler meets no
	                                lane conflict (drop scenes)                                            */
};

/* ---- POD records: layouts identical to reference nudge.h unless marked (wide) -------------------- */
typedef struct nh_Arena { void* data; uintptr_t size; } nh_Arena;                                   /* nudge.h:29-32 */
typedef struct nh_Transform { float position[3]; uint32_t body; float rotation[4]; } nh_Transform;   /* nudge.h:34-38 */
typedef struct nh_BodyProperties { float inertia_inverse[3]; float mass_inverse; } nh_BodyProperties;/* nudge.h:40-43 */
typedef struct nh_BodyMomentum { float velocity[3]; float unused0; float angular_velocity[3]; float unused1; } nh_BodyMomentum; /* nudge.h:45-50 */
typedef struct nh_SphereCollider { float radius; } nh_SphereCollider;                                /* nudge.h:52-54 */
typedef struct nh_BoxCollider { float size[3]; float unused; } nh_BoxCollider;                       /* nudge.h:56-59 */
typedef struct nh_Contact { float position[3]; float penetration; float normal[3]; float friction; } nh_Contact; /* nudge.h:61-66 */
typedef struct nh_BodyPair { uint32_t a; uint32_t b; } nh_BodyPair;                                  /* nudge.h:68-71 (wide) */
typedef struct nh_CachedContactImpulse { float impulse[3]; float unused; } nh_CachedContactImpulse;  /* nudge.h:113-116 */
/* (`unused`: zero, as in the reference, under NH_FLAG_EXACT_ORDER; in the default solver order the library keeps the contact's
   colour of the last sweep there -- an integer bit pattern, never read as a number -- to warm-start the next step's colouring) */

typedef struct nh_ContactData {                                                                      /* nudge.h:73-82 (wide) */
	nh_Contact* data;
	nh_BodyPair* bodies;
	uint64_t* tags;            /* a_tag | b_tag << 32 */
	uint32_t* features;        /* feature word (reference: low 32 bits of the tag) */
	uint32_t capacity;
	uint32_t count;
	uint64_t* sleeping_pairs;  /* tag | tag << 32, ascending: pairs of sleeping sets dropped before the narrowphase carry the larger tag low
	                              (nudge.cpp:3697), pairs of sleeping contact islands the order of their contact tags (nudge.cpp:3979) */
	uint32_t sleeping_count;
} nh_ContactData;

typedef struct nh_ColliderData {                                                                     /* nudge.h:84-98 (wide tags) */
	struct { uint32_t* tags; nh_BoxCollider* data; nh_Transform* transforms; uint32_t count; } boxes;
	struct { uint32_t* tags; nh_SphereCollider* data; nh_Transform* transforms; uint32_t count; } spheres;
} nh_ColliderData;

typedef struct nh_BodyData {                                                                         /* nudge.h:100-106 */
	nh_Transform* transforms;
	nh_BodyProperties* properties;
	nh_BodyMomentum* momentum;
	uint8_t* idle_counters;
	uint32_t count;
} nh_BodyData;

typedef struct nh_BodyConnections { nh_BodyPair* data; uint32_t count; } nh_BodyConnections;         /* nudge.h:108-111 */

typedef struct nh_ContactCache {                                                                     /* nudge.h:118-123 (wide) */
	uint64_t* tags;
	uint32_t* features;
	nh_CachedContactImpulse* data;
	uint32_t capacity;
	uint32_t count;
} nh_ContactCache;

typedef struct nh_ActiveBodies { uint32_t* indices; uint32_t capacity; uint32_t count; } nh_ActiveBodies; /* nudge.h:125-129 (wide) */

typedef struct nh_ContactImpulseData nh_ContactImpulseData;         /* nudge.h:131, opaque */
typedef struct nh_ContactConstraintData nh_ContactConstraintData;   /* nudge.h:132, opaque */
typedef struct nh_context nh_context;

/* Device-side counters of the most recent step, mirrored to the host by nh_read_counts.  (Fields are only ever added at the END; a caller built against an
   older header must be recompiled: nh_read_counts fills the whole struct.) */
typedef struct nh_Counts {
	uint32_t colliders;         /* C */
	uint32_t pairs;             /* P: broadphase pairs surviving the same-body / sleeping filters */
	uint32_t contacts;          /* K */
	uint32_t sleeping_pairs;
	uint32_t active_bodies;
	uint32_t cache;             /* entries in the contact cache after the last write */
	uint32_t culled;            /* cached impulses kept aside for sleeping pairs */
	uint32_t large_colliders;   /* colliders handled by the brute-force "large x all" broadphase pass */
	uint32_t general_contacts;  /* contacts solved by the level-scheduled path (not the one-body fast path) */
	uint32_t levels;            /* dependency levels of that path */
	uint32_t error;             /* NH_* raised on the device (capacity overflows) */
	uint32_t has_other_bodies;  /* non-zero: some body is outside the one-body fast path's common class (several pairs, dynamic partners, no contacts) */
	uint32_t unleveled;         /* internal: progress of the level relaxation */
	uint32_t raw_pairs;         /* broadphase pairs before any filter (diagnostic) */
	uint32_t broadphase_rebuilds; /* nh_collide calls since nh_create that regrouped the colliders and searched the grid; the others re-used the kept pair list */
	uint32_t sort_reuses;       /* nh_collide calls since nh_create that skipped the tag sort of the contact records: every record sat where it sat the step
	                               before, with the same key */
	uint32_t broadphase_inserts; /* colliders that left their inflated box and were re-inserted into the kept pair list (new box, new pairs) without a rebuild,
	                               since nh_create */
	uint32_t still_steps;       /* steps since nh_create that went through as STILL steps (note 9): launched as a world whose contact layout is last step's, and confirmed */
	uint32_t still_replays;     /* ... launched as one, found otherwise (by the device or because the caller left the sample's call order) and run again in full */
	uint32_t still_diff[4];     /* what still steps have found changed, summed since nh_create: collider pairs with another key / another contact count / other feature words;
	                               colliders outside their inflated box or bodies asleep (diagnostic) */
	uint32_t blk_blocks, blk_bodies, blk_ghosts;   /* the blocked solver's tables of the last step that built them (large general sets): blocks of the grid, general bodies binned,
	                               ghost copies borrowed by blocks (a sweep loads and stores blk_bodies + blk_ghosts momentum records); diagnostic / measurement */
	uint32_t asleep_steps;      /* steps since nh_create that nh_step found to be steps of a world in which every body is asleep and nothing has changed: done without a launch */
	uint32_t ahead_steps;       /* still steps (launched, since nh_create) that started at the narrowphase: the solver of the sub-step before them, inside the same nh_step call, had
	                               already written their colliders' world transforms and boxes (note 9, "xform ahead") */
	uint32_t fused_steps;       /* always 0: the one-kernel still step was removed (the word keeps the struct's layout) */
	uint32_t pair_steps;        /* still steps that started at the SOLVER: the solver lanes of the sub-step before them had evaluated every body's own collider pair for them as well
	                               (note 9, "pair ahead") -- a step of ONE launch behind a one-workgroup prologue */
	uint32_t pair_diag[4];      /* why such steps were refused, summed since nh_create: which collider plays "a" could not be told without the next scene frame / the record was not the
	                               lane's to evaluate (another key, a fifth contact, a partner that is not the static world) / the next frame's cells came out too large / some kept pair
	                               belongs to no body (diagnostic) */
} nh_Counts;

/* ---- lifecycle ---------------------------------------------------------------------------------- */
/* `stream` is a hipStream_t (or NULL for the default stream) on `device`; the context never creates one. */
int nh_create(nh_context** out, int device, void* stream, uint32_t flags);
void nh_destroy(nh_context* ctx);
int nh_set_flags(nh_context* ctx, uint32_t flags);
int nh_synchronize(nh_context* ctx);                         /* completes deferred work and waits for the stream; exports no view (note 9) */
int nh_read_counts(nh_context* ctx, nh_Counts* out);        /* synchronises the stream; exports no view (note 9) */
/* The caller's views of what still steps keep by slot (note 9), brought up to date on the context's stream: NH_VIEW_CONTACTS = contacts->data / bodies / tags /
   features in tag order, NH_VIEW_CACHE = the nh_ContactCache arrays (tags, features, data; nh_Counts.cache).  A no-op (two host-side flag tests) when the arrays
   are current -- after a full step they always are.  Replaces the reference's implicit guarantee that both arrays are current when collide() /
   write_cached_impulses() return (nudge.cpp:4009, 4158) for callers that read them from the device themselves. */
enum { NH_VIEW_CONTACTS = 1u /* + contacts->sleeping_pairs */, NH_VIEW_CACHE = 2u, NH_VIEW_ACTIVE = 4u /* active_bodies->indices */, NH_VIEW_ALL = 7u };
int nh_export_views(nh_context* ctx, uint32_t what);
int nh_set_cache_count(nh_context* ctx, uint32_t count);    /* restore a checkpointed ContactCache */
/* Tell the library that the caller has written `idle_counters` itself (initial upload excepted: a fresh context assumes nothing).  The
   library predicts on the host when a body can first be asleep -- counters rise by at most one per nh_advance -- and launches none of the
   island / sleeping kernels before that; counters written from outside invalidate the prediction until the next nh_collide has looked at
   them.  A forgotten call is detected on the device and reported as NH_ERR_STALE_HINT, never silently wrong. */
int nh_bodies_changed(nh_context* ctx);
int nh_set_tag_bits(nh_context* ctx, uint32_t bits);        /* collider tags are < 2^bits (default 32): fewer sort passes */
/* Capacity of the broadphase pair buffer (AABB-overlap pairs after the same-body filter), carved from the arena at ~210 B per
   pair by nh_collide.  0 (default) = contacts->capacity / 2 + 1024.  The reference has no such limit (its pair list lives in the
   arena too, nudge.cpp:3473): dense scenes hold more overlapping pairs than contacts (a settled ball pit: 1.7 x), so size it from
   the collider count there.  Overflow is reported as NH_ERR_PAIR_CAPACITY. */
int nh_set_pair_capacity(nh_context* ctx, uint32_t pairs);
/* Diagnostic switches for A/B runs and tests -- none is needed in production, each selects an older, slower or more talkative path; the library never reads the
   environment.  Names (value 0 / 1 unless noted): "no_still", "no_kept_pairs", "no_incremental", "no_sort_reuse", "sort_radix", "bucket_tile" (n),
   "bucket_target" (n), "colour_check_seeds", "no_resident", "no_blocks", "blk_check", "blk_min" (n), "blk_target" (n), "blk_rows_global", "blk_global_colours",
   "blk_profile", "no_asleep", "no_blk_chain", "no_local_still", "no_xform_ahead",
   "no_pair_ahead", "no_sleeper_skip", "no_sleeper_ahead", "no_early_counts", "no_listed_lookup", "halo_overlap" (1 = on), "sync_exports_views".  Unknown name: NH_ERR_INVALID.  Call right after nh_create.
   "no_early_counts": the host takes no counters from a solver's first thread -- a full step's by a copy behind its solver, and inside nh_step an event is recorded behind
   every still solver and waited for (the ring event), where by default the host spins on the number that solver leaves in pinned memory as it starts.
   (nudge_amd/engine.py maps environment variables NH_<NAME> onto these calls for its tests: a convenience of that host, not of the library.) */
int nh_set_option(nh_context* ctx, const char* name, int value);
const char* nh_error_string(int code);
int nh_last_hip_error(nh_context* ctx);

/* ---- the hot path: one entry point per reference function ------------------------------------------ */
/* collide (nudge.h:134, nudge.cpp:3000-4009) */
int nh_collide(nh_context* ctx, nh_ActiveBodies* active_bodies, nh_ContactData* contacts,
               const nh_BodyData* bodies, const nh_ColliderData* colliders,
               const nh_BodyConnections* body_connections, nh_Arena temporary);

/* Custom contacts (example/main.cpp:287: "Custom contacts can be added here").  The caller has written `extra` complete contacts -- data, bodies,
   tags (a_tag | b_tag << 32: any pair of tags that no collider pair produces), features -- behind the list nh_collide returned, at indices
   [count, count + extra) of the arrays of `contacts` (device memory; without NH_FLAG_SYNC_COUNTS `count` is what nh_read_counts reports).  Call this
   after nh_collide and before nh_read_cached_impulses: the contacts are merged into tag order (the order the reference's solver consumes,
   nudge.cpp:4027-4044, 4172) and the per-body bookkeeping is counted again; the contact count grows by `extra` (contacts->count too under
   NH_FLAG_SYNC_COUNTS).  `positions` (device memory, count + extra words, or NULL): where every contact of the list as the caller left it -- the
   old ones, then the appended ones -- now sits.  `temporary`: scratch (~60 bytes per contact of capacity).  At most 65,536 contacts per call.
   Like in the reference, contacts appended here take no part in the sleeping islands nh_collide has already formed. */
int nh_append_contacts(nh_context* ctx, nh_ContactData* contacts, const nh_BodyData* bodies, uint32_t extra, uint32_t* positions, nh_Arena temporary);

/* caller-side loop of the sample app (example/main.cpp:290-305): v -= g*dt; v,w *= 1 - dt*damping_rate */
int nh_apply_gravity_damping(nh_context* ctx, const nh_ActiveBodies* active_bodies, const nh_BodyData* bodies,
                             float time_step, const float gravity[3], float damping_rate);

/* read_cached_impulses (nudge.h:136, nudge.cpp:4021-4108) */
int nh_read_cached_impulses(nh_context* ctx, const nh_ContactCache* contact_cache, const nh_ContactData* contacts,
                            nh_Arena* memory, nh_ContactImpulseData** out);

/* write_cached_impulses (nudge.h:138, nudge.cpp:4110-4158) */
int nh_write_cached_impulses(nh_context* ctx, nh_ContactCache* contact_cache, const nh_ContactData* contacts,
                             nh_ContactImpulseData* contact_impulses);

/* setup_contact_constraints (nudge.h:140, nudge.cpp:4170-4638) */
int nh_setup_contact_constraints(nh_context* ctx, const nh_ActiveBodies* active_bodies, const nh_ContactData* contacts,
                                 const nh_BodyData* bodies, nh_ContactImpulseData* contact_impulses,
                                 nh_Arena* memory, nh_ContactConstraintData** out);

/* apply_impulses (nudge.h:142, nudge.cpp:4640-4855): `iterations` consecutive calls of the reference */
int nh_apply_impulses(nh_context* ctx, nh_ContactConstraintData* data, const nh_BodyData* bodies, uint32_t iterations);

/* update_cached_impulses (nudge.h:144, nudge.cpp:4857-4884) */
int nh_update_cached_impulses(nh_context* ctx, nh_ContactConstraintData* data, nh_ContactImpulseData* contact_impulses);

/* advance (nudge.h:146, nudge.cpp:4886-4926) */
int nh_advance(nh_context* ctx, const nh_ActiveBodies* active_bodies, const nh_BodyData* bodies, float time_step);

/* ---- multi-GPU helpers (nudge_amd/partition.py): the per-step halo record of a body ---------------------- */
/* record = transform.position (12 B) | transform.rotation (16 B) | momentum (32 B) | idle counter (1 B) + 3 B pad = 64 B.
   nh_halo_pack gathers the records of the bodies listed in `indices` (device memory) into `out` (device memory, count x 64 B);
   nh_halo_unpack writes `count` records into the consecutive body slots first_slot .. first_slot+count-1 (the `body` field of
   their transforms -- unused by the engine for bodies, nudge.h:36 -- is left alone).  Transport between the two is the host's
   business (RCCL send/recv). */
#define NH_HALO_RECORD_BYTES 64
int nh_halo_pack(nh_context* ctx, const nh_BodyData* bodies, const uint32_t* indices, uint32_t count, void* out);
int nh_halo_unpack(nh_context* ctx, const nh_BodyData* bodies, uint32_t first_slot, uint32_t count, const void* in);
/* nh_halo_update: nh_halo_unpack for records of the SAME bodies that already occupy those slots, as their owner stepped them since the last exchange (the
   per-step halo; nh_halo_unpack is for slots that change hands: refresh, migration).  The difference is the library's sleep prediction (see
   nh_bodies_changed): idle counters rise by at most one per step on the owner as they do here, so an update does not invalidate it. */
int nh_halo_update(nh_context* ctx, const nh_BodyData* bodies, uint32_t first_slot, uint32_t count, const void* in);

/* ---- the sample's sub-step loop as ONE entry point (example/main.cpp:274-328: simulate()) ---------------------------------------------------------------------
   nh_step(ctx, args, steps) = `steps` times  nh_collide, nh_apply_gravity_damping, nh_read_cached_impulses, nh_setup_contact_constraints, nh_apply_impulses(iterations),
   nh_update_cached_impulses, nh_write_cached_impulses, nh_advance  on the arrays of `args` (scratch and the two opaque objects come out of `arena`, reset every step like
   the sample does, example/main.cpp:282).  Same results as the eight calls made by the caller -- bit for bit -- with two savings: one crossing of the ABI instead of
   eight per step, and, because the library drives the call order itself, the host round trip of a still step (note 9) is taken one step LATE, so that neither the host nor
   the GPU waits for the other inside the loop.  Every step is confirmed when the call returns.  Custom contacts / user impulses between the calls need the eight calls.
   A world in which EVERY body is asleep is a fixed point of the step (no active body, no contact, every overlapping pair a sleeping pair, the cache kept aside and
   written back as it was: nudge.cpp:3669-3703, 4064-4101, 4896-4898).  Once two full steps in a row have shown that, nh_step checks once per call -- one kernel: every
   collider's world AABB and tag what they were, every body still asleep -- that nothing the caller owns has changed, and takes the steps of the call as done
   (nh_Counts.asleep_steps); anything else runs them in full.  Results are those of a library that never does this (option "no_asleep"), which the tests check. */
typedef struct nh_StepArgs {
	nh_ActiveBodies* active_bodies; nh_ContactData* contacts; const nh_BodyData* bodies; const nh_ColliderData* colliders; const nh_BodyConnections* body_connections;
	nh_ContactCache* contact_cache; nh_Arena arena;
	float time_step; float gravity[3]; float damping_rate; uint32_t iterations;
} nh_StepArgs;
int nh_step(nh_context* ctx, const nh_StepArgs* args, uint32_t steps);

/* ---- state streaming: the GL-free viewer hook (the sample redraws from bodies.transforms after simulate(), example/main.cpp:176-272, 330) -------------------------
   A viewer, a recorder or a network peer wants body transforms on the HOST every few steps without stopping the world.  nh_stream_state arms that: every `every`-th
   nh_advance (the end of a sub-step, whoever drives the eight calls) the transforms of the first `count` bodies are copied device-to-device into a library-owned staging
   buffer on the context's stream (tens of microseconds at a million bodies, ordered behind the step that produced them) and from there, on the library's side stream,
   into slot (frame mod slots) of the caller's ring -- the world's stream never waits for the host link.  A frame whose predecessor is still on its way to the host is
   dropped, not queued (nh_StreamInfo.dropped).  Ring layout: `slots` frames of count x sizeof(nh_Transform) bytes, back to back; give it pinned memory (hipHostMalloc)
   or the copies are staged by the runtime.  nh_stream_latest: the newest frame that has LANDED (never blocks): its slot, and the number of nh_advance calls (since
   nh_stream_state) it shows.  every = 0 disarms.  Reference counterpart: none needed -- its arrays are host memory. */
typedef struct nh_StreamInfo { uint32_t slot; uint32_t valid; uint64_t step; uint64_t frames, dropped; } nh_StreamInfo;
int nh_stream_state(nh_context* ctx, const nh_BodyData* bodies, uint32_t count, void* host_ring, uint32_t slots, uint32_t every);
int nh_stream_latest(nh_context* ctx, nh_StreamInfo* out);

/* ---- scene queries: ray casts, sphere, box and capsule casts, all-hits casts, overlaps and closest points against the device-resident world ---------------------------------------------
   nh_query_build snapshots the world transforms and AABBs of ALL box and sphere colliders -- those of sleeping bodies and of body 0 (the static world) included -- and
   builds a bounding-volume hierarchy over them (a linear BVH: Morton keys, a radix tree, bottom-up boxes) into buffers the library owns: they grow with the collider
   count (~190 B per collider) and are freed by nh_destroy.  nh_raycast answers `count` rays (nh_overlap, below, `count` shapes) against the LAST build: the hierarchy does not follow the bodies by itself, so
   after they have moved (after nh_step / nh_advance) call nh_query_refit (below: the same tree, today's boxes) or rebuild before casting against the new positions;
   wherever this header says "the LAST nh_query_build", a later nh_query_refit counts.  All pointers are DEVICE memory; both calls only enqueue work
   on the context's stream, like every other entry point (read the hits after nh_synchronize or a stream / event wait of your own).
   Semantics (nudge_amd/csrc/nh_query.h):
     - closest hit = the smallest t with 0 <= t <= max_t, over the colliders not belonging to `ignore_body` (0xffffffff: none is ignored); ties are broken by
       (shape, collider index) ascending, so the answer does not depend on the tree -- a brute force over all colliders gives the same bits;
     - `direction` need not be unit length: t is in units of it;
     - an origin inside a collider hits it at t = 0 with normal = -d / |d|;
     - a miss writes shape = NH_SHAPE_NONE, t = max_t, normal = 0 and body = collider = tag = 0xffffffff;
     - NH_RAY_ANY_HIT may stop at the first hit it finds (shadow / visibility rays): hit or miss agrees with the closest-hit answer and a reported hit is a real one
       with t <= max_t, but which hit is unspecified;
     - a ray with a non-finite origin or direction cannot be refused by the return code of an asynchronous call: its record is written as a miss with t = NaN.
   nh_raycast returns NH_ERR_INVALID before any nh_query_build and for null or not 16-byte aligned `rays` / `hits`; count = 0 is a no-op that returns NH_OK.
   QUERIES ARE OBSERVERS (note 9): no query call exports a view, settles deferred gravity, turns a still step into a full one or touches nh_Counts.  Made between any two
   entry points, or between two nh_step calls, they leave every later step bit-identical, with the same still_steps / still_replays / ahead_steps / pair_steps /
   asleep_steps.  They read bodies->transforms as the stream has them at that point: under NH_FLAG_FUSED_STEP the fused solver advances part of the bodies inside
   nh_apply_impulses, so a build between nh_apply_impulses and nh_advance sees a world half advanced -- build after nh_advance (or nh_step) for a consistent one.
   Not built: queries on a partitioned world (nh_partition_*). */
typedef struct nh_Ray { float origin[3]; float max_t; float direction[3]; uint32_t ignore_body; } nh_Ray;                                            /* 32 B */
typedef struct nh_RayHit { float t; float normal[3]; uint32_t body; uint32_t collider; uint32_t shape; uint32_t tag; } nh_RayHit;                     /* 32 B */
enum { NH_SHAPE_BOX = 0u, NH_SHAPE_SPHERE = 1u, NH_SHAPE_CAPSULE = 2u, NH_SHAPE_NONE = 0xffffffffu };    /* nh_RayHit.shape; NONE = miss.  CAPSULE is a QUERY
                                                                                                       shape only (nh_OverlapQuery.shape): never in
                                                                                                       nh_RayHit.shape or nh_OverlapHit.shape */
enum { NH_RAY_ANY_HIT = 1u };
int nh_query_build(nh_context* ctx, const nh_BodyData* bodies, const nh_ColliderData* colliders);
int nh_raycast(nh_context* ctx, const nh_Ray* rays, uint32_t count, nh_RayHit* hits, uint32_t flags);

/* nh_query_refit: the hierarchy of the last nh_query_build, made current -- the per-step call of a character controller, a camera or a sensor that casts every step.
   It keeps the leaf order, the tree's links, the sorted keys and the key frame of that build, and re-reads EVERYTHING else from the arrays it is given: body and
   collider transforms, shapes, tags, the collider -> body mapping.  Every collider record, every leaf box (the build's arithmetic and pad) and every internal box is
   rewritten.
   CONTRACT: after nh_query_refit(ctx, b, c) every query call writes exactly the bytes it writes after nh_query_build(ctx, b, c) on the same arrays -- for
   NH_RAY_ANY_HIT the same hit-or-miss, which is all that flag promises.  Only the TIME the queries take may differ: the tree keeps the topology of the last BUILD, so
   its boxes loosen as bodies move away from where they were sorted (nh_closest's Morton seed then looks among the keys of that build; it only proposes real colliders
   that are evaluated exactly).  Measured at 1,004,524 colliders on one MI355X
   (profiles/refit_rates.log): a refit takes 0.23 ms where a build takes 0.60 ms (0.42 and 1.1 full steps of that world); after 70 steps of free fall and landing
   the refitted tree answered 1 M incoherent rays at 1.00x and 1 M unbounded nh_closest queries at 1.00x the rate of a fresh one -- a lattice that falls straight
   down keeps its order; bodies that travel across the scene will loosen the tree faster, and the caller rebuilds when its own query times say so.
   Returns NH_ERR_INVALID for null arguments, before any nh_query_build, when boxes.count or spheres.count differs from the last build's (the leaf order is by
   combined collider index: another count is another world -- rebuild), and for the null arrays nh_query_build refuses.  Zero colliders: NH_OK, nothing launched.
   Never allocates, never waits.  An OBSERVER like the build (note 9): only launches on the context's stream; it leaves the bounds the next build accumulates alone,
   so a build after any number of refits is the build it would have been without them.
   nh_query_stats (diagnostic; WAITS for the stream): of the last build's tree, the collider count, the length and number of the leaf runs the box pass cuts it into,
   the number of nodes that cross a run boundary (the pass's second, single-workgroup phase) and the height of the tree those nodes form. */
typedef struct nh_QueryStats { uint32_t colliders, run_length, runs, top_nodes, top_depth; } nh_QueryStats;
int nh_query_refit(nh_context* ctx, const nh_BodyData* bodies, const nh_ColliderData* colliders);
int nh_query_stats(nh_context* ctx, nh_QueryStats* out);

/* ---- layer masks: per-collider layers, per-query masks -- what a query may see ------------------------------------------------------------------------------
   A camera ray that must not stop at trigger volumes, a character hull that sweeps against the static world but not against debris, a lidar that does not
   see its own vehicle, an explosion overlap that wants dynamic bodies only: every collider carries one 32-bit word of LAYER bits, every query a MASK, and
   collider c is seen by a query with mask m if and only if (layers[c] & m) != 0.  The filter sits inside the walk of the hierarchy: each node carries the
   OR of the words of the leaves below it, so a subtree that holds nothing a query may see is skipped whole -- a ray that only cares about the ground does
   not walk through a million boxes.
   LAYERS.  Until nh_query_set_layers is called every collider's word is 0xffffffff.  nh_query_set_layers copies boxes.count / spheres.count words (the
   counts of the LAST nh_query_build) from DEVICE memory into storage the library owns, by combined collider index (boxes, then spheres), and computes the
   node words (2 n - 1 words; nothing is added to the hierarchy's nodes or records); the caller's arrays are free once the call returns -- the copy is
   enqueued on the context's stream like everything else, so "free" means free to be overwritten by later work on that stream.  One NULL array: all ones
   for that shape.  Both NULL: the layers are forgotten (every word is 0xffffffff again).  A later nh_query_build with the SAME two counts keeps the
   collider words and recomputes the node words over the new tree (the layers follow the collider index, not the leaf); a build with other counts forgets
   them -- another count is another world, nh_query_refit's rule.  nh_query_refit keeps the topology and with it the node words: it launches nothing new
   and costs what it costs without layers.  With no layers set, build and refit launch exactly what they launch without this section.
   Returns NH_ERR_INVALID before any nh_query_build and for an array that is not 4-byte aligned.  Its first call (and a later one after the collider
   count has grown) ALLOCATES about 12 B per collider after a stream synchronise, as nh_overlap's scratch does; nh_destroy frees it.  Otherwise it only
   enqueues: two copies and the layer pass (timing labels q_layers_runs, q_layers_top).
   FILTER.  Context state, NH_FILTER_OFF after nh_create, read by EVERY later query call until changed:
     NH_FILTER_OFF        the library without this section; `mask` and `masks` are not read;
     NH_FILTER_UNIFORM    every query of a call uses `mask`; `masks` is not read;
     NH_FILTER_PER_QUERY  query i of a call uses masks[i]: DEVICE memory that must hold `count` words for each later call, retained BY POINTER until the
                          next nh_query_filter (the words are read when the query runs, not when the filter is set).  NULL or not 4-byte aligned:
                          NH_ERR_INVALID.
   An unknown mode, or a call before any nh_query_build, returns NH_ERR_INVALID; a refused call changes nothing -- the next query still uses the previous
   filter.  nh_query_filter is host state only: nothing is launched, nothing waits.  (The calls' own `flags` argument has no bit to spare for this.)
   THE CONTRACT, for all twenty-five query calls (nh_raycast, nh_spherecast, nh_boxcast, nh_capsulecast, their _all and _k forms, nh_overlap, nh_penetration,
   nh_region, nh_closest, nh_closest_k, nh_distance, nh_move, nh_recover, nh_walk, nh_boxmove, nh_boxwalk; for nh_region the query is the region: NH_FILTER_PER_QUERY reads masks[i] for region i)
   and for the twenty-sixth, nh_sense (the query is the SENSOR: NH_FILTER_PER_QUERY reads masks[s] for every ray of sensor s; nh_sense_rays casts nothing and reads no filter):
     - MASKED WORLD: with the filter on, a query with mask m writes byte for byte what the same call with the filter OFF writes on a world that is the same
       except for one thing: every collider with (layers & m) == 0 has a NaN pose -- "a collider of a body that does not exist", which every call above
       documents as never hit, never listed, never reported.  Collider indices, bodies and tags in the records are those of the real world.  For
       NH_RAY_ANY_HIT the guarantee is the same hit-or-miss, which is all that flag promises.
     - Everything else composes with the filter exactly as without it: `ignore_body`, NaN poses, invalid records, NH_RAY_ANY_HIT, capacities, counts and
       offsets, the tie rules, the reach rule.  The answers above are defined without the tree, so pruning by node words changes the work, never the bytes.
     - The four _touched forms of the movers (nh_move_touched, nh_boxmove_touched, nh_walk_touched, nh_boxwalk_touched) run their mover's casts under the same
       contract: results, counts and touches are those of the plain mover's casts on the masked world.
     - The two wide forms (nh_overlap_wide, nh_penetration_wide) run under the same contract: they write what nh_overlap and nh_penetration write on the
       masked world, NH_FILTER_PER_QUERY reading masks[i] for query i.
   Identities that follow:
     - mask 0 sees nothing: misses with t = max_t (max_distance), empty segments, counts 0;
     - all-ones layers (or none set) with any non-zero mask write the filter-off bytes;
     - NH_FILTER_OFF after any mode writes the filter-off bytes;
     - after nh_query_refit the bytes are those after an nh_query_build of the same arrays.
   A filter by TAG VALUE is a layer the caller derives from its tags ("layers").
   All three calls are OBSERVERS (note 9): no view export, no settling of deferred gravity, no still step turned into a full one, no change to nh_Counts.
   nh_query_layer_info (diagnostic; WAITS for the stream, like nh_query_stats): `set` says whether layers are in force, `colliders` is the last build's
   count, `any_layers` the root's node word -- the OR over all colliders (0xffffffff while none are set and the world has colliders, 0 for an empty world).
   The filtered calls launch a second instantiation of each walking kernel under the call's own timing label; the unfiltered kernels are unchanged.
   MEASURED (tools/filter_rates.py -> profiles/filter_rates.log; one MI355X, 1,048,576 incoherent queries on the landed config-2 world of 1,004,524
   colliders, the dynamic boxes in layer 2 and body 0's slabs in layer 1; ms per call: filter off / uniform mask 3, sees all / uniform mask 1, static only /
   per-query masks alternating 1 and 2):
     nh_raycast              1.952 / 2.238 / 0.303 / 2.105        nh_overlap (count, r = 1)   0.360 / 0.318 / 0.190 / 0.281
     nh_spherecast r = .75   3.591 / 3.835 / 0.325 / 3.608        nh_closest (unbounded)      1.220 / 1.765 / 2.602 / 2.828
   A cast that sees only the static world takes 0.09 - 0.16 of the unfiltered call; a mask that sees everything costs 7 - 15 % on the casts and 45 % on
   nh_closest (a third load per node).  nh_closest under a SPARSE mask is slower than unfiltered (2.1 x): its Morton seed meets only rejected leaves and
   the walk starts without a bound -- exact, but not fast; a seed that steps out to seen leaves is not built.  nh_query_set_layers 0.19 ms; a build with
   layers 0.79 ms against 0.59 without; a refit 0.24 either way.  The filter-off calls run at 0.994 - 1.005 of the parent commit's library beside it in the
   same process (which shows 0.999 - 1.015 against itself).  DESIGN 10.14 has the tables. */
enum { NH_FILTER_OFF = 0u, NH_FILTER_UNIFORM = 1u, NH_FILTER_PER_QUERY = 2u };
typedef struct nh_QueryLayerInfo { uint32_t set; uint32_t colliders; uint32_t any_layers; uint32_t reserved; } nh_QueryLayerInfo;
int nh_query_set_layers(nh_context* ctx, const uint32_t* box_layers /* boxes.count words, or NULL */, const uint32_t* sphere_layers /* spheres.count words, or NULL */);
int nh_query_filter(nh_context* ctx, uint32_t mode, uint32_t mask, const uint32_t* masks);
int nh_query_layer_info(nh_context* ctx, nh_QueryLayerInfo* out);

/* nh_spherecast: where a swept ball first touches the world of the LAST nh_query_build -- character controllers, thick projectiles, camera collision.
   nh_SphereCast's first 32 bytes are nh_Ray's fields at the same offsets; `reserved` is not read.  Exact predicates: nudge_amd/csrc/nh_query.h.
     - the swept ball is the ball of radius r = `radius` centred at o + t d, for 0 <= t <= max_t; t is in units of d, as for rays;
     - the hit on one collider is the smallest such t at which the ball touches it (touching counts, as in nh_overlap); the normal is a unit vector from
       the collider towards the ball's centre at t, so the contact point is o + t d - r * normal;
     - START OVERLAP: a ball that overlaps a collider at t = 0 under nh_overlap's own predicates (nh_q_overlap_sphere_sphere / nh_q_overlap_sphere_box) hits
       it at t = 0 with normal = -d / |d|, the ray's inside rule (how deep and which way out: nh_penetration, below);
     - over all colliders the answer follows nh_raycast: the closest hit, ties by (shape, collider index), `ignore_body`, NH_RAY_ANY_HIT, and a miss written
       exactly as a ray miss (shape = NH_SHAPE_NONE, t = max_t, normal = 0, body = collider = tag = 0xffffffff);
     - r = 0 IS A RAY: it writes the same bytes as nh_raycast with the same first 32 bytes.  A zero direction does what it does for a ray: a ball that
       touches at t = 0 hits there with a NaN normal (-d / |d| = 0 / 0), any other cast misses;
     - for r > 0 a hit also needs the ray to enter the collider's box in the hierarchy grown by r, and t is at least that entry (the reach rule, DESIGN 10.2:
       it is what lets the walk prune exactly; it moves t only where the predicate's rounding put the hit in front of a padded box);
     - a cast with a non-finite origin, direction or radius, or a negative radius, is written as a miss with t = NaN.
   Returns NH_ERR_INVALID before any nh_query_build, for flags other than 0 or NH_RAY_ANY_HIT, and for null or not 16-byte aligned `casts` / `hits`;
   count = 0 is a no-op that returns NH_OK.  An OBSERVER like nh_raycast (note 9): no view export, no settling of deferred gravity, no still step turned
   into a full one, no change to nh_Counts. */
typedef struct nh_SphereCast { float origin[3]; float max_t; float direction[3]; uint32_t ignore_body; float radius; uint32_t reserved[3]; } nh_SphereCast;  /* 48 B */
int nh_spherecast(nh_context* ctx, const nh_SphereCast* casts, uint32_t count, nh_RayHit* hits, uint32_t flags /* 0 or NH_RAY_ANY_HIT */);

/* nh_raycast_all / nh_spherecast_all: EVERY collider of the LAST nh_query_build that a ray (a swept ball) passes through, ordered along the cast -- a bullet or
   a laser that penetrates, line of sight through things the caller skips by tag, picking front to back, sensors that report all returns, a thick projectile.
   Input records are nh_raycast's / nh_spherecast's, output records nh_RayHit, in variable-length segments under nh_overlap's offsets and capacity contract.
     - THE SET of query i: every box and sphere collider of the last build (those of sleeping bodies and of body 0 included), less the colliders of
       `ignore_body`, on which the closest-hit call has a hit with 0 <= t <= max_t: for rays nh_q_ray_box / nh_q_ray_sphere; for sphere casts nh_q_sweep_box /
       nh_q_sweep_sphere, for r > 0 under nh_spherecast's reach rule applied to the collider's OWN box in the hierarchy (nh_q_leaf_box, nh_q_cast_node with
       w = r + nh_q_cast_pad): that box must be entered, and t = max(t of the predicate, the entry).  It is the test the closest-hit walk makes at a leaf
       with no best hit so far (nh_q_all_hit, nudge_amd/csrc/nh_query.h), so a brute force over all colliders gives the same set.  ONE record per collider:
       its entry.  An origin inside a collider, or a ball that starts in overlap, hits it at t = 0 with normal = -d / |d|, as in the closest-hit calls.
       Exits are not reported.  A collider of a NaN pose is never hit;
     - THE RECORD of a hit is byte for byte what the closest-hit call would write if that collider were the only one: t, normal, body, collider (the
       index within its own array), shape, tag;
     - THE ORDER within query i: ascending t compared as floats (-0 equals +0), ties by COMBINED collider index ascending (boxes 0 .. nbox-1, then the
       spheres -- the ray tie-break's order), so the output does not depend on the tree;
     - FIRST RECORD = CLOSEST HIT, a contract: where offsets[i+1] > offsets[i], hits[offsets[i]] holds exactly the 32 bytes nh_raycast (nh_spherecast)
       with flags = 0 writes for the same record on the same build or refit; where the segment is empty, that call writes a miss;
     - r = 0 IS A RAY: nh_spherecast_all with radius 0 writes the bytes nh_raycast_all writes for the same first 32 bytes;
     - offsets[0 .. count] (count + 1 words) by the exclusive scan of the per-query counts: offsets[i] = the records before query i, offsets[count] = the
       total; the records of query i are hits[offsets[i] .. offsets[i+1]);
     - COUNT ONLY: hits == NULL and capacity == 0 write offsets alone (count, read offsets[count], allocate, list);
     - CAPACITY: the records of query i are written if and only if offsets[i+1] <= capacity -- the written part is a prefix of whole segments, every byte of
       `hits` behind it is left untouched, and `offsets` is always complete;
     - a true total of 2^32 - 1 or more writes offsets[count] = 0xffffffff and no record at all (the other offsets are then unspecified), as in nh_overlap;
     - an INVALID record counts 0: a non-finite origin or direction, for sphere casts a non-finite or negative radius.  A NaN max_t lists nothing
       (t <= NaN is false); max_t = +inf lists everything ahead on the line.  A zero direction does what it does for the closest hit: the colliders that
       contain the origin (overlap the ball) at t = 0, with the NaN normal, and nothing else.
   Returns NH_ERR_INVALID before any nh_query_build, for flags != 0 (NH_RAY_ANY_HIT included: it has no meaning here), for `rays` / `casts` null or not
   16-byte aligned, `offsets` null or not 4-byte aligned, `hits` null with capacity > 0 or not 16-byte aligned, and for count >= 2^30; count = 0 is a no-op
   that returns NH_OK.
   An OBSERVER like nh_raycast (note 9): no view export, no settling of deferred gravity, no still step turned into a full one, no change to nh_Counts.
   Everything is enqueued on the context's stream, except that a larger capacity than any before grows the library's sort scratch after a stream
   synchronise, as in nh_overlap: the scratch is nh_overlap's own, and the ordering by t needs no further array -- it still takes ~24 B per record of capacity.
   Cost: the walk cannot prune by a best hit, only by max_t, it runs twice (count, list), and for rays it grows every node box by 2^-9 of its distance from
   the origin, so that no collider the ray predicates accept by rounding is pruned; the records are then ordered by one radix sort where
   bits(count) + 32 + bits(colliders) <= 64 and by two otherwise.  NOT MEASURED YET: tools/castall_rates.py times both calls (count only, count + list) on the landed config-2 world beside nh_raycast / nh_spherecast on the same records
   and nh_overlap in list mode, and writes profiles/castall_rates.log; no GPU run of it has been made, so neither ratio (count walk / closest-hit cast, list chain / nh_overlap's per record) is known.
   The all-hits casts of the other two shapes: nh_boxcast_all / nh_capsulecast_all, declared behind nh_capsulecast, whose records they read.
   The first k of each cast in one launch: nh_raycast_k / nh_spherecast_k, behind nh_capsulecast_all.
   Not built: exits. */
int nh_raycast_all(nh_context* ctx, const nh_Ray* rays, uint32_t count, uint32_t* offsets /* count + 1 */, nh_RayHit* hits, uint32_t capacity,
                   uint32_t flags /* 0 */);
int nh_spherecast_all(nh_context* ctx, const nh_SphereCast* casts, uint32_t count, uint32_t* offsets /* count + 1 */, nh_RayHit* hits, uint32_t capacity,
                      uint32_t flags /* 0 */);

/* nh_boxcast: where a swept oriented box first touches the world of the LAST nh_query_build -- "can this crate be pushed 3 m along x", where a door, lift or
   character hull stops.  nh_BoxCast's first 32 bytes are nh_Ray's fields at the same offsets; `size` holds half extents (as in nh_BoxCollider); `rotation`
   is a unit quaternion in (x, y, z, s) order (as in nh_OverlapQuery) that the library does not normalise; `reserved` is not read.  Exact predicates:
   nudge_amd/csrc/nh_query.h.
     - the swept box is the closed box of pose (o + t d, rotation) and half extents `size`, for 0 <= t <= max_t; it translates only, nothing rotates during
       the sweep; t is in units of d, as for rays;
     - the hit on one collider is the smallest such t at which the box touches it (touching counts, as in nh_overlap); the normal is a unit vector from the
       collider towards the cast box along the separating axis that is the last to close -- a face normal of either box or the normalised cross product of
       an edge pair -- signed against the direction (n.d < 0).  An edge pair within ~1e-3 rad of parallel still bounds t but never gives the normal (its
       cross product is rounding noise): when it closes last, the normal is the axis that closed last before it.  No contact point is reported;
     - START OVERLAP: a box that overlaps a collider at t = 0 under nh_overlap's own predicates (nh_q_overlap_box_box with the cast box as the query,
       nh_q_overlap_sphere_box for a sphere collider) hits it at t = 0 with normal = -d / |d|, the ray's inside rule; a start contact that only the sweep's
       rounding finds does the same (how deep and which way out: nh_penetration, below);
     - over all colliders the answer follows nh_raycast: the closest hit, ties by (shape, collider index), `ignore_body`, NH_RAY_ANY_HIT, and a miss written
       exactly as a ray miss (shape = NH_SHAPE_NONE, t = max_t, normal = 0, body = collider = tag = 0xffffffff); a collider of a body that does not exist
       (NaN pose) is never hit;
     - SIZE (0, 0, 0) IS A RAY: it writes the same bytes as nh_raycast with the same first 32 bytes, and `rotation` is not read.  A zero direction does what it
       does for a ray: a box that touches at t = 0 hits there with a NaN normal (-d / |d| = 0 / 0), any other cast misses;
     - for a nonzero size a hit also needs the ray to enter the collider's box in the hierarchy grown per axis by the cast box's world AABB half extent,
       and t is at least that entry (the reach rule, DESIGN 10.3, as for sphere casts);
     - a cast with a non-finite origin, direction or size, a negative size, or a nonzero size with a non-finite rotation is written as a miss with t = NaN.
   Returns NH_ERR_INVALID before any nh_query_build, for flags other than 0 or NH_RAY_ANY_HIT, and for null or not 16-byte aligned `casts` / `hits`;
   count = 0 is a no-op that returns NH_OK.  An OBSERVER like nh_raycast (note 9): no view export, no settling of deferred gravity, no still step turned
   into a full one, no change to nh_Counts. */
typedef struct nh_BoxCast { float origin[3]; float max_t; float direction[3]; uint32_t ignore_body;
                            float rotation[4]; float size[3]; uint32_t reserved; } nh_BoxCast;                                                    /* 64 B */
int nh_boxcast(nh_context* ctx, const nh_BoxCast* casts, uint32_t count, nh_RayHit* hits, uint32_t flags /* 0 or NH_RAY_ANY_HIT */);

/* nh_capsulecast: where a swept capsule first touches the world of the LAST nh_query_build -- character controllers, ragdoll limbs, thick swept projectiles,
   "is there head room to stand up".  A CAPSULE of centre c, rotation `rotation` (a unit quaternion in (x, y, z, s) order, as in nh_OverlapQuery, that the
   library does not normalise), radius r = `radius` >= 0 and half height hh = `half_height` >= 0 is the set of points within r of the segment c -+ a,
   a = rotate(rotation, (0, hh, 0)): its axis is the local y axis (the identity gives an upright capsule), and hh is half the segment's length, caps not
   included.  nh_CapsuleCast's first 32 bytes are nh_Ray's fields at the same offsets; `reserved` is not read.  Exact predicates: nudge_amd/csrc/nh_query.h.
     - the swept capsule is centred at o + t d, for 0 <= t <= max_t; it translates only, nothing rotates during the sweep; t is in units of d, as for rays;
     - the hit on one collider is the smallest such t at which the capsule touches it (touching counts, as in nh_overlap); the normal is a unit vector from
       the collider towards the capsule: against a sphere collider from its centre towards the segment's closest point; against a box, from an end ball
       (nh_spherecast's normal of that ball), from a box vertex towards the capsule's axis, or along the common normal of a box edge and the segment,
       signed against the direction (n.d < 0).  Box candidates are taken in the order end balls (the -a end first), vertices, edges, the first on equal
       t; an edge within ~1e-3 rad of parallel to the segment is left to the end balls and vertices.  No contact point is reported;
     - START OVERLAP: a capsule that overlaps a collider at t = 0 under nh_overlap's capsule predicates hits it at t = 0 with normal = -d / |d|, the ray's
       inside rule; a start contact that only the sweep's rounding finds does the same (how deep and which way out: nh_penetration, below);
     - over all colliders the answer follows nh_raycast: the closest hit, ties by (shape, collider index), `ignore_body`, NH_RAY_ANY_HIT (hit or miss agrees
       with the closest-hit answer, a reported hit is real), and a miss written exactly as a ray miss (shape = NH_SHAPE_NONE, t = max_t, normal = 0,
       body = collider = tag = 0xffffffff); a collider of a body that does not exist (NaN pose) is never hit;
     - HALF HEIGHT 0 IS A BALL: it writes the same bytes as nh_spherecast with the same first 32 bytes and radius, and `rotation` is not read -- so r = 0 with
       hh = 0 writes nh_raycast's bytes.  r = 0 with hh > 0 is a swept segment;
     - unless r = hh = 0, a hit also needs the ray to enter the collider's box in the hierarchy grown per axis by the capsule's world AABB half extent
       |a_k| + r, and t is at least that entry (the reach rule, DESIGN 10.4, as for sphere and box casts);
     - a cast with a non-finite origin, direction, radius or half height, a negative radius or half height, or hh > 0 with a non-finite rotation is written
       as a miss with t = NaN.
   Returns NH_ERR_INVALID before any nh_query_build, for flags other than 0 or NH_RAY_ANY_HIT, and for null or not 16-byte aligned `casts` / `hits`;
   count = 0 is a no-op that returns NH_OK.  An OBSERVER like nh_raycast (note 9): no view export, no settling of deferred gravity, no still step turned
   into a full one, no change to nh_Counts. */
typedef struct nh_CapsuleCast { float origin[3]; float max_t; float direction[3]; uint32_t ignore_body;
                                float rotation[4]; float radius; float half_height; uint32_t reserved[2]; } nh_CapsuleCast;                           /* 64 B */
int nh_capsulecast(nh_context* ctx, const nh_CapsuleCast* casts, uint32_t count, nh_RayHit* hits, uint32_t flags /* 0 or NH_RAY_ANY_HIT */);

/* nh_boxcast_all / nh_capsulecast_all: EVERY collider of the LAST nh_query_build that a swept oriented box (a swept capsule) touches, ordered along the
   cast -- a controller that slides past what it filters by tag, a push that wants every crate it will shove, a stand-up test that lists what is overhead.
   Input records are nh_boxcast's / nh_capsulecast's (64 B), output records nh_RayHit; everything else is nh_raycast_all's contract:
     - THE SET of cast i: every box and sphere collider of the last build or refit (those of sleeping bodies and of body 0 included), less the colliders of
       `ignore_body`, on which the closest-hit call has a hit with 0 <= t <= max_t.  It is the test nh_boxcast / nh_capsulecast make at a leaf with no best
       hit so far (nh_q_all_hit_box / nh_q_all_hit_capsule, nudge_amd/csrc/nh_query.h): the predicates nh_q_sweep_box_box / nh_q_sweep_box_sphere and
       nh_q_sweep_capsule_box / nh_q_sweep_capsule_sphere, and for a shape with a size -- a box of nonzero size, a capsule unless r = hh = 0 -- the reach
       rule applied to the collider's OWN box in the hierarchy (nh_q_leaf_box) grown per axis by the cast's world AABB half extent and pad under
       nh_q_cast_node3 (nh_q_leaf_entry3): that box must be entered, and t = max(t of the predicate, the entry).  So a brute force over all colliders gives
       the same set.  ONE record per collider: its entry.  A shape that starts in overlap with a collider hits it at t = 0 with normal = -d / |d|, as in the
       closest-hit calls.  Exits are not reported.  A collider of a NaN pose is never hit;
     - THE RECORD of a hit is byte for byte what nh_boxcast / nh_capsulecast with flags = 0 would write if that collider were the only one;
     - THE ORDER within cast i: ascending t compared as floats (-0 equals +0), ties by COMBINED collider index ascending (boxes 0 .. nbox-1, then the spheres);
     - FIRST RECORD = CLOSEST HIT, a contract: where offsets[i+1] > offsets[i], hits[offsets[i]] holds exactly the 32 bytes nh_boxcast (nh_capsulecast)
       with flags = 0 writes for the same record on the same build or refit; where the segment is empty, that call writes a miss;
     - DEGENERATE SHAPES write the bytes of the simpler all-hits call, offsets and records: a box of size (0, 0, 0) those of nh_raycast_all for the same first
       32 bytes, its rotation not read; a capsule of half_height 0 those of nh_spherecast_all for the same first 32 bytes and radius, its rotation not
       read; a capsule of radius = half_height = 0 those of nh_raycast_all.  In exactly these ray-like cases -- no size at all -- the walk grows every node
       box by 2^-9 of its distance from the origin, as nh_raycast_all's does; with a size, the reach rule makes the set a function of the leaf test alone;
     - offsets[0 .. count] (count + 1 words) by the exclusive scan of the per-cast counts: offsets[i] = the records before cast i, offsets[count] = the
       total; the records of cast i are hits[offsets[i] .. offsets[i+1]);
     - COUNT ONLY: hits == NULL and capacity == 0 write offsets alone (count, read offsets[count], allocate, list);
     - CAPACITY: the records of cast i are written if and only if offsets[i+1] <= capacity -- the written part is a prefix of whole segments, every byte of
       `hits` behind it is left untouched, and `offsets` is always complete;
     - a true total of 2^32 - 1 or more writes offsets[count] = 0xffffffff and no record at all (the other offsets are then unspecified), as in nh_overlap;
     - an INVALID record counts 0 -- exactly the records the closest-hit call writes with t = NaN: a non-finite origin, direction or size (radius, half
       height), a negative size, a non-finite rotation where the rotation is read.  A NaN max_t lists nothing (t <= NaN is false).  A zero direction lists
       the colliders the shape overlaps at t = 0, with the NaN normal, and nothing else.
   Returns NH_ERR_INVALID before any nh_query_build, for flags != 0 (NH_RAY_ANY_HIT included: it has no meaning here), for `casts` null or not 16-byte
   aligned, `offsets` null or not 4-byte aligned, `hits` null with capacity > 0 or not 16-byte aligned, and for count >= 2^30 -- nh_overlap's checks in
   nh_overlap's order; count = 0 is a no-op that returns NH_OK.
   An OBSERVER like nh_raycast (note 9): no view export, no settling of deferred gravity, no still step turned into a full one, no change to nh_Counts.
   Everything is enqueued on the context's stream, except that a larger capacity than any before grows the library's sort scratch after a stream
   synchronise: the scratch is nh_overlap's own, and nothing else is allocated.
   Cost: nh_raycast_all's chain with the box's / the capsule's predicates at the leaves -- the walk prunes by max_t only and runs twice (count, list), then
   one or two radix sorts and a gather that evaluates the predicate a third time for the written records (figures, or NOT MEASURED YET).
   The first k of each cast in one launch: nh_boxcast_k / nh_capsulecast_k, below.
   Not built: exits, rotating sweeps. */
int nh_boxcast_all(nh_context* ctx, const nh_BoxCast* casts, uint32_t count, uint32_t* offsets /* count + 1 */, nh_RayHit* hits, uint32_t capacity,
                   uint32_t flags /* 0 */);
int nh_capsulecast_all(nh_context* ctx, const nh_CapsuleCast* casts, uint32_t count, uint32_t* offsets /* count + 1 */, nh_RayHit* hits, uint32_t capacity,
                       uint32_t flags /* 0 */);

/* nh_raycast_k / nh_spherecast_k / nh_boxcast_k / nh_capsulecast_k: the FIRST `k` colliders along each of `count` casts, in order -- a bullet that goes
   through at most three crates, line of sight that skips the first thing it meets, a controller that wants the first
   few things ahead of its hull, a sensor with a fixed number of returns.  Input records are the closest-hit calls' (nh_Ray, nh_SphereCast, nh_BoxCast,
   nh_CapsuleCast), output records nh_RayHit at a fixed stride of k per cast, as in nh_closest_k; `k` is one value per call, 1 .. NH_CAST_K_MAX.
     - THE CONTRACT: for cast i let S_i be the segment nh_<shape>cast_all lists for the same record on the same build or refit -- the same set, the same
       records, ascending t compared as floats (-0 equals +0), ties by combined collider index ascending -- and m_i = min(k, |S_i|).  Then
       hits[i*k + j] for j < m_i holds, byte for byte, record j of S_i; hits[i*k + j] for j >= m_i holds the miss record the closest-hit call writes
       for that cast (shape = NH_SHAPE_NONE, normal = 0, body = collider = tag = 0xffffffff, t = max_t -- t = NaN for a record the closest-hit call
       writes as t = NaN); counts[i] = m_i where `counts` is not NULL.  Every byte of all count * k records is written and nothing behind them.
   What follows are identities of that contract and the contracts above:
     - PREFIX: for k < k' the records under k are the first k records of each cast under k';
     - k = 1 IS THE CLOSEST-HIT CALL with flags = 0: `hits` holds exactly the bytes nh_raycast (nh_spherecast, nh_boxcast, nh_capsulecast) writes for
       the same records -- the all-hits calls' FIRST RECORD contract where the segment is not empty, the miss otherwise;
     - DEGENERATE SHAPES write the simpler call's bytes, counts and records: a box of size (0, 0, 0) those of nh_raycast_k for the same first 32 bytes;
       a capsule of half_height 0 those of nh_spherecast_k for the same first 32 bytes and radius; a ball of radius 0 those of nh_raycast_k; a capsule
       of radius = half_height = 0 those of nh_raycast_k.  Rotations are not read where the closest-hit call does not read them;
     - REFIT: the bytes after nh_query_refit are the bytes after an nh_query_build of the same arrays;
     - an INVALID record (one the closest-hit call writes with t = NaN) counts 0 and writes k misses of t = NaN;
     - a NaN max_t lists nothing (t <= NaN is false); its k misses carry t = max_t, the NaN itself.  max_t = +inf finds the first k anywhere ahead;
     - a ZERO DIRECTION lists the colliders the shape overlaps at t = 0, with the NaN normal, the lowest combined index first, and nothing else;
     - `ignore_body` and colliders of a NaN pose behave as in the all-hits calls: never listed.
   Returns NH_ERR_INVALID, in nh_closest_k's order of checks: before any nh_query_build; for flags != 0 (NH_RAY_ANY_HIT included: it has no meaning
   here); for k = 0 or k > NH_CAST_K_MAX; for count >= 2^30; then, for count > 0, for `casts` or `hits` null or not 16-byte aligned and for `counts` not
   4-byte aligned.  count = 0 is a no-op that returns NH_OK and launches nothing.  A refused call writes nothing.
   An OBSERVER like nh_raycast (note 9): no view export, no settling of deferred gravity, no still step turned into a full one, no change to nh_Counts.
   It never allocates and never waits: ONE launch on the context's stream (timing labels q_raycast_k, q_spherecast_k, q_boxcast_k, q_capsulecast_k),
   where the all-hits chain walks twice, sorts once or twice, gathers, and has the caller read a total back to size `hits`.
   One lane per cast keeps its list of k (t, combined index) pairs in LDS and prunes the walk at the k-th t so far (why that is exact);
   the records are rebuilt from the listed colliders as the all-hits gather rebuilds them.
   MEASURED (tools/castk_rates.py -> profiles/castk_rates.log; one MI355X, 1,048,576 incoherent casts on the landed config-2 world of 1,004,524
   colliders, beside the closest-hit call and the all-hits count + list calls on the same records): at k = 1 a shape with a size costs 0.91 - 1.03 of
   its closest-hit call and a ray 5.7 x nh_raycast (its walk takes the all-hits node pad); the k call takes 0.18 - 0.29 of count + list at k = 1,
   0.33 - 0.38 at k = 4 and 0.48 - 0.81 at k = 32.  DESIGN 10.13 has the table.
   Where nh_raycast itself loses a far grazing hit that the ray predicates accept by rounding, the k = 1 identity holds with the
   all-hits first record, not with nh_raycast's bytes.
   Not built: a per-cast k, exits.  (A filter by tag VALUE is a layer the caller derives from its tags: "layer masks", below.) */
#define NH_CAST_K_MAX 32u
int nh_raycast_k(nh_context* ctx, const nh_Ray* rays, uint32_t count, uint32_t k,
                 uint32_t* counts /* count words, or NULL */, nh_RayHit* hits /* count * k */, uint32_t flags /* 0 */);
int nh_spherecast_k(nh_context* ctx, const nh_SphereCast* casts, uint32_t count, uint32_t k,
                    uint32_t* counts /* count words, or NULL */, nh_RayHit* hits /* count * k */, uint32_t flags /* 0 */);
int nh_boxcast_k(nh_context* ctx, const nh_BoxCast* casts, uint32_t count, uint32_t k,
                 uint32_t* counts /* count words, or NULL */, nh_RayHit* hits /* count * k */, uint32_t flags /* 0 */);
int nh_capsulecast_k(nh_context* ctx, const nh_CapsuleCast* casts, uint32_t count, uint32_t k,
                     uint32_t* counts /* count words, or NULL */, nh_RayHit* hits /* count * k */, uint32_t flags /* 0 */);

/* nh_closest: how far each of `count` points lies from the world of the LAST nh_query_build, and where the nearest surface is -- depenetration, "snap to
   the nearest surface", proximity and cover tests, keeping a distance from everything.  `reserved` is not read.  Exact predicates: nudge_amd/csrc/nh_query.h.
     - the SIGNED DISTANCE of p from one collider is negative inside it.  A sphere (c, R): m = p - c, L = sqrtf(m.m), distance = L - R, normal = m / L,
       point = c + R normal; at L = 0 (the centre) the normal is +y.  A box (pose, half extents h), p in the box frame l (nh_q_overlap_sphere_box's
       inverse rotation): OUTSIDE (some |l_k| > h_k) the clamp ql = clamp(l, -h, h), e = l - ql, distance = sqrtf(e.e), normal = e / distance turned
       to world, point = the world position of ql; INSIDE or on the surface the face k of least depth h_k - |l_k| (the lowest axis on equality),
       distance = 0 - depth (+0 on the surface, never -0), normal = +-e_k by the sign of l_k (a zero l_k counts as +) turned to world, point = l with
       l_k replaced by +-h_k, in world;
     - `normal` is a unit vector out of the collider (towards p when p is outside); `point` is on the collider's surface, so p = point + distance normal
       up to rounding;
     - the answer is the smallest distance with distance <= max_distance over the colliders not belonging to `ignore_body` (0xffffffff: none is
       ignored) -- inside several, the deepest -- with ties by (shape, collider index) ascending, so a brute force over all colliders gives the same
       bytes.  max_distance = +inf finds the nearest collider anywhere; max_distance = 0 only colliders that contain or touch p.  A collider of a body
       that does not exist (NaN pose) is never reported;
     - THE REACH RULE: where p lies outside the collider's box in the hierarchy (k_q_boxes_runs' padded box) at squared distance d2 > 0
       (per axis fmaxf(fmaxf(lo - p, p - hi), 0), then the sum of the squares), the distance is max(distance, sqrtf(d2)).  It is what lets the walk
       prune exactly; it moves a distance only where rounding put the predicate in front of a box padded by 2^-18 of its coordinates;
     - a miss writes shape = NH_SHAPE_NONE, distance = max_distance, normal = point = 0 and body = collider = tag = 0xffffffff;
     - a query with a non-finite point, or a NaN or negative max_distance, is written as a miss with distance = NaN;
     - `reserved` of every hit is written 0.
   Returns NH_ERR_INVALID before any nh_query_build, for flags != 0, and for null or not 16-byte aligned `queries` / `hits`; count = 0 is a no-op that
   returns NH_OK.  An OBSERVER like nh_raycast (note 9): no view export, no settling of deferred gravity, no still step turned into a full one, no change
   to nh_Counts.  The distance of a shape from the world: nh_distance, below.  The k nearest colliders: nh_closest_k, below. */
typedef struct nh_PointQuery { float point[3]; float max_distance; uint32_t ignore_body; uint32_t reserved[3]; } nh_PointQuery;                     /* 32 B */
typedef struct nh_PointHit { float distance; float normal[3]; float point[3]; uint32_t body;
                             uint32_t collider; uint32_t shape; uint32_t tag; uint32_t reserved; } nh_PointHit;                                  /* 48 B */
int nh_closest(nh_context* ctx, const nh_PointQuery* queries, uint32_t count, nh_PointHit* hits, uint32_t flags /* 0 */);

/* nh_closest_k: the `k` nearest colliders to each of `count` points, nearest first -- proximity sensors, crowd and flocking neighbourhoods, "which crates
   are within reach", candidate sets for grabbing and audio occlusion, a depenetration that needs more than the deepest collider.  The records are
   nh_closest's (nh_PointQuery in, nh_PointHit out); `k` is one value per call, 1 .. NH_CLOSEST_K_MAX.
     - THE CANDIDATES of query i: every box and sphere collider of the last build or refit -- those of sleeping bodies and of body 0 included -- less the
       colliders of `ignore_body`.  A candidate's key is nh_closest's distance for that collider alone: the predicate distance d under the reach rule
       (nh_q_point_key(d, d2), d2 the squared distance of the point from the collider's own leaf box), and it must satisfy
       key <= max_distance.  A collider of a NaN pose is never a candidate;
     - THE ORDER: ascending key, compared as floats; ties go to the lower combined collider index (boxes 0 .. nbox-1, then the spheres).  This is the
       strict order nh_closest chooses by, so the answer does not depend on the tree, and a brute force that sorts all candidates gives the same bytes;
     - THE OUTPUT: with m_i = min(k, number of candidates), hits[i*k + j] for j < m_i is the j-th candidate in that order, byte for byte the record
       nh_closest writes for that collider alone (distance = its key, normal, point, body, collider, shape, tag, reserved = 0); hits[i*k + j] for
       j >= m_i is nh_closest's miss record (distance = max_distance, or NaN for an invalid query).  Every byte of all count*k records is written and
       nothing behind them; counts[i] = m_i where `counts` is not NULL;
     - k = 1 IS nh_closest: `hits` holds exactly the bytes nh_closest writes for the same queries on the same build or refit.  PREFIX: for k < k' the
       first k records of every query under k' are the records under k;
     - an invalid query (non-finite point, NaN or negative max_distance) finds nothing: counts[i] = 0 and k miss records of distance NaN.
       max_distance = +inf finds the k nearest anywhere; max_distance = 0 only colliders that contain or touch the point, the deepest first.
   Returns NH_ERR_INVALID before any nh_query_build, for flags != 0, for k = 0 or k > NH_CLOSEST_K_MAX, for `queries` or `hits` null or not 16-byte
   aligned, for `counts` not 4-byte aligned, and for count >= 2^30; count = 0 is a no-op that returns NH_OK.  An OBSERVER like nh_closest (note 9): no
   view export, no settling of deferred gravity, no still step turned into a full one, no change to nh_Counts; it never allocates and never waits, it
   only launches on the context's stream.
   One lane per query keeps its list of k (key, index) pairs in LDS and prunes the walk at the k-th key so far (why that is exact).
   NOT MEASURED YET, and not run on a GPU yet: no GPU could be had while this was built.  tools/nearest_rates.py is the measurement (the landed config-2 world of
   1,004,524 colliders, 1 M queries, k = 1 .. 32 beside nh_closest and beside the nh_overlap detour in one run -> profiles/nearest_rates.log). */
#define NH_CLOSEST_K_MAX 32u
int nh_closest_k(nh_context* ctx, const nh_PointQuery* queries, uint32_t count, uint32_t k,
                 uint32_t* counts /* count words, or NULL */, nh_PointHit* hits /* count * k records */, uint32_t flags /* 0 */);

/* nh_overlap: which colliders of the LAST nh_query_build touch each of `count` query shapes -- explosion radii, trigger volumes, "is this spot free".
   Query shapes (nh_OverlapQuery):
     - shape = NH_SHAPE_SPHERE: the ball of radius size[0] around `center`; rotation and size[1..2] are ignored.  Radius 0 is a point query;
     - shape = NH_SHAPE_BOX: the oriented box of half extents `size` (as in nh_BoxCollider) and rotation `rotation`, a unit quaternion in nh_Transform's
       (x, y, z, s) order that the library does not normalise.
     - shape = NH_SHAPE_CAPSULE: the capsule (nh_capsulecast) of radius size[0], half height size[1] and rotation `rotation` around `center`; size[2] is
       not read.  Against a sphere collider (p, R) it overlaps iff the squared distance from p to its segment is at most (r + R)^2; against a box collider
       iff its segment comes within r of the box: the ball of radius r swept from c - a to c + a reaches the box (nh_q_sweep_box, t <= 1) or the ball at
       c + a touches it -- so whatever the sphere query accepts at either end point is accepted.  Both predicates also require the capsule's world AABB,
       c -+ (|a_k| + r), to touch the collider's, so that the walk never prunes a collider they accept.  Half height 0 IS A SPHERE query of radius size[0]:
       the same records, and `rotation` is not read.
   The answer of query i is the set of colliders that overlap its shape as CLOSED sets (touching counts), over every box and sphere collider of the last build
   (those of sleeping bodies and of body 0 included), less the colliders of `ignore_body` (0xffffffff: none is ignored).  A collider whose body does not exist
   (NaN pose) overlaps nothing.  Exact predicates: nudge_amd/csrc/nh_query.h.
   Output, by the exclusive scan of the per-query counts:
     - offsets[0 .. count] (count + 1 words): offsets[i] = the records before query i, offsets[count] = the total;
     - the records of query i are hits[offsets[i] .. offsets[i+1]), in ascending COMBINED collider index (boxes 0 .. nbox-1, then the spheres -- the ray
       tie-break's order), so the output does not depend on the tree: a brute force gives the same bytes.  `collider` is the index within its own array and
       `shape` says which array, as in nh_RayHit;
     - COUNT ONLY: hits == NULL and capacity == 0 write offsets alone (count, read offsets[count], allocate, list);
     - CAPACITY: the records of query i are written if and only if offsets[i+1] <= capacity -- the written part is a prefix of whole segments, every byte of
       `hits` behind it is left untouched, and `offsets` is always complete;
     - a true total of 2^32 - 1 or more writes offsets[count] = 0xffffffff and no record at all (the other offsets are then unspecified).  Every per-query
       count is below 2^30, so the 32-bit scan has wrapped iff some offsets[i+1] < offsets[i]; a total of exactly 2^32 - 1 is the marker itself.
   An INVALID query overlaps nothing (count 0): an unknown shape, a non-finite centre or size (for a sphere size[0] alone, for a capsule size[0] and
   size[1]), for a box or a capsule of nonzero half height a non-finite rotation, or a negative size (of those read).  As with non-finite rays, an asynchronous call cannot refuse one record.
   Returns NH_ERR_INVALID before any nh_query_build, for flags != 0, for `queries` null or not 16-byte aligned, `offsets` null or not 4-byte aligned, `hits`
   null with capacity > 0 or not 16-byte aligned, and for count >= 2^30; count = 0 is a no-op that returns NH_OK.
   An OBSERVER like nh_raycast (note 9): no view export, no settling of deferred gravity, no still step turned into a full one, no change to nh_Counts.  Everything
   is enqueued on the context's stream, except that a larger capacity than any before grows the library's sort scratch (~24 B per record of capacity) after a
   stream synchronise, as a build that grows does. */
typedef struct nh_OverlapQuery { float center[3]; uint32_t shape; float rotation[4]; float size[3]; uint32_t ignore_body; } nh_OverlapQuery;  /* 48 B */
typedef struct nh_OverlapHit { uint32_t body; uint32_t collider; uint32_t shape; uint32_t tag; } nh_OverlapHit;                            /* 16 B */
int nh_overlap(nh_context* ctx, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets /* count + 1 */, nh_OverlapHit* hits, uint32_t capacity,
               uint32_t flags /* 0 */);

/* nh_penetration: the push that frees a query shape -- for every collider of the LAST nh_query_build that each of `count` query shapes overlaps, the
   least translation of the query shape after which the two only touch (the penetration depth, "compute penetration", MTD): what a character
   controller needs when a cast starts in contact (START OVERLAP above), a crate pushed against a wall, a spawn test that nudges a shape into free space.
   THE CALL IS nh_overlap WITH A RICHER RECORD, and that is a contract:
     - for the same queries on the same build or refit, `offsets` holds exactly the bytes nh_overlap writes, and record j carries in its last 16 bytes
       (body, collider, shape, tag) exactly the nh_OverlapHit nh_overlap writes at j.  The set is decided by nh_overlap's own predicates (the same
       kernels run them), and the order is nh_overlap's: by query, then by combined collider index;
     - everything else carries over unchanged, with 32-byte records: query shapes (a capsule of half height 0 IS A SPHERE query: the same bytes as the
       sphere query of that radius, `rotation` not read), COUNT ONLY, the CAPACITY prefix rule (the records of query i are written iff
       offsets[i+1] <= capacity, every byte behind the written prefix is left untouched), the 0xffffffff overflow marker, invalid queries counting 0,
       `ignore_body`, colliders of a NaN pose, the return codes (`hits` 16-byte aligned), the growth of the sort scratch by capacity, and the OBSERVER
       property (note 9);
     - `normal` is a unit vector from the collider towards the query shape, the casts' convention;
     - `depth` >= +0: the query shape moved by depth * normal touches the collider, and no shorter translation in any direction separates the two, up
       to rounding and to the 2^-20 the box / box radii carry (measured: within 3.7e-6 of the pair's sizes plus centre distance).  A pair
       that nh_overlap accepts by rounding alone gets depth = +0, never a negative value or -0.
   Per pair (exact arithmetic: nudge_amd/csrc/nh_query.h, "penetration"; d and the normals of a point are nh_closest's):
     - sphere query / sphere: depth = r - (|c - p| - R), normal = (c - p) / |c - p|, +y at coincident centres;
     - sphere query / box: depth = r - d with d the signed distance of the centre from the box (inside: r + the depth of its nearest face), its normal;
     - box query / sphere: depth = R - d with d the signed distance of the sphere's centre from the query box, that normal negated;
     - capsule / sphere: from the sphere's centre to the segment's closest point m: depth = (r + R) - |m|, normal = m / |m|; where the segment passes
       through the centre, a x e_k normalised for the axis k of the smallest |a_k|;
     - box query / box: the least overlap over the 15 separating axes of nh_overlap's test, an edge pair's divided by the length of its cross product;
       ties to the first of: faces of the query box, faces of the collider, edge pairs; an edge pair within ~1e-3 rad of parallel gives neither depth
       nor normal.  normal = that axis, from the collider to the query box (the + side where the centres project to the same point);
     - capsule / box: where the segment misses the box, depth = r - their distance (the end points against the box, the -a end first, then the twelve
       box edges against the segment) and normal = along their closest points; where it meets the box, depth = r + the least overlap over the box's
       face normals and the three a x e_k, normal = that axis on the centre's side.
   No contact point and no resolved push-out of a query against all its colliders is reported: callers combine the records.  The distance
   of a shape from colliders it does not touch: nh_distance, below.
   Cost: the chain is nh_overlap's in list mode (1.49 ms to list 1 M sphere queries of one box's size on the landed config-2 world) with a
   gather that reads 108 and writes 32 bytes per record where nh_overlap's reads 52 and writes 16.  NOT MEASURED YET: tools/penetration_rates.py times
   nh_penetration beside nh_overlap in list mode for 1 M sphere, box and capsule queries and writes profiles/penetration_rates.log; no GPU run of it
   exists. */
typedef struct nh_PenetrationHit { float normal[3]; float depth; uint32_t body; uint32_t collider; uint32_t shape; uint32_t tag; } nh_PenetrationHit;  /* 32 B */
int nh_penetration(nh_context* ctx, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets /* count + 1 */, nh_PenetrationHit* hits,
                   uint32_t capacity, uint32_t flags /* 0 */);

/* nh_region: which colliders of the LAST nh_query_build or nh_query_refit lie inside each of `count` convex regions -- the colliders in a camera
   frustum or a shadow cascade before nh_stream_state is read, the colliders in a client's area of interest, "everything in this slab".  The large
   question: a region may cover the whole world.  Every other query call gives one lane to a query; here the work of ONE region spreads over the GPU.
   REGIONS (nh_Region): the intersection of the first `plane_count` (1 .. NH_REGION_MAX_PLANES) half-spaces.  Plane k is (nx, ny, nz, d): a point x is
   inside it iff n.x + d >= 0.  n need not be unit length.  Planes behind `plane_count` and `reserved` are not read.
   PER PLANE (float32, exactly nudge_amd/csrc/nh_query.h, "region"; each product rounded before its sum, dot = (x*x + y*y) + z*z, no fused multiply-add):
   the plane KEEPS a collider at world position p iff s + r >= 0.0f, with s = dot(n, p) + d and r the collider's reach along n:
     - sphere of radius R: r = R * sqrtf(dot(n, n));
     - box of half extents h and rotation q: r = (h.x * |dot(n, A.c0)| + h.y * |dot(n, A.c1)|) + h.z * |dot(n, A.c2)|, A = the rotation matrix of q.
   THE ANSWER of region i is every box and sphere collider of the last build or refit (those of sleeping bodies and of body 0 included) that EVERY one of
   its planes keeps, less the colliders of `ignore_body` (0xffffffff: none is ignored).  A collider of a NaN pose (a body that does not exist) is never
   listed: s is NaN and the >= fails.  This is the standard plane-by-plane frustum test, and it is CONSERVATIVE: it never misses a collider that reaches
   into the region, and it may list one that lies outside it near an edge or a corner where two planes meet (the collider crosses each plane, but not
   where they cross each other).  The answer is defined without the tree: a brute force over all colliders gives the same bytes.
   An INVALID region lists nothing (count 0): plane_count == 0 or > NH_REGION_MAX_PLANES, a non-finite coefficient among those it reads, or a counted
   plane whose dot(n, n) is not finite or not > 0 (a zero normal, a normal whose square overflows).  An asynchronous call cannot refuse one record.
   OUTPUT, ORDER AND CAPACITY ARE nh_overlap's, word for word (the same chain of launches writes them): offsets[0 .. count] by the exclusive scan of
   the per-region counts; the records of region i are hits[offsets[i] .. offsets[i+1]) as nh_OverlapHit in ascending COMBINED collider index; COUNT ONLY
   with hits == NULL and capacity == 0; the CAPACITY prefix rule (segment i is written iff offsets[i+1] <= capacity, every byte of `hits` behind the
   written prefix is left untouched, `offsets` is always complete); a true total of 2^32 - 1 or more writes offsets[count] = 0xffffffff and no record.
   Returns NH_ERR_INVALID before any nh_query_build, for flags != 0, for `regions` null or not 16-byte aligned, `offsets` null or not 4-byte aligned,
   `hits` null with capacity > 0 or not 16-byte aligned, and for count >= 2^30 -- nh_overlap's checks in nh_overlap's order; count = 0 is a no-op that
   returns NH_OK.  A world of zero colliders gives all-zero offsets.
   An OBSERVER like nh_overlap (note 9): no view export, no settling of deferred gravity, no still step turned into a full one, no change to nh_Counts.
   Everything is enqueued on the context's stream, except that a list call with a larger capacity than any before grows nh_overlap's sort scratch, and one
   with a larger count than any before a cursor word per region, each after a stream synchronise.  Layer masks: the twenty-first call of that contract.
   HOW: a work item is (region, entry node), the entry nodes being the disjoint subtrees of at most 1024 consecutive leaves the box pass
   starts its top phase from (about ten thousand at a million colliders).  A lane tests an item's box against the planes; for each item that is not
   outside, a wave sweeps the entry's contiguous leaves with the exact predicate, the planes in scalar registers.  No walk, no stack, no one-lane tail.
   Timing labels: q_region_count, q_region_list, then nh_overlap's own.
   MEASURED (tools/region_rates.py -> profiles/region_rates.log; one MI355X, one run, the landed config-2 world of 1,004,524 colliders and 9,823 entry
   nodes; ms per call, the best of 5 blocks of 20 calls by device events -- nh_overlap one call a block; the count-only call / it followed by the exactly
   sized list call):
     (a) one region that is the world's AABB, 1,004,524 records          0.152 / 0.681      nh_overlap with that box, one lane      1795.8 / 5979.2
     (b) one frustum that sees a tenth, 100,452 records                  0.048 / 0.191
     (c) 64 such frusta, 4,518,700 records                               0.557 / 2.323
     (d) 4,096 cubes of one tile's size (267 units), 29,785,535 records  1.582 / 8.173      nh_overlap with the cubes, a lane each    33.42 / 109.20
   WHICH CALL FOR WHICH QUESTION: nh_region for a volume of a tile's size or more (nh_overlap takes 21 x as long to count at that size and 11,800 x for the
   world, where a full step takes 0.27 ms) and for anything that is not a sphere, a box or a capsule; nh_overlap for shapes of a body's size, where a lane per
   query is the right shape (1 M of them count in 0.64 ms) and its predicates are exact where this test is conservative (in (d) it lists 174 fewer of
   29.8 M records).  For large spheres, boxes and capsules there is nh_overlap_wide (below): the same decomposition with nh_overlap's exact predicates; it and
   nh_overlap cross at a radius of about 12 units, eight bodies across, on that world (4,096 spheres: nh_overlap 6 x faster at radius 1.5, 2 x at 6, equal at
   12; nh_overlap_wide 2.5 x faster at 24, 16 x at 96, 38 x at a tile's 267).  With 30 M records the sort of the shared chain is the largest part of the
   list call.  DESIGN 10.16 has the tables and the per-label times.
   Not built: regions of more than eight planes; exact (non-conservative) convex intersection; queries on a partitioned world, as before. */
#define NH_REGION_MAX_PLANES 8u
typedef struct nh_Region { float planes[NH_REGION_MAX_PLANES][4]; uint32_t plane_count; uint32_t ignore_body; uint32_t reserved[2]; } nh_Region;   /* 144 B */
int nh_region(nh_context* ctx, const nh_Region* regions, uint32_t count, uint32_t* offsets /* count + 1 */, nh_OverlapHit* hits, uint32_t capacity,
              uint32_t flags /* 0 */);

/* ---- sensors: depth cameras and lidar fans cast from poses ---------------------------------------------------------------------------------------
   nh_sense: `count` sensors with `beam_count` rays each -- agent perception, every step -- in ONE launch from (sensor poses, one shared beam pattern) to
   depth / id images.  No nh_Ray and no nh_RayHit record is materialised: 4,096 agents with 64 x 64 beams are 16.7 M rays, 537 MB of ray records and
   537 MB of hit records through nh_raycast, against 192 KB of sensors, 64 KB of pattern and 67 MB for a depth image here.  A sensor MOUNTED on a body
   follows it with no per-frame upload: step -> nh_query_refit -> nh_sense is an agent's whole frame on the device.
   THE RAY of beam j of sensor s has index i = s * beam_count + j and is the nh_Ray
       origin = p_s,  direction = rotate(q_s, beams[j].direction),  max_t = beams[j].range,  ignore_body = sensors[s].ignore_body
   (float32, exactly nudge_amd/csrc/nh_query.h, "sensors": nh_q_sensor_pose, nh_q_sensor_ray; rotate is the step's own quaternion rotation).  The pose
   (p_s, q_s) is the sensor's own `position` / `rotation` when `body` == 0xffffffff or `bodies` == NULL (the `body` word is then not read for a NULL
   `bodies`); otherwise the sensor's pose is the LOCAL transform of body `body`, composed with bodies->transforms[body] as a collider's is with its body's
   (nudge.cpp:1165-1175): p_s = rotate(q_body, position) + p_body, q_s = q_body * rotation.  bodies->transforms is read as the stream has it at that point.
   A mount with body >= bodies->count makes every ray of that sensor INVALID: all six words of origin and direction are the quiet NaN 0x7fc00000; max_t
   and ignore_body are set as for any other ray.  The direction need not be unit length (t is in units of it): a beam of unit direction measures range in
   world units, and a pinhole pattern with direction.z = 1 measures depth along the optical axis.
   nh_sense_rays writes exactly these `count * beam_count` nh_Ray records (for a caller that wants the rays themselves, for nh_raycast_all or nh_raycast_k
   on a sensor's rays, and for the tests).
   nh_sense writes, for every i, into each non-NULL channel of `out` (a HOST struct of DEVICE pointers, each count * beam_count long or NULL) the
   corresponding field of the nh_RayHit that nh_raycast writes for ray i under the same `flags` and the context's filter: t[i] = .t (max_t at a miss, NaN
   at an invalid ray), body[i] = .body and tag[i] = .tag (0xffffffff at a miss), hits[i] = the whole record.  Everything else follows from that identity
   and has no rules of its own: zero directions, origins inside a collider, NaN poses, `ignore_body`, the tie rule, NH_RAY_ANY_HIT (the same hit-or-miss;
   a reported hit is a real one with t <= max_t), and the MASKED WORLD contract of the layer masks, where the query is the SENSOR: NH_FILTER_PER_QUERY
   reads masks[s] for sensor s (`count` words), as nh_region reads masks[i] for region i.  A NULL channel costs nothing; a depth image is `t` alone.
   THE TREE is that of the last nh_query_build / nh_query_refit, while a mounted sensor reads TODAY's body transforms: after a step, call nh_query_refit
   first, or the sensors have moved and the world they see has not.
   Both return NH_ERR_INVALID before any nh_query_build; for flags other than 0 or NH_RAY_ANY_HIT (nh_sense_rays: other than 0); for
   count * beam_count >= 2^31; and, where count and beam_count are both non-zero, for `sensors`, `beams`, `rays` or out->hits null (hits: when given) or
   not 16-byte aligned, out->t / out->body / out->tag not 4-byte aligned, `out` NULL or all four channels NULL, and `bodies` given with a NULL
   bodies->transforms.  count == 0 or beam_count == 0 is a no-op that returns NH_OK: nothing is read.  A refused call writes nothing.
   Never allocate, never wait: ONE launch each on the context's stream (timing labels q_sense, q_sense_rays).  OBSERVERS like nh_raycast (note 9): no view
   export, no settling of deferred gravity, no still step turned into a full one, no change to nh_Counts.
   HOW: the work item of a WAVE is (sensor, block of 64 consecutive beams).  The sensor's record, its mount and the pose composition are
   read and done once per wave; the lanes read 64 adjacent beams, rotate them and walk the tree with nh_raycast's own per-ray body on a ray held in
   registers; each requested channel leaves as one 4-byte store per lane.  The ORDER of the pattern decides which rays share a wave: beams that are
   neighbours in direction should be neighbours in the pattern (an 8 x 8 image tile per 64 beams rather than a 64-pixel row: INTEGRATION.md, "sensors").
   MEASURED (tools/sense_rates.py -> profiles/sense_rates.log; one MI355X, one run, the landed config-2 world of 1,004,524 colliders; sensors riding on
   dynamic bodies; 16,777,216 rays a call; ms per call, the best of 5 blocks of 5 calls by device events; nh_sense writing t / t + body / full records,
   then nh_sense_rays, then nh_raycast -- the yardstick -- on the records nh_sense_rays wrote):
     4,096 cameras x 64 x 64 beams in 8 x 8 tiles     8.154 / 8.161 / 8.431     0.121     7.951
     the same pattern in row-major order              9.006 / 9.040 / 9.401     0.121     8.842
     256 lidars x 64 rings x 1,024 azimuths           2.809 / 2.816 / 2.957     0.114     2.831
   So the WALK is the cost: nh_sense takes what nh_raycast takes on the same rays (0.98 - 1.01 of its rate), whichever channels it writes, and materialising
   the rays costs 1.5 % on top.  What nh_sense saves is not time but the 1.07 GB of ray and hit records, the per-frame upload or the caller's own
   ray kernel, and one launch.  Pattern order is worth 10 % (tiles against rows).  DESIGN 10.25 has the table and the grid that lost.
   Not built: beams with a radius (sphere-cast sensors); different patterns within one call; per-beam time offsets (a rolling lidar); normals as a channel
   of their own (they are in `hits`); noise models and images beyond depth / ids; all-hits or first-k forms of a sensor; packet or shared-stack traversal;
   sensors on a partitioned world. */
typedef struct nh_Beam { float direction[3]; float range; } nh_Beam;                               /* 16 B: sensor-local direction; max_t of its ray */
typedef struct nh_Sensor { float position[3]; uint32_t body;                                        /* mount: a body index, or 0xffffffff = world frame */
                           float rotation[4];
                           uint32_t ignore_body; uint32_t reserved[3]; } nh_Sensor;                 /* 48 B; reserved is not read */
typedef struct nh_SenseOut { float* t; uint32_t* body; uint32_t* tag; nh_RayHit* hits; } nh_SenseOut;   /* DEVICE pointers, each count * beam_count long or NULL */
int nh_sense(nh_context* ctx, const nh_BodyData* bodies /* or NULL */, const nh_Sensor* sensors, uint32_t count, const nh_Beam* beams, uint32_t beam_count,
             const nh_SenseOut* out, uint32_t flags /* 0 or NH_RAY_ANY_HIT */);
int nh_sense_rays(nh_context* ctx, const nh_BodyData* bodies /* or NULL */, const nh_Sensor* sensors, uint32_t count, const nh_Beam* beams, uint32_t beam_count,
                  nh_Ray* rays /* count * beam_count */, uint32_t flags /* 0 */);

/* nh_overlap_wide and nh_penetration_wide: nh_overlap and nh_penetration for LARGE volumes -- an explosion radius, a large trigger volume, a client's area
   of interest, a vehicle-sized box.  nh_overlap gives one lane to a query, which is the right shape for a body-sized question and the wrong one for a
   volume that holds thousands of colliders: one lane then walks thousands of nodes.  Here the work of ONE query spreads over the GPU, as nh_region's does,
   with nh_overlap's exact predicates in place of the plane test -- so spheres and capsules can be asked, nothing is listed that only the conservative
   plane test would keep, and the penetration form exists.
   THE ANSWER, THE OUTPUT, THE ORDER AND THE CAPACITY RULE ARE nh_overlap's AND nh_penetration's, BYTE FOR BYTE: for the same queries on the same build or
   refit nh_overlap_wide writes exactly what nh_overlap writes and nh_penetration_wide exactly what nh_penetration writes -- `offsets`, the records, and
   every byte of `hits` behind the written prefix left untouched; COUNT ONLY with hits == NULL and capacity == 0; the CAPACITY prefix rule; offsets[count] =
   0xffffffff and no record for a true total of 2^32 - 1 or more; an invalid query counts 0; a capsule of half height 0 is the sphere query; `ignore_body`;
   a collider of a NaN pose is never listed.  Only the distribution of the work differs, and with it the time.
   Returns NH_ERR_INVALID in the cases and in the order of nh_overlap (before any nh_query_build, flags != 0, count >= 2^30, `queries` null or not 16-byte
   aligned, `offsets` null or not 4-byte aligned, `hits` null with capacity > 0 or not 16-byte aligned); count = 0 is a no-op that returns NH_OK.
   OBSERVERS like nh_overlap (note 9): no view export, no settling of deferred gravity, no still step turned into a full one, no change to nh_Counts.
   Everything is enqueued on the context's stream, except that a list call with a larger capacity than any before grows nh_overlap's sort scratch, and one
   with a larger count than any before nh_region's cursor word per query, each after a stream synchronise.  Layer masks: both run under that contract.
   THE CALLER CHOOSES THE CALL BY SIZE, as it chooses nh_region today; a batch that mixes body-sized and tile-sized volumes is the caller's to split (there
   is no dispatch by size inside nh_overlap: its flags != 0 refusal stands).  The lists feed nh_overlap_events and nh_overlap_bodies as nh_overlap's do.
   HOW: a work item is (query, entry node) over the entry nodes of nh_region.  A lane tests the entry's box against the query's padded world
   AABB -- nh_overlap's own node test; for each item that is left a wave sweeps the entry's contiguous leaves, 64 a step, with the exact predicate of the
   shape pair, the query decoded once per item at a wave-uniform address.  Counts are ballots summed by one integer atomic per item; the list pass
   reserves slots of the query's segment by one atomic per step, and nh_overlap's sort and gathers make the bytes: no atomic decides a byte of the output.
   Capsules of nonzero half height run in launches of their own, as in nh_overlap.
   Timing labels: q_wide_count, q_wide_count_capsule, q_wide_list, q_wide_list_capsule, then nh_overlap's own.
   MEASURED (tools/overlap_wide_rates.py -> profiles/overlap_wide_rates.log; one MI355X, one run, the landed config-2 world of 1,004,524 colliders of about
   1.5 units and 9,823 entry nodes; ms per call, the best of 5 blocks of 20 calls by device events -- nh_overlap one call a block from 20 ms up; the
   count-only call / it followed by the exactly sized list call; every pair wrote the same bytes):
                                                                          nh_overlap_wide        nh_overlap            nh_region, the same boxes
     (a) one box that is the world's AABB, 1,004,524 records               0.150 /  0.681     1783.3 / 5831.8           0.149 / 0.677
     (d) 4,096 cubes of one tile's size (267 units), 29,798,281 records    1.102 /  7.014      33.50 / 109.73           1.558 / 8.342 (170 records more)
     4,096 spheres of radius 1.5, 8,192 records                            0.377 /  1.208      0.059 /   0.222
     4,096 spheres of radius 6, 84,418 records                             0.389 /  1.267      0.179 /   0.610
     4,096 spheres of radius 12, 244,564 records                           0.411 /  1.344      0.391 /   1.248
     4,096 spheres of radius 24, 861,337 records                           0.435 /  1.478      1.066 /   3.335
     4,096 spheres of radius 96, 12,444,142 records                        0.729 /  3.684      12.02 /  38.15
     4,096 spheres of radius 267, 89,800,260 records                       2.137 / 16.436      82.16 / 259.98
     (d) through nh_penetration_wide / nh_penetration                      1.100 /  6.978      33.49 / 109.89
   WHICH CALL FOR WHICH QUESTION: the two cross at a radius of about 12 units on that world -- a volume eight bodies across, 60 colliders a query.  Below it
   nh_overlap: the wide call pays a node test per (query, entry node) whatever the size, 0.38 ms for 4,096 queries x 9,823 entries.  Above it nh_overlap_wide.
   nh_region stays the call for volumes given by planes; for a box it is no faster than the exact test (d).
   Not built: a dispatch by size inside nh_overlap; wide forms of nh_distance and nh_recover; queries on a partitioned world, as before. */
int nh_overlap_wide(nh_context* ctx, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets /* count + 1 */, nh_OverlapHit* hits,
                    uint32_t capacity, uint32_t flags /* 0 */);
int nh_penetration_wide(nh_context* ctx, const nh_OverlapQuery* queries, uint32_t count, uint32_t* offsets /* count + 1 */, nh_PenetrationHit* hits,
                        uint32_t capacity, uint32_t flags /* 0 */);

/* TRIGGER EVENTS -- nh_overlap_bodies and nh_overlap_events: what ENTERED and what LEFT each of `count` overlap volumes since the last step, per collider
   or per body, computed on the device from two lists.  A trigger volume, an explosion radius or a client's area of interest is listed every step by
   nh_overlap or nh_region; what a caller acts on is the difference between this step's list and the last one's, and for a compound body one event, not
   one per collider.
   A LIST (nh_HitList: a host struct of DEVICE pointers) is what a list call of nh_overlap or nh_region wrote, or what these two calls write: `offsets`
   (count + 1 words), `hits`, and the `capacity` that call was given.  Both calls read lists only -- not the hierarchy, not the colliders, not the layer
   filter: they are not query calls of the filter contract above, and a list stays usable after any number of builds, refits and steps.
   PRESENT SEGMENTS: segment i of an input list is present iff offsets[i+1] <= capacity and offsets[count] != 0xffffffff -- nh_overlap's own written-prefix
   rule, so the present segments are a prefix and the caller sees from its own offsets where a list was cut short.  No record at or beyond `capacity` is
   ever read, whatever the offsets hold (a pair offsets[i+1] < offsets[i] is an absent segment); lists that no list call wrote give unspecified records
   but never an access outside the arrays.
   nh_overlap_bodies -- ONE RECORD PER BODY: for every present segment of `in`, one record per distinct body in it: the record of the body's lowest
   COMBINED collider index in the segment, copied whole (body, collider, shape, tag); the records of a segment in ascending body.  An absent segment
   counts 0.  (The input's segments must be in nh_overlap's order, ascending combined collider index: the sort is stable and that order decides the tie.)
   nh_overlap_events -- WHAT ENTERED AND WHAT LEFT: the IDENTITY of a record is (shape, collider) with flags = 0, and both inputs are in nh_overlap's
   order; with NH_EVENTS_BY_BODY it is `body`, and both inputs are outputs of nh_overlap_bodies.
     - a volume's segments are read only when both its `cur` and its `prev` segment are present (or prev == NULL); any other volume gives no event and
       counts 0 in both outputs;
     - `entered` gets, for volume i, the records of cur's segment whose identity is not in prev's segment, copied from cur in cur's order;
     - `left` gets the records of prev's segment whose identity is not in cur's segment, copied from prev in prev's order: `body` and `tag` are those of
       the step the collider was last seen in;
     - prev == NULL is the FIRST FRAME: `entered` equals cur's present segments and `left` is empty.
   OUTPUT (`out`, `entered`, `left`, each on its own) follows nh_overlap's rules word for word: offsets[0 .. count] by the exclusive scan of the per-volume
   counts, always complete; COUNT ONLY with hits == NULL and capacity == 0; the records of volume i are written iff offsets[i+1] <= capacity, and every byte
   behind the written prefix is left untouched.  An output's total is at most its input's, so the overflow marker never appears in an output.  Outputs
   must not alias inputs or each other.
   Returns NH_ERR_INVALID before any nh_query_build, for unknown flags, for count >= 2^30, and (count > 0) for a NULL cur, in, out, entered or left, for
   `offsets` null or not 4-byte aligned, for `hits` null with capacity > 0 or not 16-byte aligned, and where the input capacities add up to 2^32 - 2 or
   more; count = 0 is a no-op that returns NH_OK (nh_overlap's order: before the lists are looked at).
   OBSERVERS (note 9): no view export, no settling of deferred gravity, no still step turned into a full one, no change to nh_Counts.  Everything is
   enqueued on the context's stream, except that larger input capacities than any before grow the library's scratch after a stream synchronise: 4.5 B of
   flag and scan words (one word, scanned in place) per record of in.capacity or prev.capacity + cur.capacity, and for nh_overlap_bodies nh_overlap's own sort scratch (~24 B per record
   of in.capacity).  nh_destroy frees both.
   HOW: the work item is the RECORD, so one region of a million records spreads over the GPU.  A record finds its volume by a binary
   search over `offsets` (the last i with offsets[i] <= r: empty segments are stepped over) and its identity in the other list's segment by a second one;
   the exclusive scan of the per-record flags gives the compacted position and the output's offsets[i] = scan[input offsets[i]].  No atomics: the bytes
   are deterministic.  nh_overlap_bodies sorts (segment, body) keys with the library's stable radix sort, flags the first record of each run, scans and
   compacts.
   Timing labels: q_bodies_prefix, q_bodies_keys, q_bodies_flag, q_bodies_offsets, q_bodies_compact; q_events_flag, q_events_offsets, q_events_compact;
   the sort's and the scan's own between them.
   MEASURED (tools/events_rates.py -> profiles/events_rates.log; one MI355X, one run, the landed config-2 world of 1,004,524 colliders; two lists per case,
   the volumes at A and moved by one body's size; ms per call, the best of 5 blocks of 10 calls by device events; in brackets the ratio to the list call --
   count + exactly sized list -- that produced the input):
                                                                  list call   nh_overlap_bodies   nh_overlap_events, by collider / by body
     (1) 1 M sphere queries of a box's size, 2,185,844 records      2.545       0.359 (0.141)       0.140 (0.055) / 0.141 (0.055)
     (2) 4,096 cubes of a tile's size, 29,776,132 records           7.994       3.997 (0.500)       2.264 (0.283) / 2.294 (0.287)
     (3) one region that is the world, 1,004,524 records            0.675       0.170 (0.251)       0.062 (0.092) / 0.063 (0.094)
   The bodies' time is its radix sort's (3.25 of 4.0 ms in (2): six passes for 32 + bits(count) = 45 key bits); the events' time is the flag kernel's two
   binary searches (1.86 of 2.26 ms in (2)).  In this world every collider is its own body, so (1)'s body list is as long as its input.
   Not built: a stay list (it is `cur` minus `entered`); events for nh_penetration's 32-byte records; events for the movers' touch records, which are
   nh_Touch, not nh_OverlapHit. */
typedef struct nh_HitList { uint32_t* offsets /* count + 1 */; nh_OverlapHit* hits; uint32_t capacity; uint32_t reserved; } nh_HitList;   /* host struct, DEVICE pointers */
enum { NH_EVENTS_BY_BODY = 1u };
int nh_overlap_bodies(nh_context* ctx, uint32_t count, const nh_HitList* in, const nh_HitList* out, uint32_t flags /* 0 */);
int nh_overlap_events(nh_context* ctx, uint32_t count, const nh_HitList* prev /* or NULL */, const nh_HitList* cur, const nh_HitList* entered,
                      const nh_HitList* left, uint32_t flags /* 0 or NH_EVENTS_BY_BODY */);

/* CONTACT EVENTS -- nh_contact_pairs, nh_contact_events and nh_step_contact_pairs: which body pairs touch, how hard, and which pairs BEGAN and STOPPED
   touching since the last step, computed on the device.  The solver's contact list has one record per contact POINT, in collider-tag order; what a game,
   a robot or a recorder acts on is one record per BODY PAIR and the difference of two steps' records.
   nh_contact_pairs -- ONE RECORD PER UNORDERED BODY PAIR of a contact list (nh_ContactList: a host struct of DEVICE pointers; the list is the first
   min(*count, capacity) contacts, or `capacity` of them with count == NULL; nothing at or beyond `capacity` is ever read), sorted ascending by (lo, hi).
   The rules are exact -- a host oracle reproduces every byte (tests/hostoracle/hostcontacts.cpp):
     - a contact's pair is lo = min(a, b), hi = max(a, b); the contact is FLIPPED when its `a` is not lo, and then contributes its impulse and its
       normal with the sign inverted (exact), so that every vector of a record has the sense lo -> hi; a == b is a pair like any other;
     - a RUN is a maximal stretch of consecutive contacts of the list with the same (lo, hi) -- contacts are in tag order, so a collider pair's points
       are one run.  A run's sums start at +0 and take its contacts left to right in fp32, a contact's normal impulse being
       (ix * nx + iy * ny) + iz * nz (the library is built with -ffp-contract=off);
     - a pair's `impulse` and `normal_impulse` start at +0 and take its runs' sums in list order.  This TWO-LEVEL order is the specification, not an
       implementation detail: it is what lets the runs be reduced before the sort.  Sums with a NaN in them are NaN, of unspecified payload;
     - the DEEPEST contact: start with the pair's first contact and replace iff penetration > best, in list order -- ties keep the lower index, a NaN
       penetration never replaces anything, and one that comes first is never replaced.  position, penetration, normal (same sense) and `deepest`,
       its index in the list, are that contact's;
     - `first` is the lowest contact index of the pair and `count` the number of its contact points.
   `impulses` holds one nh_CachedContactImpulse per contact (`unused` is not read), or is NULL: every impulse is zero.  `body_count` promises that every
   body index of the list is below it and sizes the sort keys -- lo << bits | hi, sorted over only the 8-bit passes that 2 x bits(body_count - 1) need;
   0 = unknown, all 64 bits.  A list that breaks the promise gives unspecified records, never an access outside the arrays.
   OUTPUT (nh_PairList; `out`, `began`, `ended`, each on its own): *count always receives the true number of records; the records are written iff that
   number is <= capacity -- all or none, as nh_overlap does with a segment -- every byte behind the written records is left untouched, and so is every
   byte of `pairs` when nothing is written.  COUNT ONLY: pairs == NULL and capacity == 0.
   nh_contact_events -- THE DIFFERENCE OF TWO PAIR LISTS, both outputs of nh_contact_pairs / nh_step_contact_pairs (unique ascending keys).  A list is
   PRESENT iff its *count <= capacity.  If `cur` or a non-NULL `prev` is absent both outputs count 0.  `began` gets cur's records whose (lo, hi) is not
   in prev, copied whole from cur in cur's order; `ended` gets prev's records that are not in cur, copied from prev: they carry the values of the last
   step the pair touched.  prev == NULL is the FIRST FRAME: `began` equals cur and `ended` is empty.  Outputs must not alias inputs or each other.
   nh_step_contact_pairs -- THE SAME FOR THE WORLD'S OWN LAST STEP, with no download: it (1) calls nh_export_views(NH_VIEW_CONTACTS | NH_VIEW_CACHE) -- a
   no-op after a full step; it has that call's effect on speculation (note 9) and no other, so nh_Counts.still_steps / still_replays are those of a world
   that calls nh_export_views at the same places --, (2) takes the contact and the cache count from the context's device counters, clamped to the two
   capacities, (3) finds each contact's cache entry by (tag, feature) -- the binary search nh_read_cached_impulses does; a contact without an entry has a
   zero impulse -- and (4) runs nh_contact_pairs' pipeline on the result.  `contacts` and `cache` are the structs of the step.  It changes no body state,
   no counter of nh_Counts and nothing a later step computes.  Call it after nh_advance, or after nh_step returns: the cache then holds the impulses the
   step solved, as world-space vectors (nudge.cpp:4857-4884).  BETWEEN nh_collide AND nh_write_cached_impulses THE CACHE IS STILL LAST STEP'S: there the
   impulses are the warm-start values of the contacts that persist and zero for the new ones, not what this step will solve.
   Returns NH_ERR_INVALID, before any launch, for flags != 0; for a NULL ctx, in, out, cur, began, ended, contacts or cache; for a pair list whose `count`
   is NULL or not 4-byte aligned, whose `pairs` is NULL with capacity > 0 or not 16-byte aligned; for a contact list with capacity > 0 and a NULL data or
   bodies (the step-bound call: any NULL array of either struct), for `data` or `impulses` not 16-byte or `bodies` not 8-byte aligned; and for any capacity
   of 2^31 or more.  A contact list of capacity 0 is the empty list: *out->count = 0 and no other launch.  nh_contact_pairs and nh_contact_events read
   lists only and need no nh_query_build; like the trigger events they are no entry points of the step (note 9).
   SCRATCH is the context's: per contact of the largest `capacity` seen 92 B (a 64-byte run record, two 8-byte keys, two 4-byte values, one flag word), per
   pair of the largest prev.capacity + cur.capacity seen 4 B (one flag word, scanned in place), and 514 KB for the sort.  It grows after a stream
   synchronise, only when a capacity exceeds every earlier one; nh_destroy frees it.  Everything else is enqueued on the context's stream.
   HOW: flag the run heads, scan, one lane per run head walks its run and writes one partial record; the stable radix sort orders the run
   keys; flag the pair heads, scan, one lane per pair head merges its runs in order and writes the record with four 16-byte stores.  Events: per record a
   binary search in the other list, a scan, a copy.  No atomics: the bytes are a function of the input alone.  A run or a pair with very many members --
   one huge compound body resting on another -- is walked by ONE lane: correct and slow; there is no second path.
   Timing labels: cp_run_flag, cp_runs, cp_runs_lookup, cp_pair_flag, cp_merge; cp_ev_flag, cp_ev_compact; the sort's and the scan's own between them.
   MEASURED (tools/contact_events_rates.py -> profiles/contact_events_rates.log; one MI355X, one run, the landed config-2 world of 1,004,401 bodies, 4,017,582
   contacts and 1,004,400 body pairs; ms per call, the best of 5 blocks of 10 calls by device events; in brackets the price in steady steps of the same run):
     nh_step(1), still steps / full steps (option no_still)                    0.280 / 0.497
     nh_contact_pairs on the exported views (count only)                       0.309 (0.279)
     nh_step_contact_pairs, views current                                      0.374
     nh_step_contact_pairs behind every step, by difference: after a still step, view export included / after a full step     0.545 (1.95) / 0.378 (0.76)
     nh_contact_events on two consecutive steps' lists (0 began, 0 ended) / the first frame            0.084 / 0.041
     nh_overlap_bodies on one list of 1,004,524 records, the nearest existing sort-and-compact         0.168
   The sort of the 1 M run keys -- five passes for 2 x 20 key bits -- is 0.19 of the 0.31 ms, the run walk 0.09 (0.14 with the cache search), the merge 0.035; the events' time
   is the flag kernel's binary searches (0.07).  The pair list equals the host oracle byte for byte.  No bar was set in advance.
   Not built: a "stayed" list (it is `cur` minus `began`); per-body reductions; a threshold filter (threshold `normal_impulse` yourself). */
typedef struct nh_ContactPair {      /* 64 bytes */
	uint32_t lo, hi;             /* the two bodies, lo <= hi */
	uint32_t first, count;       /* lowest contact index of the pair in the input list; number of contact points */
	float impulse[3];            /* sum of the contacts' impulse vectors, in the sense lo -> hi */
	float normal_impulse;        /* sum of dot(impulse_i, normal_i) */
	float position[3]; float penetration;   /* of the DEEPEST contact */
	float normal[3];             /* of that contact, same sense */
	uint32_t deepest;            /* its index in the input list */
} nh_ContactPair;
typedef struct nh_ContactList {      /* host struct, DEVICE pointers */
	const nh_Contact* data; const nh_BodyPair* bodies;
	const nh_CachedContactImpulse* impulses;   /* one per contact, or NULL: all zero */
	const uint32_t* count;       /* device word, or NULL: `capacity` is the count */
	uint32_t capacity;           /* host bound: nothing at or beyond it is ever read; *count is clamped to it */
	uint32_t body_count;         /* every body index < body_count (sizes the sort keys), or 0: unknown, full 32 bits */
} nh_ContactList;
typedef struct nh_PairList { uint32_t* count /* device word */; nh_ContactPair* pairs /* 16-byte aligned */; uint32_t capacity; uint32_t reserved; } nh_PairList;

int nh_contact_pairs(nh_context* ctx, const nh_ContactList* in, const nh_PairList* out, uint32_t flags /* 0 */);
int nh_contact_events(nh_context* ctx, const nh_PairList* prev /* or NULL */, const nh_PairList* cur,
                      const nh_PairList* began, const nh_PairList* ended, uint32_t flags /* 0 */);
int nh_step_contact_pairs(nh_context* ctx, const nh_ContactData* contacts, const nh_ContactCache* cache,
                          uint32_t body_count, const nh_PairList* out, uint32_t flags /* 0 */);

/* BODY IMPULSES -- nh_body_impulses, nh_impulse_sums, nh_blast_impulses and nh_touch_impulses: push, blast and wake bodies on the device.  The way back from
   the queries into the simulation: a list of impulse records (nh_ImpulseList: a host struct of DEVICE pointers), written by the caller's own kernel or by one
   of the two generators below, is summed per body in an order that does not depend on the hardware and added to the bodies' momentum, with nothing downloaded:
   "refit, recover, walk_touched, touch_impulses, body_impulses, step" and "overlap_wide, overlap_bodies, blast_impulses, body_impulses, step" are frames that
   never leave the device.  The rules are exact -- a host oracle reproduces every byte (tests/hostoracle/hostimpulse.cpp):
     - LIST: the first min(*count, capacity) records, or `capacity` of them with count == NULL; nothing at or beyond `capacity` is ever read;
     - a record is VALID iff 0 < body < bodies->count.  Body 0 is the static world (nudge.cpp:3663, 3954) and takes no impulse; NH_IMPULSE_NO_BODY is
       invalid by the same test;
     - a record's PAIR (L, T): L is `impulse`.  With NH_IMPULSE_AT_CENTRE `point` is not read and T = (+0, +0, +0); otherwise r = point -
       transforms[body].position componentwise and T = (r.y * J.z - r.z * J.y, r.z * J.x - r.x * J.z, r.x * J.y - r.y * J.x) in fp32 -- two products and
       one subtraction per component, no contraction (the library is built with -ffp-contract=off);
     - a RUN is a maximal stretch of consecutive valid records of one body; an invalid record ends a run and belongs to none.  A run's six sums start
       at +0 and take its records left to right;
     - a BODY's six sums start at +0 and take its runs' sums in list order -- the stable sort's order.  This TWO-LEVEL order is the specification, as it
       is for the contact events: it is what lets the runs be reduced before the sort.  Sums with a NaN in them are NaN, of unspecified
       payload.
   nh_impulse_sums -- ONE nh_ImpulseSum PER DISTINCT VALID BODY, ascending by body; `count` is the body's number of records.  The output follows
   nh_contact_pairs' contract: *count always receives the true number; the records are written iff that number is <= capacity -- all or none -- every byte
   behind the written records is left untouched; sums == NULL with capacity 0 counts only.  It reads bodies->transforms and bodies->count and writes no
   body state; it is no entry point of the step (note 9).
   nh_body_impulses -- THE SAME PIPELINE, but the lane of each distinct body loads the body's nh_BodyMomentum whole, adds
       velocity[c]       += linear[c] * mass_inverse                                  (per component: one product, one sum)
       angular_velocity  += W . angular,  W = the world-space inverse inertia of (rotation, inertia_inverse), six terms as the solver computes them;
                            x = (W.xx * Tx + W.xy * Ty) + W.xz * Tz,  y = (W.xy * Tx + W.yy * Ty) + W.yz * Tz,  z = (W.xz * Tx + W.yz * Ty) + W.zz * Tz
   and stores the record whole, unused0 and unused1 with the bits they had.  With NH_IMPULSE_WAKE the lane also stores idle_counters[body] = 0: the next
   nh_collide then wakes the body's whole set, as the reference does (nudge.cpp:3669-3672, 3960-3971).  Without the flag no idle counter is written: a
   sleeper keeps the velocity it was given until something wakes it, exactly as if the caller had written the momentum array.  Bodies without a valid record
   are not touched.
   RELATION TO THE STEP: nh_body_impulses writes momentum, so it first completes pending work (as nh_halo_unpack does).  With NH_IMPULSE_WAKE it then
   does on the host everything nh_bodies_changed does, unconditionally -- whether anybody was asleep is known only on the device.  Without the flag it
   leaves speculation to the device-side checks of note 9, as for momentum written from outside: the still step whose checks fail is replayed.
   nh_blast_impulses -- ONE RECORD IN, ONE RECORD OUT: `hits` is a list of nh_overlap, nh_overlap_wide, nh_region or nh_overlap_bodies for `count` volumes;
   segment i belongs to blasts[i].  Record j of the list gives out[j] for every j < min(offsets[count], hits->capacity); its segment is found by binary
   search in `offsets` (an index past every offset belongs to the last blast).  With p = transforms[hit.body].position: r = p - centre,
   d = sqrtf((r.x * r.x + r.y * r.y) + r.z * r.z), s = strength * (1.0f - falloff * (d / radius)).  If hit.body == 0, hit.body >= bodies->count or !(s > 0)
   the record is NH_IMPULSE_NO_BODY with all other words 0 -- there is no compaction.  Otherwise dir = d > 0 ? r / d : (0, 1, 0) (three plain divisions),
   impulse = dir * s, point = p, flags = NH_IMPULSE_AT_CENTRE, body = hit.body.  Plain `/` and sqrtf are correctly rounded on the host and on the device.
   A compound body gets one record per COLLIDER the volume touches: one record per BODY is the caller's nh_overlap_bodies first.
   nh_touch_impulses -- INTEGRATION's pushing recipe, word for word, on what a _touched mover wrote for `count` movers with `k` slots each: slot j of mover
   i gives out[i * k + j], a real record iff j < min(counts[i], k), hit.shape != NH_SHAPE_NONE, hit.body != 0, hit.t > 0, phase < 32 with
   (pushes[i].phases >> phase) & 1, and the approach a = -((d.x * n.x + d.y * n.y) + d.z * n.z) > 0 (d the touch's `direction`, n its hit.normal, the
   sign bit inverted).  Then m = mass_over_dt * a, or max_impulse where that is smaller; impulse[c] = -n[c] * m; point[c] = origin[c] + d[c] * t; flags
   are the push's, body = hit.body.  Otherwise NH_IMPULSE_NO_BODY with all other words 0.  Touch slots at or behind counts[i] are never read.
   Neither generator reads the query tree or obeys the layer filter; neither is an entry point of the step.
   Returns NH_ERR_INVALID, before any launch, for a NULL ctx, bodies, in or out (generators: blasts / hits / pushes / counts / touches / out with
   count > 0); for unknown flags; for `records` NULL with capacity > 0 or not 16-byte aligned; for a count word that is not 4-byte aligned; for a capacity of
   2^31 or more; for NULL body arrays with bodies->count > 0 (nh_impulse_sums and nh_blast_impulses: transforms; nh_body_impulses: all four); for a sum
   list that breaks nh_PairList's rules.  Capacity 0 is the empty list: nh_impulse_sums sets *count = 0, nh_body_impulses completes pending work and
   otherwise does nothing.
   SCRATCH is the context's: per record of the largest `capacity` seen 60 B (a 32-byte run record, two 8-byte keys, two 4-byte values, one flag word,
   scanned in place), and 514 KB for the sort.  It grows after a stream synchronise, only when a capacity exceeds every earlier one; nh_destroy frees
   it.  Everything else is enqueued on the context's stream.
   HOW: flag the run heads, scan, one lane per run head walks its run with two 16-byte loads per record and writes one partial sum; the
   stable radix sort orders the run keys over only the 8-bit passes that bits(bodies->count - 1) need; flag the body heads, scan, one lane per body head
   merges its runs in order and either writes the sum with two 16-byte stores or applies it.  No atomics: the bytes are a function of the input alone.  A
   body with very many runs is merged by ONE lane: correct and slow; there is no second path.
   Timing labels: bi_run_flag, bi_runs, bi_body_flag, bi_sums, bi_apply; bi_blast, bi_touch; the sort's and the scan's own between them.
   MEASURED (tools/body_impulses.py -> profiles/body_impulses.log; one MI355X, one run, the landed config-2 world of 1,004,401 bodies and 4,017,582 contacts; ms per
   call, the best of 5 blocks of 10 calls by device events):
     nh_step(1), still steps, before / after the series                                       0.282 / 0.274   (profiles/contact_events_rates.log: 0.280, median 0.291)
     nh_impulse_sums / nh_body_impulses, one record per body in body order (1,004,400 records)  0.163 / 0.173   (with NH_IMPULSE_WAKE 0.173)
     nh_impulse_sums / nh_body_impulses, four records per body, shuffled (4,017,600 records)   0.538 / 0.554
     nh_overlap_wide, nh_overlap_bodies, nh_blast_impulses, nh_impulse_sums: one blast over 6,329 colliders, 6,216 bodies pushed     0.207
     nh_contact_pairs on the same world's exported views, for scale                             0.306
   The sort of the run keys -- three passes for 20 key bits -- is 0.12 of the 0.16 ms (0.27 of the 0.54 for 4 M runs of one record), the run walk 0.023 (0.124), the
   apply 0.027 (0.105: a gather of four scattered partial sums per body); the blast chain is launch-bound (some twenty launches of 6 - 7 us).  The sums equal the host
   oracle byte for byte on both lists.  No bar was set in advance.
   Not built: velocity-change records; torque-only records; forces over time; impulses on partitioned worlds; the `namespace nudge` extension; a second
   path for huge bodies. */
typedef struct nh_BodyImpulse { float point[3]; uint32_t body; float impulse[3]; uint32_t flags; } nh_BodyImpulse;   /* 32 B, 16-byte aligned */
enum { NH_IMPULSE_AT_CENTRE = 1u };          /* record flag: `point` is not read, the record has no angular part */
#define NH_IMPULSE_NO_BODY 0xFFFFFFFFu       /* a record that applies to nobody (what the generators write for "nothing here") */
typedef struct nh_ImpulseList { const nh_BodyImpulse* records; const uint32_t* count /* device word, or NULL: capacity is the count */; uint32_t capacity; uint32_t reserved; } nh_ImpulseList;
typedef struct nh_ImpulseSum { uint32_t body; uint32_t count; float linear[3]; float angular[3]; } nh_ImpulseSum;   /* 32 B */
typedef struct nh_ImpulseSumList { uint32_t* count /* device word */; nh_ImpulseSum* sums /* 16-byte aligned */; uint32_t capacity; uint32_t reserved; } nh_ImpulseSumList;
enum { NH_IMPULSE_WAKE = 1u };               /* call flag */
typedef struct nh_Blast { float centre[3]; float radius; float strength; float falloff; uint32_t reserved[2]; } nh_Blast;   /* 32 B */
typedef struct nh_Push { float mass_over_dt; float max_impulse; uint32_t phases /* bit p: touches of phase p push */; uint32_t flags /* 0 or NH_IMPULSE_AT_CENTRE */; } nh_Push;   /* 16 B, one per mover */

int nh_impulse_sums (nh_context* ctx, const nh_BodyData* bodies, const nh_ImpulseList* in, const nh_ImpulseSumList* out, uint32_t flags /* 0 */);
int nh_body_impulses(nh_context* ctx, const nh_BodyData* bodies, const nh_ImpulseList* in, uint32_t flags /* 0 or NH_IMPULSE_WAKE */);
int nh_blast_impulses(nh_context* ctx, const nh_BodyData* bodies, const nh_Blast* blasts, uint32_t count, const nh_HitList* hits, nh_BodyImpulse* out, uint32_t flags /* 0 */);
/* (nh_touch_impulses is declared behind nh_Touch, with the movers' _touched forms) */

/* ---- fast bodies: sweep the colliders that travel far along their velocity, stop their bodies at the hit ------------------------------------------
   The engine steps discretely, as the reference does, and the reference has no sweep: a body that travels further in one step than a thin obstacle is
   deep leaves no contact and passes through it (a ball of radius 0.25 at 240 m/s and 1/120 s moves 2 m a step: a wall 0.1 thick never sees it).
   nh_sweep takes the casts from the bodies' own state and nh_sweep_limit applies the result, with no download between them:
       nh_step, nh_query_refit, nh_sweep, nh_sweep_limit          -- every step; a tunnelling guard that never leaves the device
   Both are opt-in: no other call changes a byte.
   THE SWEEP OF A COLLIDER.  For the combined collider index c (boxes first, then spheres) take its record in the tree of the last nh_query_build /
   nh_query_refit: world position p_c, rotation q_c, half extents h (a sphere: its radius in h.x), body b, tag.  bodies->transforms and bodies->momentum
   are read as the stream has them.  In fp32, exactly nudge_amd/csrc/nh_query.h ("fast bodies"), only + - * and compares, no contraction:
       r = p_c - transforms[b].position                                                     (componentwise)
       u = velocity + (w.y * r.z - w.z * r.y, w.z * r.x - w.x * r.z, w.x * r.y - w.y * r.x)   (w the angular velocity: two products, one subtraction, one sum)
       d = u * time_step
       m = the smallest of the three half extents (a sphere: the radius);  s = min_travel * m
   SELECTED iff 0 < b < bodies->count and ((d.x * d.x + d.y * d.y) + d.z * d.z) > s * s.  A NaN anywhere makes the comparison false: body 0, a collider of
   a body that does not exist (a NaN pose) and non-finite momentum are never swept; the state of a body >= bodies->count is not read.
   THE CAST of a selected collider is a 64-byte record.  A box gives the nh_BoxCast { origin = p_c, max_t = 1.0f, direction = d, ignore_body = b,
   rotation = q_c, size = h * core (one product per component), reserved = 0 }; a sphere the nh_CapsuleCast { the same head, rotation = (0, 0, 0, 1),
   radius = h.x * core, half_height = 0, reserved = 0 } -- by nh_capsulecast's own contract nh_spherecast's ball of that radius.  Nothing rotates during
   a sweep, and other dynamic bodies stand where the tree has them.
   `core`, in [0, 1]: only the inner `core` share of the shape is swept, because touching counts in the cast predicates: a body that rests on or slides
   along the ground would start every sweep of its full shape in contact at t = 0, while its core does not.
   nh_sweep lists the selected colliders in ascending combined index -- boxes before spheres.  counts[0] / counts[1] ALWAYS receive the true numbers of
   selected boxes / spheres.  Entry i writes colliders[i] (the combined index), casts[i] (the record above) and hits[i]: EXACTLY the 32 bytes nh_boxcast
   writes for casts[i] with flags 0 under the context's filter -- for a sphere entry nh_capsulecast's bytes, which are nh_spherecast's for the ball
   (head, radius).  That identity is the whole contract of `hits`: start overlaps of the core, the reach rule, ties and NaN handling are the casts' own
   rules.  Under NH_FILTER_PER_QUERY the query is the COLLIDER: masks[c] is read by combined index (boxes + spheres words in all).
   A NULL channel costs nothing; with hits == NULL nothing walks the tree.  The channels are written iff counts[0] + counts[1] <= capacity -- all or none,
   and no byte behind the written records is touched (nh_contact_pairs' rule); capacity == 0 with all three channels NULL counts only.  A tree of zero
   colliders writes counts 0, 0.
   nh_sweep returns NH_ERR_INVALID, before any launch and writing nothing: before any nh_query_build; for a NULL ctx, bodies, params, list or
   list->counts; for bodies->transforms or bodies->momentum NULL with bodies->count > 0; for counts / colliders not 4-byte or casts / hits not 16-byte
   aligned; for flags != 0; for capacity >= 2^31; for a channel given with capacity 0; for time_step, min_travel or core not finite, min_travel or core
   negative, or core > 1.
   An OBSERVER like nh_sense (note 9): no view export, no settling of deferred gravity, no still step turned into a full one, no change to nh_Counts.  It
   never waits for a count: its kernels read the device counts, its grids are sized from `capacity` and the tree and stride.  It allocates one flag /
   scan word per collider of the tree, on first use or when the tree has grown, behind a stream synchronise (as nh_overlap's scratch).
   HOW: one lane per collider computes the rule and writes a flag; the library's scan gives the places; a gather writes `colliders` and
   `casts`.  Then two walk kernels, one per shape so that a wave is homogeneous, over the entries [0, counts[0]) and [counts[0], total), one lane per ENTRY:
   the lane finds its collider by binary search in the scan words, rebuilds the cast in registers, and answers it with nh_boxcast's / nh_spherecast's own
   per-cast body.  No cast record is read back.  Compacting before the walk is the point: in a world at rest with a few thousand fast bodies a
   lane-per-collider walk would run waves with one live lane.  Timing labels: q_sweep_flag, q_sweep_gather, q_sweep_box, q_sweep_ball.
   nh_sweep_limit reads counts, colliders and hits of a list nh_sweep filled (casts is not read; a total above capacity means nothing was written and
   nothing is read).  The body of entry i is that of collider colliders[i] in the tree, as nh_sweep saw it.  An entry LIMITS iff its hit is a real one
   (shape != NH_SHAPE_NONE) with t > 0; a core that starts in overlap (t == 0) limits nothing -- the body is already deep inside, and contacts are what
   frees it.  f_b = the smallest such t over body b's entries, 1.0f when none limits.  For every body with f_b < 1 ONE lane loads its nh_BodyMomentum's
   first 16 bytes, multiplies velocity[c] *= f_b (three products) and stores them; every other word keeps its bits: the angular velocity and the idle counter are
   not written.  factors[i], if given, receives f of entry i's body (1.0f for an entry that names no collider of the tree or no body).  The minimum of
   non-negative floats does not depend on the order (an atomic min on the bit patterns): the bytes are a function of the input alone.  The work is
   proportional to the list: the per-body words (8 B per body of bodies->count, allocated as above) are never cleared, the list's own entries set the
   ones they use.  Timing labels: q_limit_init, q_limit_min, q_limit_apply.
   RELATION TO THE STEP: exactly nh_body_impulses' without NH_IMPULSE_WAKE -- it completes pending work first, then leaves speculation to the device-side
   checks of note 9.  Returns NH_ERR_INVALID for a NULL ctx, bodies, list or list->counts, before any nh_query_build, for flags != 0, for
   bodies->momentum NULL with bodies->count > 0, for the alignments above (factors: 4 bytes), for capacity >= 2^31 and for capacity > 0 with colliders or
   hits NULL.  Capacity 0 completes pending work and otherwise does nothing.
   WHAT THIS BUYS: the limited body's next nh_advance ends with its core touching the obstacle, and the step after that finds an ordinary contact, at
   a depth of at most (1 - core) of the shape.  WHAT IT COSTS: the clamped share of the momentum is gone; the reference's contacts are inelastic, so
   against static geometry nothing else is lost.
   MEASURED: NOT MEASURED YET (tools/fast_bodies.py -> profiles/sweep_rates.log has not been run on a GPU; no bar is set in advance).
   Not built: rotation during the sweep; the coming step's gravity in d (2.7 mm per step squared at 60 Hz); sweeps relative to other moving bodies;
   restoring the speed after the impact step; speculative contacts; partitioned worlds. */
typedef struct nh_SweepParams { float time_step; float min_travel; float core; uint32_t reserved; } nh_SweepParams;      /* 16 B */
typedef struct nh_SweepList {
    uint32_t* counts;      /* device, 2 words, always written: selected boxes, selected spheres */
    uint32_t* colliders;   /* device, capacity words or NULL: combined indices, ascending */
    nh_BoxCast* casts;     /* device, capacity x 64 B or NULL: the records above */
    nh_RayHit* hits;       /* device, capacity x 32 B or NULL */
    uint32_t capacity;
    uint32_t reserved;
} nh_SweepList;
int nh_sweep(nh_context* ctx, const nh_BodyData* bodies, const nh_SweepParams* params, const nh_SweepList* list, uint32_t flags /* 0 */);
int nh_sweep_limit(nh_context* ctx, const nh_BodyData* bodies, const nh_SweepList* list, float* factors /* device floats, capacity, or NULL */, uint32_t flags /* 0 */);

/* ---- joints: ball, distance and hinge joints solved on the device -------------------------------------------------------------------------------------
   The reference has no joints; its sample says where a caller's own constraints go: "for (i < iterations) { nudge::apply_impulses(...); NOTE: Custom
   constraint impulses should be applied here. }" (example/main.cpp:313-317).  On a device-resident world that loop cannot be the caller's without a download and
   an upload of the momentum per iteration, so the library offers it: a door on a hinge, a rope bridge, a crate on a chain, a ragdoll, a trailer on a hitch.
   All four calls are opt-in; they slot between the calls of the call-by-call ABI and no other call changes a byte:
       nh_joints_prepare, nh_joint_connections                         -- when the list changes (the topology is the caller's and static)
       nh_collide (the connections among its body_connections), nh_apply_gravity_damping, nh_read_cached_impulses, nh_setup_contact_constraints,
       nh_joints_setup, iterations x { nh_apply_impulses(1), nh_joints_apply(1) }, nh_update_cached_impulses, nh_write_cached_impulses, nh_advance
   Under NH_FLAG_SINGLE_APPLY or NH_FLAG_FUSED_STEP there is one contact apply per step: joints can only FOLLOW it (nh_apply_impulses(iterations), then
   nh_joints_apply(iterations)) -- and under NH_FLAG_FUSED_STEP the bodies that solver owns have then been advanced already.  Use neither flag for jointed worlds.
   RECORDS (device memory, 16-byte aligned).  nh_Joint: two bodies, a type, flags (0), one body-local anchor per body, six parameters p -- DISTANCE: p[0] =
   min_length, p[1] = max_length, the rest 0; HINGE: p[0..2] = axis_a, p[3..5] = axis_b, body-local unit vectors that the library does not normalise; BALL: all
   0.  For body 0, the static world, transforms[0] is read like any other transform; its velocity counts as zero and its momentum is never read or written.
   nh_JointImpulse: the accumulated impulse per row, caller-owned and persistent like the contact cache; the caller zeroes it once.
   A joint is VALID iff its type is known, flags == 0, a != b, a and b < bodies->count and, for DISTANCE, 0 <= min <= max (comparisons: a NaN is invalid).  An
   invalid joint does nothing anywhere and has level 0.
   THE SCHEDULE: THE CALLER'S LIST ORDER, REPLAYED IN PARALLEL.  nh_joints_setup and every sweep of nh_joints_apply give the bytes of the serial loop "for each
   joint in list order, for each row in row order".  That order is the specification and what the host oracle runs (tests/hostoracle/hostjoint.cpp).  The device gets
   there through dependency LEVELS: level(j) = 1 + max(level of the last earlier valid joint of the same BIN that names j's dynamic body a, the same for b); a
   joint without such a predecessor has level 1, body 0 creates no dependency.  Joints of one level share no dynamic body, so any execution that finishes level L
   before level L + 1 is the serial loop.  The caller controls the depth: a rope listed link by link has as many levels as links; listed even links first, odd
   links second, it has two.
   nh_JointList.offsets (assemblies + 1 device words, or NULL: the list is one assembly) are permitted CUT POINTS: the caller promises that no dynamic body is named
   on both sides of one.  BIN w holds the assemblies i with offsets[i] / NH_JOINT_BIN == w; their joints are one contiguous span.  An assembly holds at most
   NH_JOINT_ASSEMBLY_MAX joints, a span therefore at most 1279.  One workgroup owns one bin (it finds its span by two binary searches in `offsets`); levels restart at 1
   per bin.  A body shared by two assemblies of the SAME bin is scheduled correctly by the level rule and is no error.
   nh_joints_prepare(ctx, bodies_count, list, plan) -- when the list changes, not per step.  Writes levels[j]; order[]: every span's joint indices sorted by
   (level, index), level-0 joints first; status[0]: NH_JOINT_ERR_OFFSETS (offsets[0] != 0, offsets[assemblies] != count or offsets[i + 1] < offsets[i]),
   NH_JOINT_ERR_ASSEMBLY_SIZE (an ascending pair more than NH_JOINT_ASSEMBLY_MAX apart; a list without offsets: count above it), NH_JOINT_ERR_SHARED_BODY (a dynamic
   body named by valid joints of two different bins; not looked for under NH_JOINT_ERR_OFFSETS); status[1]: valid joints; status[2]: the highest level; status[3]:
   bins with at least one joint.  With status[0] != 0: levels[j] = 0, order[j] = j, status[2] = status[3] = 0.  The owner check is one word per body, cleared per
   call: a min over bin numbers sets it, a second pass compares -- the bits are a function of the input alone.  count == 0 writes four zero status words.
   nh_joints_setup and nh_joints_apply read status[0] ON THE DEVICE and do nothing when it is non-zero.
   THE ARITHMETIC (nudge_amd/csrc/nh_joint.h states it once; fp32, only + - * /, sqrtf and compares, no contraction: the library is built with
   -ffp-contract=off; dot products and 3x3 products associate left to right, (x + y) + z; rotate, cross, dot, the world inverse inertia W and the tangent pair are
   the solver's own).  Per joint: r_x = rotate(q_x, anchor_x); d = (p_b + r_b) - (p_a + r_a); mi_x = mass_inverse, W_x = W(q_x, inertia_inverse) -- body 0: mi = 0,
   W = 0.  A ROW has a linear direction n (or none), ja and jb (linear: ja = -(r_a x n), jb = r_b x n; angular: ja = -t, jb = t), k = [(mi_a + mi_b), linear rows
   only] + ja . (W_a ja) + jb . (W_b jb), m = k > 0 ? 1 / k : 0, bias = clamp(beta * C, -max_bias, max_bias) with beta = time_step > 0 ? baumgarte / time_step : 0,
   and bounds [lo, hi].
     BALL      three rows: n = e_x, e_y, e_z; C = d.x, d.y, d.z; unbounded.
     DISTANCE  one row: len = sqrtf(d . d), n = len > 0 ? d / len : (0, 1, 0).  min == max: C = len - min, unbounded (a rod); len > max: C = len - max, [-inf, 0];
               len < min: C = len - min, [0, +inf]; otherwise the row is DEAD: m = 0, bias = 0, and its accumulated impulse is forced to +0.
     HINGE     BALL's three rows, then two angular ones: a1 = rotate(q_a, axis_a), a2 = rotate(q_b, axis_b), (t1, t2) = the solver's tangents of a1,
               C_k = (a1 x a2) . t_k, unbounded.
   ONE VISIT of a row: jv = n . (v_b - v_a) + ja . w_a + jb . w_b; lambda = -(jv + bias) * m; acc' = clamp(acc + lambda, lo, hi); delta = acc' - acc;
   v_a -= n * (delta * mi_a); w_a += (W_a ja) * delta; v_b += n * (delta * mi_b); w_b += (W_b jb) * delta.  unused0 and unused1 of nh_BodyMomentum keep their bits
   (the reference's setup stashes mass_inverse in unused0, nudge.cpp:4182-4199).
   nh_joints_setup(ctx, active_bodies, bodies, list, plan, params, impulses) -- after nh_setup_contact_constraints.  It completes pending work and is an entry
   point of the step in note 9's sense.  A joint is LIVE this step iff it is valid and one of its dynamic bodies is on this step's active list (the list and its
   device-side count as nh_apply_gravity_damping reads them; one flag byte per body in context scratch).  Per live joint, in schedule order: the rows are built
   into the context's solve records, acc_k = warm * impulses[j].row[k] (a dead row: +0), and every acc_k is applied as a delta.  A joint that is not live writes
   nothing, and its nh_JointImpulse keeps its bytes.
   nh_joints_apply(ctx, bodies, list, plan, impulses, iterations) -- `iterations` sweeps in ONE launch: the bin's workgroup walks the levels with a workgroup
   barrier between them, lanes take the joints of a level and move the two bodies' 32-byte momentum records with 16-byte accesses; after the last sweep the
   lane stores impulses[j] whole (rows the type does not have: +0; reserved: 0).  It completes pending work first.  NH_ERR_STALE_SETUP without an nh_joints_setup
   of a list of this count since the last nh_collide or nh_joints_prepare.
   nh_joint_connections(ctx, list, out) -- (a, b) per valid joint, (0, 0) per invalid one (valid by the bodies_count of the last nh_joints_prepare, which must
   have been called: NH_ERR_INVALID otherwise); nh_collide skips connections with a zero.  Passed as nh_BodyConnections, an assembly sleeps and wakes as one set.
   All calls return NH_ERR_INVALID, before any launch and writing nothing: for a NULL ctx, list, plan, bodies, active_bodies, params, impulses, out or plan array;
   for joints NULL with count > 0; for joints / impulses not 16-byte, out not 8-byte, offsets / status / levels / order not 4-byte aligned; for count or assemblies
   >= 2^31; for plan->capacity < count; for NULL body arrays with bodies->count > 0; for a time_step, baumgarte, max_bias or warm that is not finite or is
   negative, or warm > 1; for iterations == 0.  count == 0: setup and apply complete pending work and do nothing else.
   SCRATCH is the context's: 432 B of solve record per joint of the largest count seen, and per body of the largest bodies->count one owner word and one flag byte.
   It grows behind a stream synchronise; nh_destroy frees it.  Everything else is enqueued on the context's stream; nothing waits for a count.
   Timing labels: j_owner (clear, offsets check, owner min, owner compare), j_levels, j_setup (flag bytes and setup), j_sweep, j_connections.
   MEASURED: NOT MEASURED YET (tools/joints.py -> profiles/joint_rates.log has not been run at size on a GPU; no bar is set in advance).
   Not built: weld joints; hinge limits and motors; springs; block (3x3) solves; assemblies over 1024 joints; joints inside nh_step and still steps; partitioned
   worlds; the `namespace nudge` extension. */
enum { NH_JOINT_BALL = 1u, NH_JOINT_DISTANCE = 2u, NH_JOINT_HINGE = 3u };
#define NH_JOINT_BIN 256u
#define NH_JOINT_ASSEMBLY_MAX 1024u
enum { NH_JOINT_ERR_ASSEMBLY_SIZE = 1u, NH_JOINT_ERR_SHARED_BODY = 2u, NH_JOINT_ERR_OFFSETS = 4u };          /* bits of plan->status[0] */
typedef struct nh_Joint { uint32_t a, b, type, flags /* 0 */; float anchor_a[3], anchor_b[3]; float p[6]; } nh_Joint;          /* 64 B */
typedef struct nh_JointImpulse { float row[6]; uint32_t reserved[2]; } nh_JointImpulse;                                       /* 32 B */
typedef struct nh_JointParams { float time_step, baumgarte, max_bias, warm; } nh_JointParams;                                 /* 16 B */
typedef struct nh_JointList {        /* host struct, DEVICE pointers; host counts */
	const nh_Joint* joints;
	const uint32_t* offsets;         /* assemblies + 1 device words, or NULL */
	uint32_t count, assemblies;
} nh_JointList;
typedef struct nh_JointPlan {        /* host struct, DEVICE pointers */
	uint32_t* status;                /* 4 words */
	uint32_t* levels;                /* capacity words */
	uint32_t* order;                 /* capacity words */
	uint32_t capacity, reserved;
} nh_JointPlan;
int nh_joints_prepare(nh_context* ctx, uint32_t bodies_count, const nh_JointList* list, const nh_JointPlan* plan);
int nh_joints_setup(nh_context* ctx, const nh_ActiveBodies* active_bodies, const nh_BodyData* bodies, const nh_JointList* list, const nh_JointPlan* plan,
                    const nh_JointParams* params, const nh_JointImpulse* impulses);
int nh_joints_apply(nh_context* ctx, const nh_BodyData* bodies, const nh_JointList* list, const nh_JointPlan* plan, nh_JointImpulse* impulses, uint32_t iterations);
int nh_joint_connections(nh_context* ctx, const nh_JointList* list, nh_BodyPair* out);

/* nh_distance: how far each of `count` query shapes is from the world of the LAST nh_query_build or nh_query_refit, and towards what -- the clearance
   of a crate, a hull or a limb.  nh_penetration describes a pair that overlaps; this describes the pairs that do not.
   Query shapes: nh_overlap's (NH_SHAPE_SPHERE, NH_SHAPE_BOX, NH_SHAPE_CAPSULE), the same fields read and the same validity rules; the first 48 bytes
   of nh_DistanceQuery are an nh_OverlapQuery.  `reserved` is not read.
   Output: one nh_PointHit per query, nh_closest's record --
     - `distance`: the key of the collider, below;
     - `normal`: a unit vector from the collider towards the query shape;
     - `point`: the witness on the collider's surface; the witness on the query shape is point + distance * normal;
     - body, collider, shape, tag as in nh_closest; `reserved` = 0.
   THE ANSWER is the smallest key with key <= max_distance over every collider of the last build or refit (those of sleeping bodies and of body 0
   included), less those of `ignore_body` (0xffffffff: none is ignored); ties go to the lower combined collider index (boxes 0 .. nbox-1, then the
   spheres).  A collider of a NaN pose is never reported.  A miss is nh_closest's miss record (shape = NH_SHAPE_NONE, normal = point = 0,
   body = collider = tag = 0xffffffff) with distance = max_distance; an INVALID query -- one that nh_overlap counts 0, or whose max_distance is NaN or
   negative -- writes the miss record with distance = NaN.  max_distance = +inf finds the nearest collider anywhere; max_distance = 0 only overlaps.
   Per pair (exact arithmetic: nudge_amd/csrc/nh_query.h, "distance": fixed enumerations, no iterative GJK, so a brute force gives the same bytes):
     - sphere query (c, r) / sphere or box: nh_closest's signed distance d of c, separation = d - r, its normal and its point;
     - box query / sphere (p, R): d of p from the QUERY box, separation = d - R, that normal negated, point = p + R normal;
     - capsule / sphere (p, R): m from p to the segment's closest point, separation = (|m| - R) - r, normal = m / |m|, point = p + R normal;
     - capsule / box: the least of nh_penetration's SHALLOW candidates (the end points against the box, the -a end first, then the twelve box edges against
       the segment; the first on equality) at distance d, separation = d - r, normal along the closest points, point = the box's;
     - box query / box: the least distance over, in this order and the first on equality, the 8 vertices of the query box against the collider (vertex v
       has the sign + on axis k where bit k of v is set), the 8 vertices of the collider against the query box, and the 144 edge pairs (the query box's
       edges by axis x, y, z and corner (-, -), (+, -), (-, +), (+, +), each against the collider's twelve in the same order).  A box with a zero half
       extent is valid.
   THE OVERLAP RECORD: distance 0, normal = point = 0, the identity fields filled.  It is written where nh_overlap's predicate of the pair accepts, where
   the computed separation is <= 0, and where there is no direction (the closest points coincide) -- the casts' START OVERLAP stance: how deep and which
   way out is nh_penetration's answer.  INVARIANT: the normal is a unit vector iff the record is a separated one.
   THE KEY, under the reach rule of DESIGN 10.5: key = max(separation clamped at +0, sqrtf(g2)), g2 the squared per-axis gap between the query's world
   AABB (centre -+ r; the box's |R| size; the capsule's |a_k| + r; not padded) and the collider's own box in the hierarchy (k_q_boxes_runs' padded box).
   The written `distance` is the key.  It moves a distance only where rounding put the pair function in front of a box padded by 2^-18 of its
   coordinates.  THE CORNER: the key holds for an overlap record too -- should rounding ever put apart (g2 > 0) the boxes of a pair that is accepted as
   overlapping, the record carries the distance sqrtf(g2) > 0 with its zero normal, and it competes (and is cut by max_distance) with that key, exactly
   as the walk sees it.  Test the normal, not the distance, to tell the two kinds of record apart.  For box / box and both capsule pairs the corner
   cannot occur: their overlap predicates require the unpadded AABBs to touch.
   IDENTITIES (contracts):
     - a capsule of half height 0 writes the sphere query's bytes, and its rotation is not read;
     - a sphere of radius 0 writes nh_closest's bytes for the same point, max_distance and ignore_body, wherever nh_closest reports distance > 0;
     - after nh_query_refit the bytes are those after an nh_query_build of the same transforms.
   Accuracy (measured): against float64 evaluations the distance lies within 2.3e-7, and both witnesses within 3.7e-7, of the pair's sizes
   plus centre distance.
   Returns NH_ERR_INVALID before any nh_query_build, for flags != 0, for null or not 16-byte aligned `queries` / `hits`, and for count >= 2^30;
   count = 0 is a no-op that returns NH_OK and launches nothing.  An OBSERVER like nh_closest (note 9): no view export, no settling of deferred gravity,
   no still step turned into a full one, no change to nh_Counts; it never allocates and never waits, it only launches on the context's stream.
   Cost: one lane per query on the walk of nh_closest; the box / box pair function is ~150 segment tests where nh_closest's is one clamp.
   Measured (MI355X, the landed config-2 world of 1,004,524 colliders, 1 M queries of up to half a body's size, tools/distance_rates.py ->
   profiles/distance_rates.log): unbounded, 1.6-1.8 ms as spheres, 4.2-4.4 ms as capsules, 33-36 ms as boxes beside nh_closest's 1.1-1.3 ms on
   the centres; with max_distance 2 near the bodies 0.77 / 1.02 / 4.92 ms beside 0.81 ms. */
typedef struct nh_DistanceQuery { float center[3]; uint32_t shape; float rotation[4]; float size[3]; uint32_t ignore_body;   /* = nh_OverlapQuery, 48 B */
                                  float max_distance; uint32_t reserved[3]; } nh_DistanceQuery;                              /* 64 B */
int nh_distance(nh_context* ctx, const nh_DistanceQuery* queries, uint32_t count, nh_PointHit* hits, uint32_t flags /* 0 */);

/* nh_move: collide-and-slide for `count` swept capsules against the world of the LAST nh_query_build or nh_query_refit -- the loop a character controller
   runs around nh_capsulecast (cast, advance to the contact, deflect what is left of the displacement along the surface, cast again), on the device, in ONE
   launch, so that no slide costs a launch, a wait and an upload.  nh_Move is nh_CapsuleCast field for field with `skin` where max_t is and `max_slides`
   where reserved[0] is; the capsule (rotation, radius, half_height) is nh_capsulecast's, and half_height = 0 is a ball.  `reserved` is not read.
   ONE MOVE, all in float32; the arithmetic is nudge_amd/csrc/nh_query.h, "move" (nh_q_move_begin / nh_q_move_go / nh_q_move_advance), which is the
   definition and fixes the order of every operation (each product rounded before its sum, no fused multiply-add; dot products (x*x + y*y) + z*z).
   State: p = origin, v = displacement, d0 = displacement, no n_prev, slides = 0, flags = 0, last = the miss record of a capsule cast with max_t = 1.  Repeat:
     1. v.v == 0: stop.
     2. last = the closest-hit answer nh_capsulecast with flags 0 writes for { p, 1.0f, v, ignore_body, rotation, radius, half_height }: the same decode,
        reach rule and tie rule, under the context's layer filter (the per-query mask index is the move's index).
     3. a miss: p = p + v (one add per component), v = 0, stop.
     4. a hit with t == 0 (START OVERLAP, or touching): flags |= NH_MOVE_START_OVERLAP, stop; p and v keep their bits.  The normal of such a hit is
        -v / |v| and says nothing about the surface: getting out is nh_recover's business (below).
     5. a hit with t > 0: flags |= NH_MOVE_HIT, slides += 1, p = p + t*v, then p = p + skin*n (a multiply and an add per component each), rem = (1 - t)*v.
     6. deflect: s = rem.n; v' = rem - s*n if s < 0, else rem.  Where a hit was taken before and v'.n_prev < 0 (a CREASE): c = n_prev x n; c.c < 2^-24:
        v' = 0; else v' = c * ((rem.c) / (c.c)); then v' = 0 if v'.n_prev < 0 or v'.n < 0.  Then v' = 0 unless v'.d0 > 0 (a move never turns against what
        was asked for), and v' = 0 unless v'.v' > 2^-40 * (d0.d0).  If one of these rules wrote v' = 0 and rem was not 0: flags |= NH_MOVE_WEDGED -- a
        head-on hit sets it, through the d0 rule.  v = v', n_prev = n.
        (The crease's last test compares rounded products of c with the normals it was built from: off the coordinate axes it fires on rounding dust in
        about six creases in ten, which then end WEDGED where an exact evaluation would slide along c.  DESIGN 10.15.)
     7. slides > max_slides and v.v > 0: flags |= NH_MOVE_SLIDES_OUT, stop.  So a move makes at most max_slides + 1 casts; max_slides = 0 is one cast.
   Output: position = p, remaining = v, slides, flags, last_hit = last.  flags == 0 with remaining == 0: the move went through freely.
   SKIN is the gap the capsule keeps: after a hit it is pushed skin along the NORMAL (not back along the path, which at a grazing angle would take
   skin / sin of the angle away from the travel, or leave less than skin of clearance), so the next cast starts free.  skin = 0 is valid and leaves the capsule touching: the
   next cast is then a START OVERLAP, so it is of use with max_slides = 0 only.  Scale skin to the scene: it must exceed the rounding of p (2^-23 of its
   largest coordinate) by a margin for the slide to start free; 0.01 for bodies of size 1 near the origin.
   INVALID RECORDS -- a non-finite origin or displacement; a non-finite or negative radius, half height or skin; half_height > 0 with a non-finite
   rotation; max_slides > NH_MOVE_MAX_SLIDES -- write flags = NH_MOVE_INVALID, position = the bits of origin, remaining = the bits of displacement,
   slides = 0 and last_hit = the miss record with t = NaN.  displacement = 0 is a valid no-op that makes no cast.  (Finite inputs whose sums overflow make a
   cast with a non-finite origin: it is a miss with t = NaN, as in nh_capsulecast, and the move ends there.)
   IDENTITIES (contracts):
     - with max_slides = 0, last_hit holds byte for byte what nh_capsulecast with flags 0 writes for { origin, 1.0f, displacement, ignore_body, rotation,
       radius, half_height };
     - half_height = 0 does not read `rotation`: its casts are nh_spherecast's;
     - REPLAY: running the loop on the host, one nh_capsulecast call per round and nh_q_move_advance between them, gives nh_move's 64 bytes per record;
     - after nh_query_refit the bytes are those after an nh_query_build of the same arrays; nh_query_filter is honoured in all three modes.
   Returns NH_ERR_INVALID before any nh_query_build, for flags != 0, for count >= 2^30, and for count > 0 with `moves` or `results` null or not 16-byte
   aligned; count = 0 is a no-op that returns NH_OK and launches nothing.  Every byte of `count` results is written and nothing behind them.  Never
   allocates, never waits: ONE launch on the context's stream (timing label q_move).  An OBSERVER like nh_capsulecast (note 9): no view export, no
   settling of deferred gravity, no still step turned into a full one, no change to nh_Counts.
   NOT BUILT: rotation during the move (boxes move by nh_boxmove, below); gravity (step-up, ground snapping and slope limits are nh_walk, below; depenetration of a move that
   starts in overlap is nh_recover, below: recover, then move or walk); moving platforms (the velocity of what is hit); pushing dynamic bodies (queries are observers; what
   the move touched is listed by nh_move_touched, below).
   Cost: one lane per move, up to max_slides + 1 walks of nh_capsulecast's; a lane that has finished waits for the slowest of its wave.  Measured (one
   MI355X, the landed config-2 world of 1,004,524 colliders, 1,048,576 moves of r = hh = 0.5 from just above resting bodies by 0.75 - 3 units, max_slides 4;
   tools/move_rates.py -> profiles/move_rates.log): 1.90 ms beside 1.14 ms for nh_capsulecast on the first casts alone; the moves made 1.61 casts
   on average, so the call takes 1.03 of (casts per move x the capsule cast's time) on that workload. */
#define NH_MOVE_MAX_SLIDES 8u
enum { NH_MOVE_HIT = 1u, NH_MOVE_START_OVERLAP = 2u, NH_MOVE_SLIDES_OUT = 4u, NH_MOVE_WEDGED = 8u, NH_MOVE_INVALID = 0x80000000u };
typedef struct nh_Move { float origin[3]; float skin; float displacement[3]; uint32_t ignore_body;
                         float rotation[4]; float radius; float half_height; uint32_t max_slides; uint32_t reserved; } nh_Move;      /* 64 B */
typedef struct nh_MoveResult { float position[3]; uint32_t flags; float remaining[3]; uint32_t slides; nh_RayHit last_hit; } nh_MoveResult;   /* 64 B */
int nh_move(nh_context* ctx, const nh_Move* moves, uint32_t count, nh_MoveResult* results, uint32_t flags /* 0 */);

/* nh_recover: push each of `count` query shapes (spheres, boxes, capsules: nh_OverlapQuery's encoding) out of everything it overlaps in the world of the
   LAST nh_query_build or nh_query_refit -- what follows a start overlap: a capsule that ends a step sunk into a body that moved onto it, a crate spawned
   into a pile, a character teleported to a checkpoint.  The loop a host would run around nh_penetration (list, download, pick a push, upload, again) runs on
   the device, one lane per query, in ONE call.  nh_Recover is nh_OverlapQuery (its first 48 bytes, field for field) followed by `skin` and
   `max_iterations`; `reserved` is not read.
   ONE RECOVER, all in float32; the arithmetic is nudge_amd/csrc/nh_query.h, "recover" (nh_q_recover_begin / nh_q_recover_better / nh_q_recover_advance),
   which is the definition and fixes the order of every operation (each product rounded before its sum, no fused multiply-add).
   State: p = center, iterations = 0, flags = 0, last = the NONE record (normal = 0, depth = 0, body = collider = tag = 0xffffffff, shape = NH_SHAPE_NONE).
   Repeat:
     1. S = the colliders nh_overlap lists for the shape at p: the same decode, the same predicates, ignore_body excluded, under the context's layer
        filter (the per-query mask index is the query's index).  NaN poses are never in S.  S empty: stop.
     2. Among S the collider of greatest depth under the pair function nh_penetration uses for that pair; ties go to the lowest combined collider index
        (boxes before spheres).  last = that pair's nh_PenetrationHit: the bytes nh_penetration writes for it with the query at p.
     3. s = depth + skin.  s == 0: flags |= NH_RECOVER_TOUCHING, stop.
     4. iterations == max_iterations: flags |= NH_RECOVER_OVERLAPPING, stop.
     5. p = p + s * normal (one multiply and one add per component), iterations += 1, flags |= NH_RECOVER_PUSHED.
   Output: position = p, push = p - center (one subtract per component), iterations, flags, last.  So a recover makes at most max_iterations pushes and
   max_iterations + 1 walks; max_iterations = 0 only looks.  A result with none of OVERLAPPING, TOUCHING and INVALID set is FREE: the last walk ran
   nh_overlap's very predicates at that very p and found nothing, so nh_overlap of the same shape at `position` counts 0 -- exactly.
   DEEPEST FIRST, not a sum of pushes: a maximum with an index tie-break does not depend on the order a walk meets the leaves, so the answer is defined
   without the tree and a brute force over all colliders gives the same 64 bytes; a float sum over S would depend on the walk order.
   SKIN is the gap kept: for a convex pair, depth along the minimum-translation normal leaves the pair touching, and another skin along the same normal
   leaves at least skin between them, so the next round no longer sees that collider and a following nh_move starts free.  skin = 0 is valid and leaves the
   shape touching: the next walk then finds the pair again at a depth of 0 (TOUCHING) or of rounding dust, which may spend the iterations on pushes of an
   ulp.  Scale skin to the scene: it must exceed the rounding of p (2^-23 of its largest coordinate) by a margin; 0.01 for bodies of size 1 near the origin.
   OVERFLOW: a p that overflows makes the next round's query invalid; an invalid query overlaps nothing, so the recover ends there, as nh_move's does.
   INVALID RECORDS -- anything nh_overlap counts as an invalid query (an unknown shape, a non-finite centre, a non-finite or negative size the shape reads,
   a non-finite rotation where it is read), a non-finite or negative skin, max_iterations > NH_RECOVER_MAX_ITERATIONS -- write flags =
   NH_RECOVER_INVALID, position = the bits of center, push = 0, iterations = 0 and last = the NONE record.
   IDENTITIES (contracts):
     - a query for which nh_overlap counts 0 returns flags = 0, position = the bits of center and last = the NONE record;
     - with max_iterations = 0, last is the record of greatest depth (ties to the lowest collider index) in the segment nh_penetration writes for the same
       first 48 bytes, position keeps the bits of center, and flags is NH_RECOVER_OVERLAPPING, NH_RECOVER_TOUCHING or 0;
     - REPLAY: one nh_penetration call per round and nh_q_recover_advance on the host between them give nh_recover's 64 bytes per record;
     - a capsule of half height 0 writes the sphere query's bytes and does not read `rotation`;
     - after nh_query_refit the bytes are those after an nh_query_build of the same arrays; nh_query_filter is honoured in all three modes (the
       twenty-second call of the MASKED WORLD contract).
   Returns NH_ERR_INVALID before any nh_query_build, for flags != 0, for count >= 2^30, and for count > 0 with `queries` or `results` null or not 16-byte
   aligned; count = 0 is a no-op that returns NH_OK and launches nothing.  Every byte of `count` results is written and nothing behind them.  Never
   allocates, never waits: two launches on the context's stream (spheres and boxes; capsules of nonzero half height, as nh_overlap splits them), one timing
   label, q_recover.  An OBSERVER like nh_overlap (note 9): no view export, no settling of deferred gravity, no still step turned into a full one, no
   change to nh_Counts.
   NOT BUILT: rotation out of overlap (the shape keeps its orientation); a push shared among several colliders at once (each round answers the deepest
   one only, so a shape between two colliders it cannot clear -- a ball in a slot narrower than itself, a concave wedge -- is pushed back and forth and
   ends OVERLAPPING: raise max_iterations, move it by other means, or accept the overlap); velocities (recover moves a position, nothing else).
   Cost: one lane per query, up to max_iterations + 1 walks of nh_overlap's with the pair function at each accepted leaf; a lane that has finished waits
   for the slowest of its wave.  Measured (one MI355X, the landed config-2 world of 1,004,524 colliders, 1,048,576 shapes of size 0.5 sunk into the tops of
   resting bodies, skin 0.01, max_iterations 4; tools/recover_rates.py -> profiles/recover_rates.log): 1.35 ms for spheres, 1.83 ms for
   capsules, 1.97 ms for boxes, 1.96 - 2.08 walks per query on average -- 0.70, 0.91 and 0.96 of ONE nh_penetration count call + list call on the same
   first 48 bytes (of which the host loop makes one per round, with a download and an upload), and 1.08, 1.37 and 1.43 of (walks per query x the
   nh_overlap count walk).  Filter off, beside the parent commit's library in the same process: nh_overlap 0.995, nh_move 1.001 of its times. */
#define NH_RECOVER_MAX_ITERATIONS 8u
enum { NH_RECOVER_PUSHED = 1u, NH_RECOVER_OVERLAPPING = 2u, NH_RECOVER_TOUCHING = 4u, NH_RECOVER_INVALID = 0x80000000u };
typedef struct nh_Recover { float center[3]; uint32_t shape; float rotation[4]; float size[3]; uint32_t ignore_body;   /* = nh_OverlapQuery, 48 B */
                            float skin; uint32_t max_iterations; uint32_t reserved[2]; } nh_Recover;                      /* 64 B */
typedef struct nh_RecoverResult { float position[3]; uint32_t flags; float push[3]; uint32_t iterations; nh_PenetrationHit last; } nh_RecoverResult; /* 64 B */
int nh_recover(nh_context* ctx, const nh_Recover* queries, uint32_t count, nh_RecoverResult* results, uint32_t flags /* 0 */);

/* nh_walk: a GROUNDED character step for `count` capsules against the world of the LAST nh_query_build or nh_query_refit -- nh_move with the rules a
   character controller puts around it: steps are climbed (step-up), faces too steep to stand on act as walls (slope limit), the capsule follows the
   ground down a ledge or over a crest (snap), and the result says what it stands on.  The frame of a controller is nh_query_refit, nh_recover, nh_walk:
   ONE launch each, no download between them.  The first 64 bytes of nh_Walk are nh_Move field for field; `up` is the unit vector against gravity,
   `step_height` the highest riser climbed, `snap_distance` how far below the capsule ground is looked for, `min_ground_up` the cosine of the slope limit:
   the least n.up of a hit normal that still counts as ground (0: no limit).  options: NH_WALK_PROBE_ONLY = look for ground but do not move onto it.
   `reserved` and `reserved2` are not read.
   ONE WALK, all in float32; the arithmetic is nudge_amd/csrc/nh_query.h, "walk" (nh_q_walk_begin / nh_q_walk_cast / nh_q_walk_advance), which is the
   definition and fixes the order of every operation.  "The move loop from p along v with k slides" is nh_move's rules 1 - 7 with max_slides = k, each cast
   the closest-hit capsule cast { p, 1.0f, v, ignore_body, rotation, radius, half_height }.  A hit normal n is WALKABLE when u = n.up has u > 0 and
   u >= min_ground_up; otherwise it is STEEP.
     A. SLIDE: the move loop from origin along displacement with max_slides, under the climb rule: pA, vA, flags, slides, last_hit.  A start overlap ends
        the walk here: the outputs are nh_move's, ground is the miss record.  Any taken hit (t > 0) that is steep sets `blocked`.
        CLIMB RULE (steep faces act as walls), off when min_ground_up == 0: at a taken hit that is steep with u >= 0 and whose plain deflection
        w = rem - (rem.n) n (move's first deflect line) has w.up > 0, flags |= NH_WALK_STEEP and the deflection, the crease and n_prev use
        ns = (n - u up) / |n - u up| in place of n (n itself where |n - u up|^2 < 2^-24); the skin push stays along n.
     B. STEP UP, only when step_height > 0 and blocked:
        U. the move loop from origin along step_height * up with 0 slides: pU; lift = (pU - origin).up.  Abandoned on a start overlap or !(lift > 0).
        F. the move loop from pU along displacement with max_slides, under the climb rule: pF, vF, flags, slides, last_hit.  Abandoned on a start overlap.
        D. the move loop from pF along -lift * up with 0 slides: pD and its cast's record gD.
        ACCEPTED iff D took a hit with t > 0 whose normal is walkable and (pD - origin).dh > (pA - origin).dh, dh = displacement - (displacement.up) up.
        Then position = pD; remaining, slides, last_hit and the move flags (NH_WALK_STEEP with them) are F's; flags |= STEPPED | GROUNDED; ground = gD;
        step_up = (pD - pA).up; no probe.  Otherwise A stands.
     C. GROUND PROBE, when snap_distance > 0, there was no start overlap and no step was taken: the capsule cast { p, 1, -snap_distance * up }.  ground =
        its record.  A miss: airborne.  A steep hit: NH_WALK_ON_STEEP, no motion.  A walkable hit: NH_WALK_GROUNDED, and unless PROBE_ONLY or t == 0:
        p = p + t*v, p = p + skin*n (move's rule 5), drop = t * snap_distance, NH_WALK_SNAPPED.
   Output: position, flags (NH_MOVE_* of the slide that was kept in bits 0 - 3, NH_WALK_* above), remaining, slides (the hits taken in the kept slide),
   last_hit (its last cast), ground, step_up, drop, casts (every cast made: at most NH_WALK_MAX_CASTS), reserved = 0.  Where no probe and no step wrote it,
   ground is the miss record with t = 1.
   INVALID RECORDS -- whatever nh_move rejects in the first 64 bytes; a non-finite up; |up.up - 1| > 2^-10; a non-finite or negative step_height or
   snap_distance; min_ground_up non-finite or outside [0, 1]; an unknown options bit -- write flags = NH_WALK_INVALID, position = the bits of origin,
   remaining = the bits of displacement, slides = casts = 0, step_up = drop = 0 and both hit records as the miss record with t = NaN.
   IDENTITIES (contracts):
     1. with step_height = 0, snap_distance = 0 and min_ground_up = 0 the first 64 bytes of the result are nh_move's 64 bytes for the record's first 64
        bytes, and ground is the miss record;
     2. REPLAY, with min_ground_up = 0: the phases run from the host -- nh_move calls for A, U, F and D, an nh_capsulecast call for C, nh_q_walk_phase_end
        and nh_q_walk_advance between them -- give nh_walk's 112 bytes.  (`blocked` needs every taken hit of A, which nh_move's result does not hold: the
        replay reads them off nh_move's own REPLAY, one nh_capsulecast per round.)
     3. half_height = 0 does not read `rotation`;
     4. after nh_query_refit the bytes are those after an nh_query_build of the same arrays; nh_query_filter is honoured in all three modes (the per-query
        mask index is the walk's index);
     5. a result without INVALID and START_OVERLAP never has casts > NH_WALK_MAX_CASTS; a GROUNDED result's ground.normal is walkable.
   Returns NH_ERR_INVALID before any nh_query_build, for flags != 0, for count >= 2^30, and for count > 0 with `walks` or `results` null or not 16-byte
   aligned; count = 0 is a no-op that returns NH_OK and launches nothing.  Every byte of `count` results is written and nothing behind them.  Never
   allocates, never waits: ONE launch on the context's stream (timing label q_walk).  An OBSERVER like nh_move (note 9).
   NOT BUILT: rotation during the walk (boxes walk by nh_boxwalk, below); moving platforms (the velocity of what is stood on); pushing dynamic bodies (queries are observers;
   last_hit and ground are single records: what the walk touched is listed by nh_walk_touched, below); gravity integration and velocities (the caller passes a displacement); a
   per-node AND word for the filter; queries on partitioned worlds; the `namespace nudge` extension in nudge_amd/compat; any change to nh_move's crease rule.
   Cost: one lane per walk, up to 21 walks of nh_capsulecast's; the lanes of a wave walk the tree together whatever phase each is in, and a lane that has
   finished waits for the slowest of its wave.  168 VGPRs at 3 waves per SIMD, no scratch (4 waves would spill 132 - 144 bytes per lane).  Measured (one
   MI355X, the landed config-2 world of 1,004,524 colliders, 1,048,576 walks of r = 0.3, hh = 0.4, max_slides 4, snap 0.3, half on the slab walking towards a
   resting body, half on a body's top; tools/walk_rates.py -> profiles/walk_rates.log): 2.85 ms with step_height 0 (2.31 casts per walk), slope
   limit off or 45 degrees; 4.73 ms with step_height 1.0 and the limit off (2.98 casts), 5.50 ms with the limit at 45 degrees (3.79 casts), beside 0.956 ms
   for nh_capsulecast on the first casts alone: 1.29, 1.29, 1.66 and 1.52 of (casts per walk x the capsule cast's time), where nh_move reported 1.03
   (8.0 % of these walks start in overlap and end after one cast: they are in the means).  The
   host loop of the REPLAY identity on the same batch, its uploads and downloads included: 824 ms for the same bytes.  Filter off, beside the parent commit's
   library in the same process: nh_move 0.996, nh_capsulecast 1.002 of its times.  NOT MEASURED YET: the filtered instantiation. */
#define NH_WALK_MAX_CASTS (2u * (NH_MOVE_MAX_SLIDES + 1u) + 3u)   /* 21 */
enum { NH_WALK_STEPPED = 0x10u, NH_WALK_GROUNDED = 0x20u, NH_WALK_SNAPPED = 0x40u, NH_WALK_STEEP = 0x80u, NH_WALK_ON_STEEP = 0x100u, NH_WALK_INVALID = 0x80000000u };
enum { NH_WALK_PROBE_ONLY = 1u };   /* nh_Walk.options */
typedef struct nh_Walk { float origin[3]; float skin; float displacement[3]; uint32_t ignore_body;
                         float rotation[4]; float radius; float half_height; uint32_t max_slides; uint32_t reserved;      /* = nh_Move, 64 B */
                         float up[3]; float step_height; float snap_distance; float min_ground_up; uint32_t options; uint32_t reserved2; } nh_Walk;   /* 96 B */
typedef struct nh_WalkResult { float position[3]; uint32_t flags; float remaining[3]; uint32_t slides; nh_RayHit last_hit; nh_RayHit ground;
                               float step_up; float drop; uint32_t casts; uint32_t reserved; } nh_WalkResult;                                     /* 112 B */
int nh_walk(nh_context* ctx, const nh_Walk* walks, uint32_t count, nh_WalkResult* results, uint32_t flags /* 0 */);

/* nh_boxmove, nh_boxwalk: nh_move and nh_walk for swept ORIENTED BOXES -- a kinematic crate, a lift, a door, a vehicle hull, an axis-aligned character of
   a voxel world (rotation = identity) -- against the world of the LAST nh_query_build or nh_query_refit, in ONE launch each.  nh_BoxMove is nh_BoxCast
   field for field with `skin` where max_t is and `max_slides` where reserved is; `size` holds the half extents and (0, 0, 0) is a ray.  nh_BoxWalk is
   nh_BoxMove followed by the last 32 bytes of nh_Walk (up, step_height, snap_distance, min_ground_up, options, reserved2); `reserved2` is not read.  The
   results are nh_MoveResult and nh_WalkResult unchanged, with the same flag bits, NH_MOVE_MAX_SLIDES and NH_WALK_MAX_CASTS.  The box does not turn.
   DEFINITION: nh_boxmove is nh_move's rules 1 - 7 word for word, and nh_boxwalk is nh_walk's phases A, U, F, D and C word for word, the climb rule
   included, where every cast is the closest-hit answer nh_boxcast with flags 0 writes for { p, 1.0f, v, ignore_body, rotation, size }: nh_boxcast's
   decode, reach rule, tie rule and start-overlap rule, under the context's layer filter (the per-query mask index is the record's index).  The arithmetic
   between two casts is the same functions of nudge_amd/csrc/nh_query.h ("move", "walk"), which never see the shape: a cast's (hit, t, normal, collider)
   is all they read.  One kernel template serves both shapes (k_q_move<Shape, .>, k_q_walk<Shape, .>).
   INVALID RECORDS -- nh_boxmove: a non-finite origin or displacement; a non-finite or negative size component or skin; a size other than (0, 0, 0) with a
   non-finite rotation; max_slides > NH_MOVE_MAX_SLIDES.  nh_boxwalk: those, and nh_walk's rules for up, step_height, snap_distance, min_ground_up and
   options.  They are written exactly as nh_move and nh_walk write theirs (flags = NH_MOVE_INVALID / NH_WALK_INVALID, position = the bits of origin,
   remaining = the bits of displacement, the hit records as the miss record with t = NaN, every count 0).  A size with one or two components 0 (a plate, a
   rod) is a box and reads its rotation.  displacement = 0 is a valid no-op that makes no cast.
   IDENTITIES (contracts):
     1. nh_boxmove with max_slides = 0: last_hit holds byte for byte what nh_boxcast with flags 0 writes for { origin, 1.0f, displacement, ignore_body,
        rotation, size };
     2. size (0, 0, 0) does not read `rotation`, and its 64 result bytes are those of nh_move with radius = half_height = 0 and the other fields equal:
        both are ray casts;
     3. REPLAY for nh_boxmove: running the loop on the host, one nh_boxcast call per round and nh_q_move_advance between them, gives nh_boxmove's 64 bytes;
     4. nh_boxwalk with step_height = snap_distance = min_ground_up = 0 writes nh_boxmove's 64 bytes for the record's first 64 bytes, and the miss
        record as ground;
     5. REPLAY for nh_boxwalk, with min_ground_up = 0: nh_boxmove calls for A, U, F and D, an nh_boxcast call for C, and nh_query.h's decisions
        (nh_q_walk_phase_end, nh_q_walk_advance) between them give nh_boxwalk's 112 bytes (`blocked` is read off nh_boxmove's own REPLAY of A);
     6. after nh_query_refit the bytes are those after an nh_query_build of the same arrays; nh_query_filter is honoured in all three modes;
     7. a result without INVALID and START_OVERLAP never has casts > NH_WALK_MAX_CASTS (21); a GROUNDED result's ground.normal is walkable.
   Both return NH_ERR_INVALID before any nh_query_build, for flags != 0, for count >= 2^30, and for count > 0 with the records or `results` null or not
   16-byte aligned; count = 0 is a no-op that returns NH_OK and launches nothing.  Every byte of `count` results is written and nothing behind them.
   Never allocate, never wait: ONE launch each on the context's stream (timing labels q_boxmove, q_boxwalk).  OBSERVERS like nh_move (note 9).
   WHAT A BOX STANDS ON: its bottom face.  A box that stands on a slope meets it with an edge; the ground normal is still the slope's (the sweep's
   separating axis), so WALKABLE and the climb rule mean what they mean for a capsule.  A step is climbed when the whole bottom face clears the riser.
   NOT BUILT: rotation during a move; moving platforms; pushing dynamic bodies; a change to the crease rule; the
   `namespace nudge` extension; queries on partitioned worlds; sphere movers as a call of their own (half_height = 0 in nh_move is one).
   Cost: one lane per record around the box-box sweep, the heaviest leaf test of the library, instantiated once per kernel.  Registers on gfx950 (hipcc
   -Rpass-analysis=kernel-resource-usage): k_q_move<box> 146 VGPRs (147 filtered) at 3 waves per SIMD, no scratch -- asked for nh_move's 4
   waves it spills 28 - 32 bytes per lane; k_q_walk<box> 194 VGPRs (195 filtered) at 2 waves, no scratch -- at nh_walk's 3 waves it spills 56 - 60 bytes
   per lane.  The capsule instantiations are unchanged: 128 VGPRs at 4 waves and 168 at 3.
   Measured (one MI355X, one run, the landed config-2 world of 1,004,524 colliders, 1,048,576 records, max_slides 4, the library's kernel timers, medians of 7
   blocks of 10 calls; tools/boxmove_rates.py -> profiles/boxmove_rates.log): nh_boxmove of the box (0.3, 0.5, 0.4) under random rotations
   1.365 ms beside 0.661 ms for nh_boxcast on the first casts alone, 1.378 casts per move: 1.50 of (casts per move x the box cast's time) at 3 waves per SIMD,
   where nh_move reported 1.03 at the cast's own 4.  nh_boxwalk of the upright box (0.3, 0.7, 0.3), snap 0.3, at 2 waves per SIMD: 2.817 ms with step_height 0
   (2.26 casts per walk), slope limit off or 45 degrees; 5.131 ms with step_height 1.0 and the limit off (3.32 casts), 5.357 ms with the limit at 45 degrees
   (3.70 casts), beside 0.757 ms for nh_boxcast on the first casts: 1.65, 1.65, 2.04 and 1.90 of (casts per walk x the box cast's time), where nh_walk
   reported 1.29 - 1.66 (11.5 % of these walks start in overlap and end after one cast: they are in the means).  Filter off, beside the parent commit's library
   loaded twice in the same process, per block this / parent with parent / parent beside it: nh_move 1.000 (0.991 .. 1.008) beside 0.997 (0.991 .. 1.001),
   nh_walk 1.000 (0.994 .. 1.003) beside 1.001 (0.998 .. 1.004), nh_boxcast 1.002 (0.999 .. 1.011) beside 1.000 (0.996 .. 1.011), nh_capsulecast 1.000
   (0.995 .. 1.005) beside 1.002 (0.996 .. 1.008): every median inside the parent's own spread.  NOT MEASURED YET: the filtered instantiations' times; what of
   the ratios is the lower occupancy and what is divergence; a third wave for the walk with the kept slide parked in the result record. */
typedef struct nh_BoxMove { float origin[3]; float skin; float displacement[3]; uint32_t ignore_body;
                            float rotation[4]; float size[3]; uint32_t max_slides; } nh_BoxMove;                 /* 64 B  = nh_BoxCast, skin at max_t, max_slides at reserved */
typedef struct nh_BoxWalk { float origin[3]; float skin; float displacement[3]; uint32_t ignore_body;
                            float rotation[4]; float size[3]; uint32_t max_slides;                               /* = nh_BoxMove, 64 B */
                            float up[3]; float step_height; float snap_distance; float min_ground_up;
                            uint32_t options; uint32_t reserved2; } nh_BoxWalk;                                  /* 96 B  = nh_Walk's tail behind nh_BoxMove */
int nh_boxmove(nh_context* ctx, const nh_BoxMove* moves, uint32_t count, nh_MoveResult* results, uint32_t flags /* 0 */);
int nh_boxwalk(nh_context* ctx, const nh_BoxWalk* walks, uint32_t count, nh_WalkResult* results, uint32_t flags /* 0 */);

/* nh_move_touched, nh_boxmove_touched, nh_walk_touched, nh_boxwalk_touched: the four movers, and beside each result THE LIST OF EVERYTHING THE MOVER
   TOUCHED -- what a controller needs to push the crate it slid into, fire a trigger, play the footstep of the right material, ride the lift it stands on.
   last_hit and ground are single records: a capsule that slides along the floor into a crate and then along a wall reports the wall only.  The list used to
   take the REPLAY identity run from the host, one cast call and one round trip per round; the kernels hold every hit in registers when it is taken, and these
   calls let it out, in ONE launch each.
   DEFINITION: each call is its plain mover word for word -- the same rules, the same casts, the same layer filter with the record's index as the per-query
   mask index -- and `results` receives byte for byte what the plain call writes.  Every cast the mover makes whose answer is a HIT -- a collider, whether
   taken with t > 0 or a start overlap with t == 0 -- produces one TOUCH, in the order the casts are made.  A miss touches nothing; an invalid cast from an
   overflowed position touches nothing.  The fields of a touch:
     hit                 the nh_RayHit of that cast, written by the routine that writes last_hit;
     origin, direction   the p and v the cast was made from and along (rule 2 of the move): the bits the state held before the advance;
     phase               NH_TOUCH_SLIDE for every cast of a move; for a walk the phase the cast was asked for in: A and its blocked form give SLIDE, U gives
                         UP, F gives FORWARD, D gives DOWN, C gives PROBE;
     cast                how many casts the record had made before this one: nh_WalkResult.casts before its increment; for a move, the round.
   counts[i] is the number of touches of record i WHATEVER k IS: at most NH_MOVE_MAX_SLIDES + 1 (9) for a move, NH_WALK_MAX_CASTS (21) for a walk.  Touch j
   of record i goes to touches[(size_t)i * k + j] for j < min(counts[i], k): all 64 bytes, the first k in order.  THE SLOTS BEHIND THOSE ARE NOT WRITTEN --
   the one place where the query calls' habit "every byte is written" is broken, on purpose: a million walks at k = 21 would otherwise store 1.3 GB of
   nothing.  Read counts[i] before touches: a slot at or behind it holds whatever the memory held.  An INVALID record writes the plain call's result,
   counts[i] = 0 and no touch.
   WHAT A WALK LISTS is everything it probed, kept or not; the result's flags tell kept from abandoned.  With NH_WALK_STEPPED set, UP, FORWARD and DOWN are
   the path taken and SLIDE holds what blocked it; without it, SLIDE and PROBE are the path and UP, FORWARD and DOWN are an attempt that was abandoned.  A
   small k can fill up with SLIDE touches before the kept ones arrive: counts[i] > k tells, and k = the maximum never loses one.
   IDENTITIES (contracts):
     T1. `results` holds byte for byte what the plain call writes for the same records, under every filter mode, after nh_query_refit as after a build;
     T2. REPLAY per touch: `hit` is byte for byte what the shape's closest-hit cast with flags 0 (nh_capsulecast, nh_boxcast) writes for { origin, 1.0f,
         direction, ignore_body, rotation, the shape } under the record's mask; half height 0 and size (0, 0, 0) follow the sphere's and the ray's rules as in
         the plain calls;
     T3. for a move, counts == slides + (flags & NH_MOVE_START_OVERLAP ? 1 : 0) and touch j has cast == j; where last_hit is a collider, the last touch's
         hit is last_hit;
     T4. for a walk, counts <= casts; `cast` is strictly ascending and < casts; `phase` never decreases; the touches with t > 0 of the kept slide (FORWARD if
         STEPPED, else SLIDE) number `slides`; with STEPPED the last DOWN touch's hit is `ground`; without it, where `ground` is a collider, the PROBE
         touch's hit is `ground`;
     T5. a smaller k writes the same counts, and the first min(counts, k) touches hold the same bytes.
   All four return NH_ERR_INVALID, in nh_move's order, before any nh_query_build, for flags != 0, for count >= 2^30, for k == 0 or k above 9 (the two moves)
   or 21 (the two walks), and for count > 0 with any of the four pointers null, the records, `results` or `touches` not 16-byte aligned, or `counts` not
   4-byte aligned; count = 0 is a no-op that returns NH_OK and launches nothing.  A refused call writes nothing.  Never allocate, never wait: ONE launch
   each on the context's stream (timing labels q_move_touched, q_boxmove_touched, q_walk_touched, q_boxwalk_touched).  OBSERVERS like nh_move (note 9).
   NOT BUILT: touches de-duplicated per body; a contact point (the casts return none: origin + t * direction is where the SHAPE's centre was); touches for
   nh_recover; pushing dynamic bodies and moving platforms inside the library (queries are observers: INTEGRATION.md, "touched", has the caller's recipe).
   (nh_overlap_bodies, above, de-duplicates LISTS OF nh_OverlapHit per body -- what nh_overlap and nh_region write.  A mover's touches are nh_Touch records,
   which it does not read: for them the de-duplication stays not built.)
   Cost: the mover's cost, and per touch four 16-byte stores (64 B) beside the tree walk of its cast, per record one 4-byte count; the lane holds the slot
   pointer, k and the count across the sweep.  Registers on gfx950 (hipcc -Rpass-analysis=kernel-resource-usage): the
   touched capsule move 128 VGPRs at 4 waves per SIMD and the touched box move 150 (151 filtered) at 3, their plain siblings' occupancy; the touched box walk
   198 (199 filtered) at 2, its sibling's; the touched capsule walk 182 (183 filtered) at 2 waves where nh_walk runs at 3 -- asked for 3 it spills 20 - 28
   bytes per lane.  None has scratch.  The eight plain instantiations are unchanged: 128 at 4, 146 / 147 at 3, 168 at 3, 194 / 195 at 2.
   Measured (one MI355X, one run, the landed config-2 world of 1,004,524 colliders, 1,048,576 records, max_slides 4, the workloads of move_rates, walk_rates
   and boxmove_rates, the library's kernel timers, medians of 7 blocks of 10 calls; tools/touched_rates.py -> profiles/touched_rates.log), the
   touched call at k = the maximum over the plain call per block: nh_move_touched 2.311 ms beside 2.307 ms, 1.002 (1.000 .. 1.010), 0.51 touches per move;
   nh_boxmove_touched 1.378 beside 1.363 ms, 1.008 (1.005 .. 1.012), 0.38 touches; nh_boxwalk_touched (step_height 1.0) 5.159 beside 5.123 ms, 1.006 (1.000 ..
   1.009), 1.39 touches per walk; nh_walk_touched (step_height 1.0) 6.396 beside 4.705 ms, 1.360 (1.353 .. 1.364), 1.29 touches per walk: the one kernel that
   gave up a wave.  k = 4 measures the same within 0.4 %: on these workloads at most 3 in 10,000 records have more than four touches.  The four plain movers
   beside the parent commit's library loaded twice in the same process, this / parent with parent / parent beside it: nh_move 1.000 (0.991 .. 1.005) beside
   1.001 (0.994 .. 1.009), nh_boxmove 1.001 (0.994 .. 1.005) beside 0.999 (0.992 .. 1.004), nh_walk 1.001 (0.994 .. 1.004) beside 0.999 (0.994 .. 1.002),
   nh_boxwalk 1.000 (0.997 .. 1.007) beside 1.001 (0.999 .. 1.002): every median inside the parent's own spread.  NOT MEASURED YET: the filtered
   instantiations' times; the touched capsule walk at 3 waves (it was compiled, not run); workloads where most records touch many colliders. */
enum { NH_TOUCH_SLIDE = 0u, NH_TOUCH_UP = 1u, NH_TOUCH_FORWARD = 2u, NH_TOUCH_DOWN = 3u, NH_TOUCH_PROBE = 4u };   /* nh_Touch.phase: nh_walk's A, U, F, D, C */
typedef struct nh_Touch { nh_RayHit hit; float origin[3]; uint32_t phase; float direction[3]; uint32_t cast; } nh_Touch;   /* 64 B */
int nh_move_touched   (nh_context* ctx, const nh_Move* moves,    uint32_t count, nh_MoveResult* results, uint32_t k, uint32_t* counts, nh_Touch* touches, uint32_t flags /* 0 */);
int nh_boxmove_touched(nh_context* ctx, const nh_BoxMove* moves, uint32_t count, nh_MoveResult* results, uint32_t k, uint32_t* counts, nh_Touch* touches, uint32_t flags /* 0 */);
int nh_walk_touched   (nh_context* ctx, const nh_Walk* walks,    uint32_t count, nh_WalkResult* results, uint32_t k, uint32_t* counts, nh_Touch* touches, uint32_t flags /* 0 */);
int nh_boxwalk_touched(nh_context* ctx, const nh_BoxWalk* walks, uint32_t count, nh_WalkResult* results, uint32_t k, uint32_t* counts, nh_Touch* touches, uint32_t flags /* 0 */);
/* the touches as impulse records for nh_body_impulses ("body impulses", above): out[i * k + j] of slot j of mover i, count x k records */
int nh_touch_impulses (nh_context* ctx, const nh_Push* pushes, uint32_t count, uint32_t k, const uint32_t* counts, const nh_Touch* touches, nh_BodyImpulse* out, uint32_t flags /* 0 */);

/* ---- multi-GPU: one x-slab of a world per context ------------------------------------------------------------------------------------
   The world is cut into slabs along x, one rank (process, GPU, nh_context) per slab [lo, hi).  A rank's arrays hold
       body slot 0            the static world with the static colliders the rank keeps (front of the collider arrays),
       slots 1 .. n_owned     the dynamic bodies whose centre lies in the slab: authoritative here,
       the tail               GHOSTS: copies of neighbour-owned bodies that may touch something owned here (left neighbour's first),
   and one collider per dynamic body, in body-slot order behind the static ones.  An `nh_partition` keeps the per-body collider description
   (shape, local transform, tag, kind), the slab, and the lists of who is sent where; everything below is device work on the context's
   stream with device-side counts -- what the host gets back are the message lengths it needs to post the messages.  TRANSPORT IS THE CALLER'S:
   records are written to / read from caller-provided device buffers (ncclSend / ncclRecv, torch.distributed ...);
   nudge_amd/partition.py and examples/partition_rccl.cpp are two such transports over these entry points.
     every `epoch` steps (and at step 0), REFRESH:
        [optional: re-balance -- nh_partition_choose_cut / nh_partition_set_cut]
        nh_partition_pack_migrants  -> exchange -> nh_partition_unpack_migrants     (bodies whose centre left the slab change owner)
        nh_partition_pack_ghosts    -> exchange -> nh_partition_unpack_ghosts       (owned bodies that can reach across a cut within the epoch; collider arrays rebuilt)
     every other step:
        nh_partition_pack_step      -> exchange -> nh_partition_unpack_step         (64-byte records of the listed bodies, fixed lengths)
   Reference counterpart: none (the reference is single-threaded); the contact identity that makes this work is the collider TAG
   (nudge.h:86, 93; nudge.cpp:2074-2087), which travels with a body.  A dynamic body carries up to NH_PARTITION_MAX_COLLIDERS colliders (compound bodies); in the
   collider arrays the colliders of dynamic bodies stand in body-slot order, a body's own adjacent (boxes in the box array, spheres in the sphere array). */
#define NH_PARTITION_MAX_COLLIDERS 4     /* colliders a dynamic body may carry across ranks (compound bodies, nudge.cpp:3023-3025, 3058-3060): its boxes, then its spheres */
#define NH_PARTITION_FULL_BYTES 308      /* transform 32 | properties 16 | momentum 32 | 4 x (shape 16 | collider transform 32 | tag 4 | pad 4) | boxes 1, spheres 1, idle 1, pad 1 */
typedef struct nh_partition nh_partition;
typedef struct nh_PartitionConfig {
	uint32_t rank, ranks;
	double lo, hi;                                      /* the slab along x; -HUGE_VAL / HUGE_VAL at the two ends */
	uint32_t n_owned;                                   /* dynamic bodies in slots 1 .. n_owned at creation */
	uint32_t n_static_box, n_static_sph;                /* static colliders at the front of the collider arrays (never touched) */
	uint32_t body_capacity, box_capacity, sphere_capacity;   /* records the caller's arrays have room for */
	uint32_t epoch;                                     /* steps between two refreshes */
	double time_step, gravity, speed_floor;             /* how far a body can travel in an epoch: epoch dt (max(top speed, floor) + g epoch dt) */
	double max_reach;                                   /* largest distance from a body origin to the far side of its collider, over the WHOLE world */
	double cut_slack;                                   /* a cut never moves further than this from where it started (static colliders kept); HUGE_VAL = unlimited */
} nh_PartitionConfig;
typedef struct nh_PartitionInfo {
	uint32_t n_owned, n_bodies, n_boxes, n_spheres;     /* bodies = 1 + owned + ghosts; colliders incl. the static ones */
	uint32_t ghost_out[2], ghost_in[2];                 /* [0] left neighbour, [1] right neighbour: bodies listed for / received from it at the last refresh */
	double lo, hi;
	uint64_t migrated_out, migrated_in, refreshes, cut_moves;
	uint64_t quiet_refreshes;                           /* refreshes this rank found it did not need (nh_partition_refresh_is_quiet said 1) */
} nh_PartitionInfo;
/* `bodies` / `colliders`: the rank's arrays as they are at creation (1 + n_owned bodies; the static colliders, then the dynamic bodies' in slot order, Transform.body = slot). */
int nh_partition_create(nh_partition** out, nh_context* ctx, const nh_PartitionConfig* config, const nh_BodyData* bodies, const nh_ColliderData* colliders);
void nh_partition_destroy(nh_partition* p);
int nh_partition_info(nh_partition* p, nh_PartitionInfo* out);
/* Refresh, phase 1.  pack: full records of the owned bodies whose centre is left of lo -> out_left, right of (or on) hi -> out_right (device buffers of `capacity_records`
   records each; either may be NULL at an end of the row); counts[0..1] = records written (the call synchronises the stream once to tell).
   unpack: the leavers are dropped (owned bodies stay in slot order), the arrivals appended, left neighbour's first; ghosts are gone until phase 2. */
int nh_partition_pack_migrants(nh_partition* p, const nh_BodyData* bodies, void* out_left, void* out_right, uint32_t capacity_records, uint32_t counts[2]);
int nh_partition_unpack_migrants(nh_partition* p, const nh_BodyData* bodies, const void* in_left, uint32_t n_left, const void* in_right, uint32_t n_right);
/* Between the two phases -- or before phase 1, with its counts -- the ranks at a cut tell each other their TOP SPEED: a cut's ghost margin is reach + 2 x (how far anything
   on EITHER side travels in an epoch), so it must know the fastest body of the neighbour too (a fast body owned there reaches a slow one here that this rank would
   otherwise never list for it).  nh_partition_top_speed: the largest |velocity| among the bodies this rank owns now (call it BEFORE nh_partition_pack_migrants: a body that
   migrates in this refresh then counts on both sides); nh_partition_set_peer_speeds: what the left / right neighbour reported (NAN or <= 0: none).  Both are consumed by the
   next nh_partition_pack_ghosts; a host that never calls them gets margins from this rank's own top speed and `speed_floor` alone -- safe only when the floor bounds the world. */
int nh_partition_top_speed(nh_partition* p, const nh_BodyData* bodies, double* out);
/* A QUIET refresh (round 6): *quiet = 1 when a refresh would change nothing on this rank -- no owned body has crossed a cut, and the bodies within reach of a cut (at the
   speeds of nh_partition_top_speed / nh_partition_set_peer_speeds: call those first; nothing is consumed) are exactly the ones listed for the neighbours at the last
   refresh, in the same order.  When EVERY rank of the job says so the host may skip the refresh and exchange a per-step halo instead (nudge_amd/partition.py does, with an
   all-reduce of the answers): the still steps of a world at rest then run through the epoch boundary.  Never 1 before the first refresh.  One stream synchronisation. */
int nh_partition_refresh_is_quiet(nh_partition* p, const nh_BodyData* bodies, int* quiet);
int nh_partition_set_peer_speeds(nh_partition* p, double left, double right);
/* Refresh, phase 2.  pack: the owned bodies within reach of a cut for the coming epoch are listed (the lists are kept for the per-step records) and their full
   records written.  unpack: the received ghosts are installed behind the owned bodies, the collider arrays rebuilt (static ones, then one per dynamic body in
   slot order), `bodies->count` and the collider counts of the caller's structs set, and the context told that body records changed (nh_bodies_changed). */
int nh_partition_pack_ghosts(nh_partition* p, const nh_BodyData* bodies, void* out_left, void* out_right, uint32_t capacity_records, uint32_t counts[2]);
int nh_partition_unpack_ghosts(nh_partition* p, nh_BodyData* bodies, nh_ColliderData* colliders, const void* in_left, uint32_t n_left, const void* in_right, uint32_t n_right);
/* Every other step: NH_HALO_RECORD_BYTES per listed body (nh_halo_pack's record); lengths are those of the last refresh (nh_partition_info: ghost_out / ghost_in). */
int nh_partition_pack_step(nh_partition* p, const nh_BodyData* bodies, void* out_left, void* out_right);
int nh_partition_unpack_step(nh_partition* p, const nh_BodyData* bodies, const void* in_left, const void* in_right);
/* The per-step halo driven by the library: nh_partition_exchange_step = pack -> ncclGroupStart; ncclSend / ncclRecv with both neighbours; ncclGroupEnd -> unpack, all
   enqueued on the context's stream in ONE call (the host's share of a step shrinks to two calls: this one and nh_step).  The library does not link RCCL: the host hands
   it an ncclComm_t of the world's ranks and the addresses of ncclGroupStart / ncclGroupEnd / ncclSend / ncclRecv of the RCCL library its process has loaded
   (nh_partition_set_transport; left_peer / right_peer: communicator ranks of the neighbours, -1 = none).  nh_partition_transport_check sends a pattern to both peers and
   receives theirs in one group (a peer equal to the own rank: a loop-back on one GPU); with enqueue_only the host polls the stream itself -- a neighbour that never answers must not hang
   it -- and fetches the verdict with nh_partition_transport_result. */
/* (nh_partition_transport_check may re-size the message buffers: after an enqueue_only check call nh_partition_transport_result BEFORE the next exchange or check.
   An RCCL call that fails makes the exchange return NH_ERR_HIP with the group closed; nh_last_hip_error then holds the ncclResult_t, negated.) */
int nh_partition_set_transport(nh_partition* p, void* comm, void* group_start, void* group_end, void* send, void* recv, int left_peer, int right_peer);
int nh_partition_exchange_step(nh_partition* p, const nh_BodyData* bodies);
/* K sub-steps of a slab in ONE call (the loop example/main.cpp:274-328 runs for a partitioned world: halo exchange, then the eight calls, K times): nh_step with the per-step
   exchange enqueued by the library between two sub-steps over the transport of nh_partition_set_transport (needed as soon as there is a ghost on either side).  The
   chain of still steps (note 9: xform ahead, pair ahead) runs through such a call for the OWNED bodies; ghosts' colliders are transformed and their pairs evaluated when
   the halo has arrived.  `exchange_first`: the first sub-step is preceded by a per-step exchange too (0 right after a refresh, which has just installed the ghosts).
   `loopback_records` (rehearsal on one rank): that many owned bodies' records also travel through the transport to this same rank every sub-step.  K must not reach past
   the next refresh: migration and ghost lists are the host's (nh_partition_pack_migrants ...). */
int nh_partition_step(nh_partition* p, const nh_StepArgs* args, uint32_t steps, uint32_t exchange_first, uint32_t loopback_records);
int nh_partition_transport_check(nh_partition* p, uint32_t bytes, int enqueue_only);
int nh_partition_transport_result(nh_partition* p);
/* Re-balancing ("move cuts when |count_r - mean| > 5 %").  The two ranks at a cut tell each other how many bodies they own (transport: caller); when the
   counts differ by more than `tolerance` of their sum the HEAVIER side calls nh_partition_choose_cut(direction, neighbour's count) -- the x that hands half the
   difference, at most 5 % of its bodies, to the neighbour; it moves its own cut and returns it -- and sends the value over; the lighter side calls nh_partition_set_cut.
   The bodies in between migrate with the refresh that follows.  direction: -1 = the cut towards the left neighbour, +1 = towards the right. */
int nh_partition_choose_cut(nh_partition* p, const nh_BodyData* bodies, int direction, uint32_t neighbour_owned, double* cut);
int nh_partition_set_cut(nh_partition* p, int direction, double cut);
/* One owner per contact that crosses a cut (SURVEY 8(e) "determinism rule": the contact is owned by the rank owning the body with the larger collider tag, mirroring the
   a > b canonicalisation of nudge.cpp:2074-2087 / 2131-2132).  With first_ghost > 0 the bodies [first_ghost, count) of the context's world are ghosts and nh_collide makes
   contacts only for collider pairs this rank owns: a pair with the static world belongs to its dynamic body, a pair of two dynamic bodies to the body whose collider has the
   larger tag -- if that body is a ghost here, the pair yields no contact on this rank (the rank that owns the body solves it).  The host returns what the solver did to the
   ghosts (momentum after a sweep minus before) to their owners and refreshes the ghosts from the owners after every nh_apply_impulses(..., 1): nudge_amd/partition.py
   `Partition(per_iteration=True, single_owner=True)`.  0 switches the rule off.  Still steps (note 9) are not launched while it is on. */
int nh_set_first_ghost_body(nh_context* ctx, uint32_t first_ghost);
/* ... and the per-iteration exchange that goes with it, behind the C ABI (round 5; the torch form in nudge_amd/partition.py is kept as the independent check).  Records are
   the 32-byte nh_BodyMomentum; lengths are the ghost lists of the last refresh (nh_partition_info: a rank SENDS ghost_in[side] deltas and ghost_out[side] momentum records
   to the neighbour on that side and receives the other number), in the neighbour's list order.  One step of a rank (examples/partition_rccl.cpp --single-owner):
       nh_set_first_ghost_body(n_owned + 1); nh_collide; gravity; nh_read_cached_impulses; nh_partition_mark_ghosts; nh_setup_contact_constraints; EXCHANGE;
       iterations x { even ranks: nh_apply_impulses(.., 1); EXCHANGE; odd ranks: nh_apply_impulses(.., 1); EXCHANGE }; update; write; advance
       EXCHANGE = pack_deltas -> transport -> unpack_deltas (owners add what the neighbours' sweeps did to their bodies); pack_momentum -> transport -> unpack_momentum
                  (ghosts take their owners' momentum); mark_ghosts -- or nh_partition_exchange_iteration, which does all of it over the transport of nh_partition_set_transport.
   Every call first completes deferred work (note 7), so the warm start is in the momentum the records are taken from. */
int nh_partition_mark_ghosts(nh_partition* p, const nh_BodyData* bodies);
int nh_partition_pack_deltas(nh_partition* p, const nh_BodyData* bodies, void* out_left, void* out_right);
int nh_partition_unpack_deltas(nh_partition* p, const nh_BodyData* bodies, const void* in_left, const void* in_right);
int nh_partition_pack_momentum(nh_partition* p, const nh_BodyData* bodies, void* out_left, void* out_right);
int nh_partition_unpack_momentum(nh_partition* p, const nh_BodyData* bodies, const void* in_left, const void* in_right);
int nh_partition_exchange_iteration(nh_partition* p, const nh_BodyData* bodies);

/* ---- introspection for tests / measurement --------------------------------------------------------- */
/* Device pointer to the per-contact warm-start impulses of an nh_ContactImpulseData (K x 16 B, contact order). */
const nh_CachedContactImpulse* nh_contact_impulses_device(const nh_ContactImpulseData* d);
/* Per-kernel device time of the last step, measured with HIP events on the context's stream when timing is on. */
int nh_enable_timing(nh_context* ctx, int on);
/* Restrict timing to kernels whose name equals `name` (NULL or "" = all): two events per step instead of hundreds.  (With timing of ALL kernels on, nh_step looks at every
   still step's verdict inside the step -- the events are collected at that round trip; restricted to one kernel it keeps its late verdicts and collects at the end of the call.) */
int nh_set_timing_filter(nh_context* ctx, const char* name);
/* Writes up to `cap` (name, milliseconds, launches) triples accumulated since the last reset; returns the number. */
typedef struct nh_KernelTime { const char* name; double ms; uint32_t launches; uint32_t reserved; } nh_KernelTime;
int nh_kernel_times(nh_context* ctx, nh_KernelTime* out, int cap, int reset);

#ifdef __cplusplus
}
#endif

#endif /* NUDGE_HIP_H */
