// nh_still.h -- what the kernels around a still step must compute ALIKE, stated once (device code: it touches nh_DevState and wave intrinsics; the pure
// arithmetic they share -- a collider's pose, reach and AABB, the role rule, a pair's contacts -- is NH_HD in nh_math.h / nh_narrowphase.h, where tests/hostsim
// compiles it too).  A still step is correct only when the kernel that does a piece of work AHEAD (the solver's lanes, k_xform_ghosts, k_pair_begin) files the
// very bits the full step's kernel (k_xform, k_kept_filter, k_narrowphase) would have filed.  Who calls what, and which sites keep lines of their own:
// docs/KERNELS.md, "Shared between the still step's kernels".
#ifndef NH_STILL_H
#define NH_STILL_H

#include "nh_internal.h"
#include "nh_math.h"

// ---- scene bounds: the min corners of the exact AABBs in an order-preserving encoding (the Morton frame's, nudge.cpp:3086-3100) -------------------------
__device__ __forceinline__ void nh_bounds_fold(uint32_t (&lmin)[3], uint32_t (&lmax)[3], float x, float y, float z) {
	uint32_t f;
	f = nh_float_flip(x); lmin[0] = min(lmin[0], f); lmax[0] = max(lmax[0], f);
	f = nh_float_flip(y); lmin[1] = min(lmin[1], f); lmax[1] = max(lmax[1], f);
	f = nh_float_flip(z); lmin[2] = min(lmin[2], f); lmax[2] = max(lmax[2], f);
}
__device__ __forceinline__ nh_f3 nh_bounds_corner(const uint32_t (&f)[3]) { return nh_make3(nh_float_unflip(f[0]), nh_float_unflip(f[1]), nh_float_unflip(f[2])); }

// ---- this step's scene frame from the parts the LAST step's solver lanes (and k_xform_ghosts) gathered in NH_AHEAD_PARTS places, the static world's share
// beside them.  Two halves, so that a kernel can ask for more between them and wait once for all of it: the fetch, and every wave's reduction for itself ----
__device__ __forceinline__ void nh_pair_frame_fetch(const nh_DevState* __restrict__ st, uint32_t parity, uint32_t lane, uint32_t (&fr_min)[3], uint32_t (&fr_max)[3], uint32_t& fr_top) {
	const uint32_t* part = &st->ahead_part[parity][lane & (NH_AHEAD_PARTS - 1u)][0];
	fr_top = part[6];          // (the largest idle counter)
	for (int k = 0; k < 3; ++k) { fr_min[k] = min(part[k], st->still_static_min[k]); fr_max[k] = max(part[3 + k], st->still_static_max[k]); }
}
__device__ __forceinline__ void nh_pair_frame_reduce(uint32_t (&fr_min)[3], uint32_t (&fr_max)[3], uint32_t& fr_top) {
	for (int k = 0; k < 3; ++k)
		for (int d = 32; d >= 1; d >>= 1) { fr_min[k] = min(fr_min[k], (uint32_t)__shfl_xor((int)fr_min[k], d)); fr_max[k] = max(fr_max[k], (uint32_t)__shfl_xor((int)fr_max[k], d)); }
	for (int d = 32; d >= 1; d >>= 1) fr_top = max(fr_top, (uint32_t)__shfl_xor((int)fr_top, d));
}

// ---- what the NEXT step (the other parity) accumulates into: whoever opens a still step clears it -- k_xform<true>, or the narrowphase / k_pair_begin of a step
// that has none, or the full step's k_collide_begin.  Nobody touches the other parity's words during this step before the solver that gathers into them ----
__device__ __forceinline__ void nh_still_open_next(nh_DevState* st, uint32_t op) {
	st->max_idle[op] = 0u; st->delta_count[op] = 0u; st->delta_overflow[op] = 0u; st->still_esc[op] = 0u;
	st->still_asleep[op] = 0u; st->still_sleeping[op] = 0u; st->still_culled[op] = 0u;
	for (int k = 0; k < 3; ++k) { st->still_smin[op][k] = 0xffffffffu; st->still_smax[op][k] = 0u; }
}
// (xform ahead, nh_internal.h: what this step's solver may gather for the next step -- `thread` of `stride` threads of ONE workgroup)
__device__ __forceinline__ void nh_ahead_parts_reset(nh_DevState* st, uint32_t op, uint32_t thread, uint32_t stride) {
	for (uint32_t k = thread; k < NH_AHEAD_PARTS * 8u; k += stride) (&st->ahead_part[op][0][0])[k] = (k & 7u) < 3u ? 0xffffffffu : 0u;
}

// (the role rule of nh_math.h over two AABB min corners as the kernels hold them)
__device__ __forceinline__ bool nh_a_is_first(const float4& amin, const float4& bmin, uint32_t ca, uint32_t cb, float mscale, const nh_f3& mmin) {
	return nh_a_is_first(nh_make3(amin.x, amin.y, amin.z), nh_make3(bmin.x, bmin.y, bmin.z), ca, cb, mscale, mmin);
}

#endif
