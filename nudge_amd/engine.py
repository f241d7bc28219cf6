"""ctypes binding of libnudge_hip.so (include/nudge_hip.h) + a `World` convenience wrapper.

Host-side plumbing only: torch owns the device arrays (plain uint8 tensors reinterpreted as the POD records
of nudge_hip.h), the HIP stream is torch's current stream, and every entry point of the step loop is the
C-ABI function that replaces the reference call of the same name (reference example/main.cpp:274-328).

There is NO CPU fallback: importing works anywhere, but constructing a `World` raises unless the HIP
library is built and a GPU is visible.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import warnings

import numpy as np

from . import scenes as S

_HERE = os.path.dirname(os.path.abspath(__file__))
# NUDGE_HIP_LIBRARY: another build of the same library (A/B timing of kernel variants on one box)
_LIB_PATH = os.environ.get("NUDGE_HIP_LIBRARY") or os.path.join(_HERE, "libnudge_hip.so")
_LIB = None

NH_FLAG_SYNC_COUNTS = 1
NH_FLAG_EXACT_ORDER = 2
NH_FLAG_SINGLE_APPLY = 4
NH_FLAG_FUSED_STEP = 8
NH_VIEW_CONTACTS, NH_VIEW_CACHE, NH_VIEW_ACTIVE, NH_VIEW_ALL = 1, 2, 4, 7
# environment variables NH_<NAME> that World() forwards to nh_set_option (tests and dev scripts; include/nudge_hip.h lists what each does)
OPTION_NAMES = ("no_still", "no_kept_pairs", "no_incremental", "no_sort_reuse", "sort_radix", "bucket_tile", "bucket_target",
                "colour_check_seeds", "no_resident", "no_blocks", "blk_check", "blk_min", "blk_target", "blk_rows_global",
                "blk_global_colours", "blk_profile", "no_asleep", "no_blk_chain", "no_local_still", "no_xform_ahead", "sync_exports_views", "no_pair_ahead", "no_sleeper_skip", "halo_overlap", "no_early_counts", "no_sleeper_ahead", "no_listed_lookup")

EXPORTS = [
    "nh_create", "nh_destroy", "nh_set_flags", "nh_synchronize", "nh_read_counts", "nh_export_views", "nh_set_cache_count",
    "nh_set_tag_bits", "nh_set_pair_capacity", "nh_set_option", "nh_bodies_changed", "nh_error_string", "nh_last_hip_error", "nh_collide", "nh_apply_gravity_damping",
    "nh_read_cached_impulses", "nh_write_cached_impulses", "nh_setup_contact_constraints", "nh_apply_impulses",
    "nh_update_cached_impulses", "nh_advance", "nh_contact_impulses_device", "nh_enable_timing", "nh_set_timing_filter", "nh_kernel_times",
    "nh_halo_pack", "nh_halo_unpack", "nh_halo_update", "nh_append_contacts", "nh_step", "nh_stream_state", "nh_stream_latest",
    "nh_partition_create", "nh_partition_destroy", "nh_partition_info", "nh_partition_pack_migrants", "nh_partition_unpack_migrants", "nh_partition_pack_ghosts",
    "nh_partition_top_speed", "nh_partition_set_peer_speeds", "nh_partition_refresh_is_quiet", "nh_partition_mark_ghosts", "nh_partition_pack_deltas", "nh_partition_unpack_deltas",
    "nh_partition_pack_momentum", "nh_partition_unpack_momentum", "nh_partition_exchange_iteration", "nh_partition_unpack_ghosts", "nh_partition_pack_step", "nh_partition_unpack_step", "nh_partition_choose_cut", "nh_partition_set_cut",
    "nh_partition_set_transport", "nh_partition_exchange_step", "nh_partition_step", "nh_partition_transport_check", "nh_partition_transport_result", "nh_set_first_ghost_body",
    "nh_query_build", "nh_query_refit", "nh_query_stats", "nh_raycast", "nh_overlap", "nh_penetration", "nh_region", "nh_spherecast", "nh_raycast_all", "nh_spherecast_all", "nh_boxcast_all", "nh_capsulecast_all", "nh_boxcast", "nh_capsulecast", "nh_closest", "nh_closest_k", "nh_distance", "nh_move", "nh_recover", "nh_walk", "nh_boxmove", "nh_boxwalk",
    "nh_raycast_k", "nh_spherecast_k", "nh_boxcast_k", "nh_capsulecast_k",
    "nh_move_touched", "nh_boxmove_touched", "nh_walk_touched", "nh_boxwalk_touched",
    "nh_query_set_layers", "nh_query_filter", "nh_query_layer_info",
    "nh_overlap_bodies", "nh_overlap_events",
    "nh_overlap_wide", "nh_penetration_wide",
    "nh_contact_pairs", "nh_contact_events", "nh_step_contact_pairs",
    "nh_sense", "nh_sense_rays",
    "nh_impulse_sums", "nh_body_impulses", "nh_blast_impulses", "nh_touch_impulses",
    "nh_sweep", "nh_sweep_limit",
    "nh_joints_prepare", "nh_joints_setup", "nh_joints_apply", "nh_joint_connections",
]
HALO_RECORD_BYTES = 64


class Arena(C.Structure):
    _fields_ = [("data", C.c_void_p), ("size", C.c_size_t)]


class ContactData(C.Structure):
    _fields_ = [("data", C.c_void_p), ("bodies", C.c_void_p), ("tags", C.c_void_p), ("features", C.c_void_p),
                ("capacity", C.c_uint32), ("count", C.c_uint32), ("sleeping_pairs", C.c_void_p), ("sleeping_count", C.c_uint32)]


class _Shapes(C.Structure):
    _fields_ = [("tags", C.c_void_p), ("data", C.c_void_p), ("transforms", C.c_void_p), ("count", C.c_uint32)]


class ColliderData(C.Structure):
    _fields_ = [("boxes", _Shapes), ("spheres", _Shapes)]


class BodyData(C.Structure):
    _fields_ = [("transforms", C.c_void_p), ("properties", C.c_void_p), ("momentum", C.c_void_p),
                ("idle_counters", C.c_void_p), ("count", C.c_uint32)]


class BodyConnections(C.Structure):
    _fields_ = [("data", C.c_void_p), ("count", C.c_uint32)]


class ContactCache(C.Structure):
    _fields_ = [("tags", C.c_void_p), ("features", C.c_void_p), ("data", C.c_void_p), ("capacity", C.c_uint32), ("count", C.c_uint32)]


class ActiveBodies(C.Structure):
    _fields_ = [("indices", C.c_void_p), ("capacity", C.c_uint32), ("count", C.c_uint32)]


class Counts(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("colliders", "pairs", "contacts", "sleeping_pairs", "active_bodies", "cache", "culled",
                                          "large_colliders", "general_contacts", "levels", "error", "has_other_bodies", "unleveled", "raw_pairs", "broadphase_rebuilds", "sort_reuses", "broadphase_inserts",
                                          "still_steps", "still_replays", "still_diff_key", "still_diff_count", "still_diff_feature", "still_diff_escape",
                                          "blk_blocks", "blk_bodies", "blk_ghosts", "asleep_steps", "ahead_steps", "fused_steps", "pair_steps", "pair_diag_roles", "pair_diag_record", "pair_diag_scale", "pair_diag_owned")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class StepArgs(C.Structure):
    _fields_ = [("active_bodies", C.POINTER(ActiveBodies)), ("contacts", C.POINTER(ContactData)), ("bodies", C.POINTER(BodyData)), ("colliders", C.POINTER(ColliderData)),
                ("body_connections", C.POINTER(BodyConnections)), ("contact_cache", C.POINTER(ContactCache)), ("arena", Arena),
                ("time_step", C.c_float), ("gravity", C.c_float * 3), ("damping_rate", C.c_float), ("iterations", C.c_uint32)]


class PartitionConfig(C.Structure):
    _fields_ = [("rank", C.c_uint32), ("ranks", C.c_uint32), ("lo", C.c_double), ("hi", C.c_double), ("n_owned", C.c_uint32), ("n_static_box", C.c_uint32), ("n_static_sph", C.c_uint32),
                ("body_capacity", C.c_uint32), ("box_capacity", C.c_uint32), ("sphere_capacity", C.c_uint32), ("epoch", C.c_uint32),
                ("time_step", C.c_double), ("gravity", C.c_double), ("speed_floor", C.c_double), ("max_reach", C.c_double), ("cut_slack", C.c_double)]


class PartitionInfo(C.Structure):
    _fields_ = [("n_owned", C.c_uint32), ("n_bodies", C.c_uint32), ("n_boxes", C.c_uint32), ("n_spheres", C.c_uint32), ("ghost_out", C.c_uint32 * 2), ("ghost_in", C.c_uint32 * 2),
                ("lo", C.c_double), ("hi", C.c_double), ("migrated_out", C.c_uint64), ("migrated_in", C.c_uint64), ("refreshes", C.c_uint64), ("cut_moves", C.c_uint64), ("quiet_refreshes", C.c_uint64)]


class QueryStats(C.Structure):
    _fields_ = [("colliders", C.c_uint32), ("run_length", C.c_uint32), ("runs", C.c_uint32), ("top_nodes", C.c_uint32), ("top_depth", C.c_uint32)]


class QueryLayerInfo(C.Structure):
    _fields_ = [("set", C.c_uint32), ("colliders", C.c_uint32), ("any_layers", C.c_uint32), ("reserved", C.c_uint32)]


class Ray(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("max_t", C.c_float), ("direction", C.c_float * 3), ("ignore_body", C.c_uint32)]


class RayHit(C.Structure):
    _fields_ = [("t", C.c_float), ("normal", C.c_float * 3), ("body", C.c_uint32), ("collider", C.c_uint32), ("shape", C.c_uint32), ("tag", C.c_uint32)]


class SphereCast(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("max_t", C.c_float), ("direction", C.c_float * 3), ("ignore_body", C.c_uint32), ("radius", C.c_float),
                ("reserved", C.c_uint32 * 3)]


class BoxCast(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("max_t", C.c_float), ("direction", C.c_float * 3), ("ignore_body", C.c_uint32), ("rotation", C.c_float * 4),
                ("size", C.c_float * 3), ("reserved", C.c_uint32)]


class CapsuleCast(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("max_t", C.c_float), ("direction", C.c_float * 3), ("ignore_body", C.c_uint32), ("rotation", C.c_float * 4),
                ("radius", C.c_float), ("half_height", C.c_float), ("reserved", C.c_uint32 * 2)]


class PointQuery(C.Structure):
    _fields_ = [("point", C.c_float * 3), ("max_distance", C.c_float), ("ignore_body", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class PointHit(C.Structure):
    _fields_ = [("distance", C.c_float), ("normal", C.c_float * 3), ("point", C.c_float * 3), ("body", C.c_uint32), ("collider", C.c_uint32),
                ("shape", C.c_uint32), ("tag", C.c_uint32), ("reserved", C.c_uint32)]


NH_FILTER_OFF, NH_FILTER_UNIFORM, NH_FILTER_PER_QUERY = 0, 1, 2      # nh_query_filter modes (include/nudge_hip.h, "layer masks")
# scene queries (include/nudge_hip.h, "scene queries"): nh_RayHit.shape (CAPSULE: a query shape only), nh_raycast flags; numpy forms of the records
NH_SHAPE_BOX, NH_SHAPE_SPHERE, NH_SHAPE_CAPSULE, NH_SHAPE_NONE = 0, 1, 2, 0xFFFFFFFF
NH_RAY_ANY_HIT = 1
RAY = np.dtype([("origin", "<f4", 3), ("max_t", "<f4"), ("direction", "<f4", 3), ("ignore_body", "<u4")])
RAY_HIT = np.dtype([("t", "<f4"), ("normal", "<f4", 3), ("body", "<u4"), ("collider", "<u4"), ("shape", "<u4"), ("tag", "<u4")])
SPHERE_CAST = np.dtype([("origin", "<f4", 3), ("max_t", "<f4"), ("direction", "<f4", 3), ("ignore_body", "<u4"), ("radius", "<f4"), ("reserved", "<u4", 3)])
BOX_CAST = np.dtype([("origin", "<f4", 3), ("max_t", "<f4"), ("direction", "<f4", 3), ("ignore_body", "<u4"), ("rotation", "<f4", 4), ("size", "<f4", 3),
                     ("reserved", "<u4")])
CAPSULE_CAST = np.dtype([("origin", "<f4", 3), ("max_t", "<f4"), ("direction", "<f4", 3), ("ignore_body", "<u4"), ("rotation", "<f4", 4), ("radius", "<f4"),
                         ("half_height", "<f4"), ("reserved", "<u4", 2)])
OVERLAP_QUERY = np.dtype([("center", "<f4", 3), ("shape", "<u4"), ("rotation", "<f4", 4), ("size", "<f4", 3), ("ignore_body", "<u4")])
OVERLAP_HIT = np.dtype([("body", "<u4"), ("collider", "<u4"), ("shape", "<u4"), ("tag", "<u4")])
PENETRATION_HIT = np.dtype([("normal", "<f4", 3), ("depth", "<f4"), ("body", "<u4"), ("collider", "<u4"), ("shape", "<u4"), ("tag", "<u4")])
POINT_QUERY = np.dtype([("point", "<f4", 3), ("max_distance", "<f4"), ("ignore_body", "<u4"), ("reserved", "<u4", 3)])
POINT_HIT = np.dtype([("distance", "<f4"), ("normal", "<f4", 3), ("point", "<f4", 3), ("body", "<u4"), ("collider", "<u4"), ("shape", "<u4"), ("tag", "<u4"),
                      ("reserved", "<u4")])
DISTANCE_QUERY = np.dtype([("center", "<f4", 3), ("shape", "<u4"), ("rotation", "<f4", 4), ("size", "<f4", 3), ("ignore_body", "<u4"), ("max_distance", "<f4"),
                           ("reserved", "<u4", 3)])
# nh_move (include/nudge_hip.h): nh_CapsuleCast with `skin` where max_t is and `max_slides` where reserved[0] is; nh_MoveResult.flags
MOVE = np.dtype([("origin", "<f4", 3), ("skin", "<f4"), ("displacement", "<f4", 3), ("ignore_body", "<u4"), ("rotation", "<f4", 4), ("radius", "<f4"),
                 ("half_height", "<f4"), ("max_slides", "<u4"), ("reserved", "<u4")])
MOVE_RESULT = np.dtype([("position", "<f4", 3), ("flags", "<u4"), ("remaining", "<f4", 3), ("slides", "<u4"), ("last_hit", RAY_HIT)])
NH_MOVE_MAX_SLIDES = 8
NH_MOVE_HIT, NH_MOVE_START_OVERLAP, NH_MOVE_SLIDES_OUT, NH_MOVE_WEDGED, NH_MOVE_INVALID = 1, 2, 4, 8, 0x80000000
# nh_walk (include/nudge_hip.h): nh_Move followed by `up`, the step height, the snap distance, the slope limit (a cosine) and the options; nh_WalkResult.flags
WALK = np.dtype(MOVE.descr + [("up", "<f4", 3), ("step_height", "<f4"), ("snap_distance", "<f4"), ("min_ground_up", "<f4"), ("options", "<u4"), ("reserved2", "<u4")])
WALK_RESULT = np.dtype(MOVE_RESULT.descr + [("ground", RAY_HIT), ("step_up", "<f4"), ("drop", "<f4"), ("casts", "<u4"), ("reserved", "<u4")])
NH_WALK_MAX_CASTS = 2 * (NH_MOVE_MAX_SLIDES + 1) + 3
NH_WALK_STEPPED, NH_WALK_GROUNDED, NH_WALK_SNAPPED, NH_WALK_STEEP, NH_WALK_ON_STEEP, NH_WALK_INVALID = 0x10, 0x20, 0x40, 0x80, 0x100, 0x80000000
NH_WALK_PROBE_ONLY = 1
# nh_boxmove, nh_boxwalk (include/nudge_hip.h): nh_BoxCast with `skin` where max_t is and `max_slides` where reserved is, and nh_Walk's tail behind it; the
# results are MOVE_RESULT and WALK_RESULT
BOX_MOVE = np.dtype([("origin", "<f4", 3), ("skin", "<f4"), ("displacement", "<f4", 3), ("ignore_body", "<u4"), ("rotation", "<f4", 4), ("size", "<f4", 3),
                     ("max_slides", "<u4")])
BOX_WALK = np.dtype(BOX_MOVE.descr + WALK.descr[len(MOVE.descr):])
# nh_move_touched and kin (include/nudge_hip.h): one nh_Touch per cast of a mover that found a collider; nh_Touch.phase
TOUCH = np.dtype([("hit", RAY_HIT), ("origin", "<f4", 3), ("phase", "<u4"), ("direction", "<f4", 3), ("cast", "<u4")])
NH_TOUCH_SLIDE, NH_TOUCH_UP, NH_TOUCH_FORWARD, NH_TOUCH_DOWN, NH_TOUCH_PROBE = 0, 1, 2, 3, 4
NH_MOVE_MAX_TOUCHES, NH_WALK_MAX_TOUCHES = NH_MOVE_MAX_SLIDES + 1, NH_WALK_MAX_CASTS
# nh_recover (include/nudge_hip.h): nh_OverlapQuery followed by `skin` and `max_iterations`; nh_RecoverResult.flags
RECOVER = np.dtype([("center", "<f4", 3), ("shape", "<u4"), ("rotation", "<f4", 4), ("size", "<f4", 3), ("ignore_body", "<u4"), ("skin", "<f4"),
                    ("max_iterations", "<u4"), ("reserved", "<u4", 2)])
RECOVER_RESULT = np.dtype([("position", "<f4", 3), ("flags", "<u4"), ("push", "<f4", 3), ("iterations", "<u4"), ("last", PENETRATION_HIT)])
NH_RECOVER_MAX_ITERATIONS = 8
NH_RECOVER_PUSHED, NH_RECOVER_OVERLAPPING, NH_RECOVER_TOUCHING, NH_RECOVER_INVALID = 1, 2, 4, 0x80000000
NH_OVERLAP_OVERFLOW = 0xFFFFFFFF          # offsets[count] when the total is 2^32 - 1 or more
# nh_region (include/nudge_hip.h): up to NH_REGION_MAX_PLANES half-spaces (nx, ny, nz, d), inside where n.x + d >= 0
NH_REGION_MAX_PLANES = 8
NH_EVENTS_BY_BODY = 1                     # nh_overlap_events: a record's identity is its body (both inputs are nh_overlap_bodies' outputs)


class HitList(C.Structure):
    """nh_HitList: a host struct of device pointers."""
    _fields_ = [("offsets", C.c_void_p), ("hits", C.c_void_p), ("capacity", C.c_uint32), ("reserved", C.c_uint32)]
# contact events (include/nudge_hip.h): one record per touching body pair
CONTACT_PAIR = np.dtype([("lo", "<u4"), ("hi", "<u4"), ("first", "<u4"), ("count", "<u4"), ("impulse", "<f4", 3), ("normal_impulse", "<f4"),
                         ("position", "<f4", 3), ("penetration", "<f4"), ("normal", "<f4", 3), ("deepest", "<u4")])


class ContactPair(C.Structure):
    _fields_ = [("lo", C.c_uint32), ("hi", C.c_uint32), ("first", C.c_uint32), ("count", C.c_uint32), ("impulse", C.c_float * 3), ("normal_impulse", C.c_float),
                ("position", C.c_float * 3), ("penetration", C.c_float), ("normal", C.c_float * 3), ("deepest", C.c_uint32)]


class ContactList(C.Structure):
    """nh_ContactList: a host struct of device pointers."""
    _fields_ = [("data", C.c_void_p), ("bodies", C.c_void_p), ("impulses", C.c_void_p), ("count", C.c_void_p), ("capacity", C.c_uint32), ("body_count", C.c_uint32)]


class PairList(C.Structure):
    """nh_PairList: a host struct of device pointers."""
    _fields_ = [("count", C.c_void_p), ("pairs", C.c_void_p), ("capacity", C.c_uint32), ("reserved", C.c_uint32)]
# body impulses (include/nudge_hip.h): impulse records in, one sum per body out or the bodies' momentum changed
BODY_IMPULSE = np.dtype([("point", "<f4", 3), ("body", "<u4"), ("impulse", "<f4", 3), ("flags", "<u4")])
IMPULSE_SUM = np.dtype([("body", "<u4"), ("count", "<u4"), ("linear", "<f4", 3), ("angular", "<f4", 3)])
BLAST = np.dtype([("centre", "<f4", 3), ("radius", "<f4"), ("strength", "<f4"), ("falloff", "<f4"), ("reserved", "<u4", 2)])
PUSH = np.dtype([("mass_over_dt", "<f4"), ("max_impulse", "<f4"), ("phases", "<u4"), ("flags", "<u4")])
NH_IMPULSE_AT_CENTRE = 1                  # record flag: `point` is not read, the record has no angular part
NH_IMPULSE_NO_BODY = 0xFFFFFFFF           # a record that applies to nobody
NH_IMPULSE_WAKE = 1                       # call flag of nh_body_impulses: idle_counters[body] = 0 as well


class BodyImpulse(C.Structure):
    _fields_ = [("point", C.c_float * 3), ("body", C.c_uint32), ("impulse", C.c_float * 3), ("flags", C.c_uint32)]


class ImpulseList(C.Structure):
    """nh_ImpulseList: a host struct of device pointers."""
    _fields_ = [("records", C.c_void_p), ("count", C.c_void_p), ("capacity", C.c_uint32), ("reserved", C.c_uint32)]


class ImpulseSum(C.Structure):
    _fields_ = [("body", C.c_uint32), ("count", C.c_uint32), ("linear", C.c_float * 3), ("angular", C.c_float * 3)]


class ImpulseSumList(C.Structure):
    """nh_ImpulseSumList: a host struct of device pointers."""
    _fields_ = [("count", C.c_void_p), ("sums", C.c_void_p), ("capacity", C.c_uint32), ("reserved", C.c_uint32)]


# fast bodies (include/nudge_hip.h, "fast bodies"): the colliders that travel far, swept along their velocity
SWEEP_CHANNELS = ("colliders", "casts", "hits")


class SweepParams(C.Structure):
    _fields_ = [("time_step", C.c_float), ("min_travel", C.c_float), ("core", C.c_float), ("reserved", C.c_uint32)]


class SweepList(C.Structure):
    """nh_SweepList: a host struct of device pointers."""
    _fields_ = [("counts", C.c_void_p), ("colliders", C.c_void_p), ("casts", C.c_void_p), ("hits", C.c_void_p), ("capacity", C.c_uint32), ("reserved", C.c_uint32)]


# joints (include/nudge_hip.h, "joints"): ball, distance and hinge joints between the calls of the step
NH_JOINT_BALL, NH_JOINT_DISTANCE, NH_JOINT_HINGE = 1, 2, 3
NH_JOINT_BIN, NH_JOINT_ASSEMBLY_MAX = 256, 1024
NH_JOINT_ERR_ASSEMBLY_SIZE, NH_JOINT_ERR_SHARED_BODY, NH_JOINT_ERR_OFFSETS = 1, 2, 4
JOINT = np.dtype([("a", "<u4"), ("b", "<u4"), ("type", "<u4"), ("flags", "<u4"), ("anchor_a", "<f4", 3), ("anchor_b", "<f4", 3), ("p", "<f4", 6)])
JOINT_IMPULSE = np.dtype([("row", "<f4", 6), ("reserved", "<u4", 2)])


class Joint(C.Structure):
    _fields_ = [("a", C.c_uint32), ("b", C.c_uint32), ("type", C.c_uint32), ("flags", C.c_uint32), ("anchor_a", C.c_float * 3), ("anchor_b", C.c_float * 3),
                ("p", C.c_float * 6)]


class JointImpulse(C.Structure):
    _fields_ = [("row", C.c_float * 6), ("reserved", C.c_uint32 * 2)]


class JointParams(C.Structure):
    _fields_ = [("time_step", C.c_float), ("baumgarte", C.c_float), ("max_bias", C.c_float), ("warm", C.c_float)]


class JointList(C.Structure):
    """nh_JointList: a host struct of device pointers and host counts."""
    _fields_ = [("joints", C.c_void_p), ("offsets", C.c_void_p), ("count", C.c_uint32), ("assemblies", C.c_uint32)]


class JointPlan(C.Structure):
    """nh_JointPlan: a host struct of device pointers."""
    _fields_ = [("status", C.c_void_p), ("levels", C.c_void_p), ("order", C.c_void_p), ("capacity", C.c_uint32), ("reserved", C.c_uint32)]


class Blast(C.Structure):
    _fields_ = [("centre", C.c_float * 3), ("radius", C.c_float), ("strength", C.c_float), ("falloff", C.c_float), ("reserved", C.c_uint32 * 2)]


class Push(C.Structure):
    _fields_ = [("mass_over_dt", C.c_float), ("max_impulse", C.c_float), ("phases", C.c_uint32), ("flags", C.c_uint32)]
REGION = np.dtype([("planes", "<f4", (NH_REGION_MAX_PLANES, 4)), ("plane_count", "<u4"), ("ignore_body", "<u4"), ("reserved", "<u4", 2)])


def frustum_planes(m):
    """The six inside-facing planes of the clip volume -w <= x, y, z <= w of a 4 x 4 clip matrix for column vectors, clip = m @ (x, y, z, 1): the rows
    of `m` added to and subtracted from its last row (left, right, bottom, top, near, far), as a (6, 4) float32 array (nx, ny, nz, d), not normalised --
    nh_region's planes as they are."""
    m = np.asarray(m, dtype=np.float64).reshape(4, 4)
    return np.stack([m[3] + m[0], m[3] - m[0], m[3] + m[1], m[3] - m[1], m[3] + m[2], m[3] - m[2]]).astype(np.float32)


# sensors (include/nudge_hip.h, "sensors"): one shared pattern of beams, one record per sensor
BEAM = np.dtype([("direction", "<f4", 3), ("range", "<f4")])
SENSOR = np.dtype([("position", "<f4", 3), ("body", "<u4"), ("rotation", "<f4", 4), ("ignore_body", "<u4"), ("reserved", "<u4", 3)])
SENSE_CHANNELS = ("t", "body", "tag", "hits")


class SenseOut(C.Structure):
    """nh_SenseOut: a host struct of device pointers."""
    _fields_ = [("t", C.c_void_p), ("body", C.c_void_p), ("tag", C.c_void_p), ("hits", C.c_void_p)]


def pinhole_beams(width, height, fov_y, range, tile=8):
    """The beams of a pinhole camera that looks down its local -z axis with +y up (the frustum of a perspective matrix): (beams, back).  Pixel (row,
    column) looks through its centre; the direction has z = -1, so that t is DEPTH along the optical axis, and a hit farther than `range` of depth is a
    miss.  The beams come in tile x tile blocks, row-major over the blocks and within one (a ragged edge keeps its smaller blocks), so that the 64 beams
    a wave holds are an 8 x 8 patch of the image and not a 64-pixel row; `back` is the permutation to row-major: image = channel[..., back].reshape(height,
    width).  tile = 1 is the row-major pattern (`back` the identity).  A table made in float64 and rounded once: no bits are promised."""
    width, height, tile = int(width), int(height), max(int(tile), 1)
    rows, cols = np.mgrid[0:height, 0:width]
    order = np.lexsort((cols.ravel() % tile, rows.ravel() % tile, cols.ravel() // tile, rows.ravel() // tile))          # (last key first)
    ty = np.tan(0.5 * float(fov_y))
    tx = ty * width / height
    beams = np.zeros(width * height, dtype=BEAM)
    beams["direction"][:, 0] = ((cols.ravel()[order] + 0.5) / width * 2.0 - 1.0) * tx
    beams["direction"][:, 1] = (1.0 - (rows.ravel()[order] + 0.5) / height * 2.0) * ty
    beams["direction"][:, 2] = -1.0
    beams["range"] = range
    back = np.empty(width * height, dtype=np.int64)
    back[order] = np.arange(width * height)
    return beams, back


def lidar_beams(azimuths, elevations, range):
    """The beams of a spinning lidar whose axis is its local +y: one unit direction per (elevation, azimuth), angles in radians, azimuth from local -z
    towards +x, ordered elevation-major -- a wave's 64 beams are neighbours in azimuth on one ring.  t is then the range along the beam in world
    units.  (len(elevations) * len(azimuths)) records of BEAM; index = e * len(azimuths) + a."""
    az, el = np.asarray(azimuths, dtype=np.float64).reshape(-1), np.asarray(elevations, dtype=np.float64).reshape(-1)
    e, a = np.meshgrid(el, az, indexing="ij")
    beams = np.zeros(e.size, dtype=BEAM)
    beams["direction"] = np.stack([np.cos(e) * np.sin(a), np.sin(e), -np.cos(e) * np.cos(a)], axis=-1).reshape(-1, 3)
    beams["range"] = range
    return beams


class OverlapQuery(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("shape", C.c_uint32), ("rotation", C.c_float * 4), ("size", C.c_float * 3), ("ignore_body", C.c_uint32)]


class OverlapHit(C.Structure):
    _fields_ = [("body", C.c_uint32), ("collider", C.c_uint32), ("shape", C.c_uint32), ("tag", C.c_uint32)]


class PenetrationHit(C.Structure):
    _fields_ = [("normal", C.c_float * 3), ("depth", C.c_float), ("body", C.c_uint32), ("collider", C.c_uint32), ("shape", C.c_uint32), ("tag", C.c_uint32)]


class Recover(C.Structure):
    _fields_ = OverlapQuery._fields_ + [("skin", C.c_float), ("max_iterations", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class RecoverResult(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("flags", C.c_uint32), ("push", C.c_float * 3), ("iterations", C.c_uint32), ("last", PenetrationHit)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ms", C.c_double), ("launches", C.c_uint32), ("reserved", C.c_uint32)]


def build(force=False):
    """Compile libnudge_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j4"]
    if force:
        subprocess.check_call(cmd + ["clean"])
    subprocess.check_call(cmd)
    return _LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(f"{_LIB_PATH} is missing: run `make -C nudge_amd/csrc` (there is no CPU fallback)")
        L = C.CDLL(_LIB_PATH)
        L.nh_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_uint32]
        L.nh_destroy.argtypes = [C.c_void_p]
        L.nh_destroy.restype = None
        L.nh_set_flags.argtypes = [C.c_void_p, C.c_uint32]
        L.nh_set_tag_bits.argtypes = [C.c_void_p, C.c_uint32]
        L.nh_set_pair_capacity.argtypes = [C.c_void_p, C.c_uint32]
        L.nh_bodies_changed.argtypes = [C.c_void_p]
        L.nh_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.nh_step.argtypes = [C.c_void_p, C.POINTER(StepArgs), C.c_uint32]
        L.nh_synchronize.argtypes = [C.c_void_p]
        L.nh_read_counts.argtypes = [C.c_void_p, C.POINTER(Counts)]
        L.nh_export_views.argtypes = [C.c_void_p, C.c_uint32]
        L.nh_stream_state.argtypes = [C.c_void_p, C.POINTER(BodyData), C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
        L.nh_stream_latest.argtypes = [C.c_void_p, C.POINTER(StreamInfo)]
        L.nh_set_cache_count.argtypes = [C.c_void_p, C.c_uint32]
        L.nh_error_string.argtypes = [C.c_int]
        L.nh_error_string.restype = C.c_char_p
        L.nh_last_hip_error.argtypes = [C.c_void_p]
        L.nh_collide.argtypes = [C.c_void_p, C.POINTER(ActiveBodies), C.POINTER(ContactData), C.POINTER(BodyData),
                                 C.POINTER(ColliderData), C.POINTER(BodyConnections), Arena]
        L.nh_apply_gravity_damping.argtypes = [C.c_void_p, C.POINTER(ActiveBodies), C.POINTER(BodyData), C.c_float,
                                               C.POINTER(C.c_float), C.c_float]
        L.nh_read_cached_impulses.argtypes = [C.c_void_p, C.POINTER(ContactCache), C.POINTER(ContactData), C.POINTER(Arena), C.POINTER(C.c_void_p)]
        L.nh_write_cached_impulses.argtypes = [C.c_void_p, C.POINTER(ContactCache), C.POINTER(ContactData), C.c_void_p]
        L.nh_setup_contact_constraints.argtypes = [C.c_void_p, C.POINTER(ActiveBodies), C.POINTER(ContactData), C.POINTER(BodyData),
                                                   C.c_void_p, C.POINTER(Arena), C.POINTER(C.c_void_p)]
        L.nh_apply_impulses.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BodyData), C.c_uint32]
        L.nh_update_cached_impulses.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.nh_advance.argtypes = [C.c_void_p, C.POINTER(ActiveBodies), C.POINTER(BodyData), C.c_float]
        L.nh_contact_impulses_device.argtypes = [C.c_void_p]
        L.nh_contact_impulses_device.restype = C.c_void_p
        L.nh_enable_timing.argtypes = [C.c_void_p, C.c_int]
        L.nh_set_timing_filter.argtypes = [C.c_void_p, C.c_char_p]
        L.nh_kernel_times.argtypes = [C.c_void_p, C.POINTER(KernelTime), C.c_int, C.c_int]
        L.nh_halo_pack.argtypes = [C.c_void_p, C.POINTER(BodyData), C.c_void_p, C.c_uint32, C.c_void_p]
        L.nh_halo_unpack.argtypes = [C.c_void_p, C.POINTER(BodyData), C.c_uint32, C.c_uint32, C.c_void_p]
        L.nh_halo_update.argtypes = [C.c_void_p, C.POINTER(BodyData), C.c_uint32, C.c_uint32, C.c_void_p]
        L.nh_append_contacts.argtypes = [C.c_void_p, C.POINTER(ContactData), C.POINTER(BodyData), C.c_uint32, C.c_void_p, Arena]
        # multi-GPU: one x-slab per context (include/nudge_hip.h, "multi-GPU")
        L.nh_partition_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(PartitionConfig), C.POINTER(BodyData), C.POINTER(ColliderData)]
        L.nh_partition_destroy.argtypes = [C.c_void_p]
        L.nh_partition_destroy.restype = None
        L.nh_partition_info.argtypes = [C.c_void_p, C.POINTER(PartitionInfo)]
        L.nh_partition_pack_migrants.argtypes = [C.c_void_p, C.POINTER(BodyData), C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32 * 2)]
        L.nh_partition_unpack_migrants.argtypes = [C.c_void_p, C.POINTER(BodyData), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.nh_partition_pack_ghosts.argtypes = [C.c_void_p, C.POINTER(BodyData), C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32 * 2)]
        L.nh_partition_unpack_ghosts.argtypes = [C.c_void_p, C.POINTER(BodyData), C.POINTER(ColliderData), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.nh_partition_top_speed.argtypes = [C.c_void_p, C.POINTER(BodyData), C.POINTER(C.c_double)]
        L.nh_partition_set_peer_speeds.argtypes = [C.c_void_p, C.c_double, C.c_double]
        L.nh_partition_refresh_is_quiet.argtypes = [C.c_void_p, C.POINTER(BodyData), C.POINTER(C.c_int)]
        L.nh_partition_pack_step.argtypes = [C.c_void_p, C.POINTER(BodyData), C.c_void_p, C.c_void_p]
        L.nh_partition_mark_ghosts.argtypes = [C.c_void_p, C.POINTER(BodyData)]
        L.nh_partition_exchange_iteration.argtypes = [C.c_void_p, C.POINTER(BodyData)]
        for _fn in (L.nh_partition_pack_deltas, L.nh_partition_unpack_deltas, L.nh_partition_pack_momentum, L.nh_partition_unpack_momentum):
            _fn.argtypes = [C.c_void_p, C.POINTER(BodyData), C.c_void_p, C.c_void_p]
        L.nh_partition_unpack_step.argtypes = [C.c_void_p, C.POINTER(BodyData), C.c_void_p, C.c_void_p]
        L.nh_partition_choose_cut.argtypes = [C.c_void_p, C.POINTER(BodyData), C.c_int, C.c_uint32, C.POINTER(C.c_double)]
        L.nh_partition_set_cut.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.nh_partition_set_transport.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.nh_partition_exchange_step.argtypes = [C.c_void_p, C.POINTER(BodyData)]
        L.nh_partition_step.argtypes = [C.c_void_p, C.POINTER(StepArgs), C.c_uint32, C.c_uint32, C.c_uint32]
        L.nh_partition_transport_check.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
        L.nh_partition_transport_result.argtypes = [C.c_void_p]
        L.nh_set_first_ghost_body.argtypes = [C.c_void_p, C.c_uint32]
        L.nh_query_build.argtypes = [C.c_void_p, C.POINTER(BodyData), C.POINTER(ColliderData)]
        # (an older build of the library, loaded through NUDGE_HIP_LIBRARY for an A/B, has no refit: World.query_refit then raises AttributeError)
        if hasattr(L, "nh_query_refit"):
            L.nh_query_refit.argtypes = [C.c_void_p, C.POINTER(BodyData), C.POINTER(ColliderData)]
            L.nh_query_stats.argtypes = [C.c_void_p, C.POINTER(QueryStats)]
        # (likewise the layer masks: World.query_set_layers / query_filter / query_layer_info then raise AttributeError)
        if hasattr(L, "nh_query_set_layers"):
            L.nh_query_set_layers.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            L.nh_query_filter.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
            L.nh_query_layer_info.argtypes = [C.c_void_p, C.POINTER(QueryLayerInfo)]
        L.nh_raycast.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.nh_spherecast.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.nh_boxcast.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.nh_capsulecast.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.nh_closest.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.nh_closest_k.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
        # (likewise the first-k casts: World.raycast_k and its siblings then raise AttributeError)
        if hasattr(L, "nh_raycast_k"):
            for fn in (L.nh_raycast_k, L.nh_spherecast_k, L.nh_boxcast_k, L.nh_capsulecast_k):
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
        # (an older build of the library, loaded through NUDGE_HIP_LIBRARY for an A/B, has no nh_distance: World.distance then raises AttributeError)
        if hasattr(L, "nh_distance"):
            L.nh_distance.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        # (likewise nh_move: World.move then raises AttributeError)
        if hasattr(L, "nh_move"):
            L.nh_move.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        # (likewise nh_recover: World.recover then raises AttributeError)
        if hasattr(L, "nh_recover"):
            L.nh_recover.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        # (likewise nh_walk: World.walk then raises AttributeError)
        if hasattr(L, "nh_walk"):
            L.nh_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        # (likewise nh_boxmove and nh_boxwalk: World.boxmove and World.boxwalk then raise AttributeError)
        if hasattr(L, "nh_boxmove"):
            L.nh_boxmove.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
            L.nh_boxwalk.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        # (likewise the movers' _touched forms: World.move_touched_records and its siblings then raise AttributeError)
        if hasattr(L, "nh_move_touched"):
            for fn in (L.nh_move_touched, L.nh_boxmove_touched, L.nh_walk_touched, L.nh_boxwalk_touched):
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
        L.nh_overlap.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.nh_penetration.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        # (an older build of the library, loaded through NUDGE_HIP_LIBRARY for an A/B, has no nh_region: World.region then raises AttributeError)
        if hasattr(L, "nh_region"):
            L.nh_region.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        # (likewise the wide forms of nh_overlap and nh_penetration: World.overlap_wide / penetration_wide then raise AttributeError)
        if hasattr(L, "nh_overlap_wide"):
            L.nh_overlap_wide.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
            L.nh_penetration_wide.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        # (an older build of the library, loaded through NUDGE_HIP_LIBRARY for an A/B, has no all-hits casts: World.raycast_all then raises AttributeError)
        if hasattr(L, "nh_raycast_all"):
            L.nh_raycast_all.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
            L.nh_spherecast_all.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        # (likewise the all-hits box and capsule casts: World.boxcast_all / capsulecast_all then raise AttributeError)
        if hasattr(L, "nh_boxcast_all"):
            L.nh_boxcast_all.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
            L.nh_capsulecast_all.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        # (likewise the trigger events: World.overlap_bodies_records / overlap_events_records then raise AttributeError)
        if hasattr(L, "nh_overlap_events"):
            L.nh_overlap_bodies.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
            L.nh_overlap_events.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        # (likewise the contact events: World.contact_pairs_records / contact_events_records / step_contact_pairs then raise AttributeError)
        if hasattr(L, "nh_contact_events"):
            L.nh_contact_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
            L.nh_contact_events.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
            L.nh_step_contact_pairs.argtypes = [C.c_void_p, C.POINTER(ContactData), C.POINTER(ContactCache), C.c_uint32, C.c_void_p, C.c_uint32]
        # (likewise the sensors: World.sense_records / sense_rays_records / sense then raise AttributeError)
        if hasattr(L, "nh_sense"):
            L.nh_sense.argtypes = [C.c_void_p, C.POINTER(BodyData), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(SenseOut), C.c_uint32]
            L.nh_sense_rays.argtypes = [C.c_void_p, C.POINTER(BodyData), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        # (likewise the body impulses: World.impulse_sums_records / body_impulses_records and the generators then raise AttributeError)
        if hasattr(L, "nh_body_impulses"):
            L.nh_impulse_sums.argtypes = [C.c_void_p, C.POINTER(BodyData), C.c_void_p, C.c_void_p, C.c_uint32]
            L.nh_body_impulses.argtypes = [C.c_void_p, C.POINTER(BodyData), C.c_void_p, C.c_uint32]
            L.nh_blast_impulses.argtypes = [C.c_void_p, C.POINTER(BodyData), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
            L.nh_touch_impulses.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        # (likewise the fast bodies: World.sweep_records / sweep_limit_records / sweep then raise AttributeError)
        if hasattr(L, "nh_sweep"):
            L.nh_sweep.argtypes = [C.c_void_p, C.POINTER(BodyData), C.POINTER(SweepParams), C.POINTER(SweepList), C.c_uint32]
            L.nh_sweep_limit.argtypes = [C.c_void_p, C.POINTER(BodyData), C.POINTER(SweepList), C.c_void_p, C.c_uint32]
        # (likewise the joints: World.joints_* then raise AttributeError)
        if hasattr(L, "nh_joints_prepare"):
            L.nh_joints_prepare.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(JointList), C.POINTER(JointPlan)]
            L.nh_joints_setup.argtypes = [C.c_void_p, C.POINTER(ActiveBodies), C.POINTER(BodyData), C.POINTER(JointList), C.POINTER(JointPlan), C.POINTER(JointParams), C.c_void_p]
            L.nh_joints_apply.argtypes = [C.c_void_p, C.POINTER(BodyData), C.POINTER(JointList), C.POINTER(JointPlan), C.c_void_p, C.c_uint32]
            L.nh_joint_connections.argtypes = [C.c_void_p, C.POINTER(JointList), C.c_void_p]
        _LIB = L
    return _LIB


class NudgeError(RuntimeError):
    pass


class StreamInfo(C.Structure):
    _fields_ = [("slot", C.c_uint32), ("valid", C.c_uint32), ("step", C.c_uint64), ("frames", C.c_uint64), ("dropped", C.c_uint64)]


def _check(L, rc, what):
    if rc != 0:
        raise NudgeError(f"{what}: {L.nh_error_string(rc).decode()} ({rc})")


class World:
    """A world resident in HBM, stepped through the C ABI.  `scene` uses the layouts of nudge_amd.scenes."""

    def __init__(self, scene, device=0, max_contacts=None, arena_bytes=None, flags=NH_FLAG_SYNC_COUNTS, tag_bits=None, capacity=None, max_pairs=None):
        """`capacity` = dict(bodies=, boxes=, spheres=): allocate room for more records than the scene holds (the
        partitioned world appends ghost / migrated bodies: nh_partition_unpack_ghosts behind partition.HipPartition, which sets the counts itself;
        partition.TorchPartition rewrites the arrays and calls set_counts()).
        `max_pairs`: capacity of the broadphase pair buffer (nh_set_pair_capacity); default max_contacts / 2 + 1024."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("nudge_amd.World needs a HIP device (no CPU fallback)")
        self.torch = torch
        self.L = lib()
        self.dev = torch.device("cuda", device)
        torch.cuda.set_device(self.dev)
        self.params = dict(scene["params"])
        nb = len(scene["body_transforms"])
        nbox, nsph = len(scene["box_tags"]), len(scene["sphere_tags"])
        if max_contacts is None:
            max_contacts = max(4096, 8 * nb)
        self.nb, self.nbox, self.nsph, self.max_contacts = nb, nbox, nsph, max_contacts
        capacity = capacity or {}
        cap_b, cap_x, cap_s = max(nb, capacity.get("bodies", 0)), max(nbox, capacity.get("boxes", 0)), max(nsph, capacity.get("spheres", 0))
        self.capacity = dict(bodies=cap_b, boxes=cap_x, spheres=cap_s)
        self._keep = {}

        def up(name, arr, min_bytes=16, cap=0):
            a = np.ascontiguousarray(arr)
            raw = a.view(np.uint8).reshape(-1)
            t = torch.zeros(max(raw.size, min_bytes, cap * a.dtype.itemsize), dtype=torch.uint8, device=self.dev)
            if raw.size:
                t[:raw.size] = torch.from_numpy(raw.copy()).to(self.dev)
            self._keep[name] = t
            return t

        def alloc(name, nbytes):
            t = torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device=self.dev)
            self._keep[name] = t
            return t

        self.bodies = BodyData(up("bt", scene["body_transforms"], cap=cap_b).data_ptr(), up("bp", scene["body_properties"], cap=cap_b).data_ptr(),
                               up("bm", scene["body_momentum"], cap=cap_b).data_ptr(), up("bi", scene["idle_counters"], cap=cap_b).data_ptr(), nb)
        self.colliders = ColliderData(
            _Shapes(up("xt", scene["box_tags"].astype(np.uint32), cap=cap_x).data_ptr(), up("xd", scene["box_data"], cap=cap_x).data_ptr(),
                    up("xx", scene["box_transforms"], cap=cap_x).data_ptr(), nbox),
            _Shapes(up("st", scene["sphere_tags"].astype(np.uint32), cap=cap_s).data_ptr(), up("sd", scene["sphere_data"], cap=cap_s).data_ptr(),
                    up("sx", scene["sphere_transforms"], cap=cap_s).data_ptr(), nsph))
        con = np.asarray(scene.get("connections", np.zeros((0, 2), np.uint32)), dtype=np.uint32).reshape(-1, 2)
        self.connections = BodyConnections(up("cn", con).data_ptr(), len(con))
        K = max_contacts
        self.contacts = ContactData(alloc("cd", 32 * K).data_ptr(), alloc("cb", 8 * K).data_ptr(), alloc("ct", 8 * K).data_ptr(),
                                    alloc("cf", 4 * K).data_ptr(), K, 0, alloc("cs", 8 * K).data_ptr(), 0)
        self.cache = ContactCache(alloc("kt", 8 * K).data_ptr(), alloc("kf", 4 * K).data_ptr(), alloc("kd", 16 * K).data_ptr(), K, 0)
        self.active = ActiveBodies(alloc("ai", 4 * cap_b).data_ptr(), cap_b, 0)
        if arena_bytes is None:
            ncol = cap_x + cap_s
            nb = cap_b
            cells = 1
            while cells < 4 * ncol:
                cells <<= 1
            cells = min(max(cells, 1 << 16), 1 << 24)
            pairs = max_pairs if max_pairs else K // 2 + 1024
            arena_bytes = (64 << 20) + ncol * 200 + cells * 8 + K * 320 + pairs * 216 + nb * 64
        self.arena_t = alloc("arena", arena_bytes)
        self.arena = Arena(self.arena_t.data_ptr(), arena_bytes)

        self.ctx = C.c_void_p()
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        _check(self.L, self.L.nh_create(C.byref(self.ctx), device, C.c_void_p(stream), flags), "nh_create")
        self.flags = flags
        # A/B switches for tests and dev scripts: environment variables NH_<NAME>=<int> become nh_set_option(name, value) calls HERE -- the library itself never
        # reads the environment (include/nudge_hip.h: nh_set_option)
        for key, val in sorted(os.environ.items()):
            if not key.startswith("NH_"):
                continue
            name = key[3:].lower()
            if name not in OPTION_NAMES:           # (a stale or unrelated NH_* variable must not keep a world from being created)
                warnings.warn(f"nudge_amd: environment variable {key} names no library option; ignored")
                continue
            try:
                num = int(val)
            except ValueError:
                num = 1
            rc = self.L.nh_set_option(self.ctx, name.encode(), num)
            if rc:
                warnings.warn(f"nudge_amd: nh_set_option({name}, {num}) refused: {self.L.nh_error_string(rc).decode()}")
        if tag_bits is None:
            mt = 1
            for k in ("box_tags", "sphere_tags"):
                if len(scene[k]):
                    mt = max(mt, int(scene[k].max()))
            tag_bits = max(8, int(mt).bit_length())
        self.L.nh_set_tag_bits(self.ctx, tag_bits)
        if max_pairs:
            _check(self.L, self.L.nh_set_pair_capacity(self.ctx, int(max_pairs)), "nh_set_pair_capacity")
        self.steps_done = 0
        self.sum_contacts = 0
        self._imp = C.c_void_p()
        self._con = C.c_void_p()

    def close(self):
        if getattr(self, "ctx", None):
            self.L.nh_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the reference's step loop (example/main.cpp:274-328), one C-ABI call per reference call ----
    def collide(self):
        _check(self.L, self.L.nh_collide(self.ctx, C.byref(self.active), C.byref(self.contacts), C.byref(self.bodies),
                                         C.byref(self.colliders), C.byref(self.connections), self.arena), "nh_collide")
        self._temp = Arena(self.arena.data, self.arena.size)

    def append_contacts(self, data, bodies, tags, features, count=None):
        """Custom contacts behind the list collide() returned (reference example/main.cpp:287): numpy arrays of S.CONTACT records, (n, 2) uint32
        body pairs, uint64 tags (a_tag | b_tag << 32) and uint32 features; `count` = contacts so far (read from the device when not given)."""
        torch = self.torch
        n = len(tags)
        if n == 0:
            return
        k = self.counts()["contacts"] if count is None else count
        if k + n > self.max_contacts:
            raise NudgeError("append_contacts: contact capacity")
        for name, arr, width in (("cd", np.ascontiguousarray(data), 32), ("cb", np.ascontiguousarray(bodies, dtype=np.uint32), 8),
                                 ("ct", np.ascontiguousarray(tags, dtype=np.uint64), 8), ("cf", np.ascontiguousarray(features, dtype=np.uint32), 4)):
            raw = arr.view(np.uint8).reshape(-1)
            assert raw.size == width * n, name
            self._keep[name][width * k:width * (k + n)] = torch.from_numpy(raw.copy()).to(self.dev)
        _check(self.L, self.L.nh_append_contacts(self.ctx, C.byref(self.contacts), C.byref(self.bodies), n, None, self.arena), "append_contacts")

    def gravity(self):
        p = self.params
        g = (C.c_float * 3)(0.0, p["gravity"], 0.0)
        _check(self.L, self.L.nh_apply_gravity_damping(self.ctx, C.byref(self.active), C.byref(self.bodies), p["time_step"], g, p["damping_rate"]), "gravity")

    def read_cache(self):
        _check(self.L, self.L.nh_read_cached_impulses(self.ctx, C.byref(self.cache), C.byref(self.contacts), C.byref(self._temp), C.byref(self._imp)), "read_cached_impulses")

    def setup(self):
        _check(self.L, self.L.nh_setup_contact_constraints(self.ctx, C.byref(self.active), C.byref(self.contacts), C.byref(self.bodies),
                                                           self._imp, C.byref(self._temp), C.byref(self._con)), "setup_contact_constraints")

    def apply(self, iterations=None):
        it = self.params["iterations"] if iterations is None else iterations
        _check(self.L, self.L.nh_apply_impulses(self.ctx, self._con, C.byref(self.bodies), it), "apply_impulses")

    def update(self):
        _check(self.L, self.L.nh_update_cached_impulses(self.ctx, self._con, self._imp), "update_cached_impulses")

    def write_cache(self):
        _check(self.L, self.L.nh_write_cached_impulses(self.ctx, C.byref(self.cache), C.byref(self.contacts), self._imp), "write_cached_impulses")

    def advance(self, time_step=None):
        dt = self.params["time_step"] if time_step is None else time_step
        _check(self.L, self.L.nh_advance(self.ctx, C.byref(self.active), C.byref(self.bodies), dt), "advance")

    def step(self, steps=1, iterations=None):
        """`steps` sub-steps of the sample's loop (example/main.cpp:274-328).  Worlds that do not ask for host-visible counts go through nh_step -- the eight calls made
        by the library itself, one crossing of the ABI for all the steps; the others (NH_FLAG_SYNC_COUNTS: `sum_contacts` is kept per step) make the eight calls here."""
        if steps > 0 and not (self.flags & NH_FLAG_SYNC_COUNTS) and not getattr(self, "eight_calls", False):
            p = self.params
            it = p["iterations"] if iterations is None else iterations
            # (rebuilt every call -- a dozen host-side stores -- so that a changed time step, gravity or damping is never ignored; the structs it points to are this
            # object's own: counts changed by set_counts are seen through the pointers)
            args = self._step_args = StepArgs(C.pointer(self.active), C.pointer(self.contacts), C.pointer(self.bodies), C.pointer(self.colliders), C.pointer(self.connections),
                                              C.pointer(self.cache), self.arena, p["time_step"], (C.c_float * 3)(0.0, p["gravity"], 0.0), p["damping_rate"], it)
            _check(self.L, self.L.nh_step(self.ctx, C.byref(args), steps), "nh_step")
            self.steps_done += steps
            return
        for _ in range(steps):
            self.collide()
            self.gravity()
            self.read_cache()
            self.setup()
            self.apply(iterations)
            self.update()
            self.write_cache()
            self.advance()
            self.step_done()

    def partition_step(self, partition, steps, exchange_first, loopback_records=0, iterations=None):
        """`steps` sub-steps of a partitioned world in ONE library call (nh_partition_step): the per-step halo exchange is enqueued by the library between two sub-steps
        over the transport of nh_partition_set_transport; the chain of still steps runs through the call."""
        p = self.params
        it = p["iterations"] if iterations is None else iterations
        args = self._step_args = StepArgs(C.pointer(self.active), C.pointer(self.contacts), C.pointer(self.bodies), C.pointer(self.colliders), C.pointer(self.connections),
                                          C.pointer(self.cache), self.arena, p["time_step"], (C.c_float * 3)(0.0, p["gravity"], 0.0), p["damping_rate"], it)
        _check(self.L, self.L.nh_partition_step(partition, C.byref(args), steps, 1 if exchange_first else 0, loopback_records), "nh_partition_step")
        self.steps_done += steps

    def step_done(self):
        """Book-keeping of one finished step; callers that drive the eight calls themselves (partition.py, per-iteration exchange) call it after advance()."""
        self.steps_done += 1
        if self.flags & NH_FLAG_SYNC_COUNTS:
            self.sum_contacts += self.contacts.count

    # ---- checkpoint / restore of the caller-owned persistent state (bodies + contact cache), device to device ----
    def snapshot(self):
        """Everything that persists from one step to the next on the caller's side (nudge.h: BodyData transforms / momentum / idle
        counters and the ContactCache), cloned on the device."""
        self.export_views(NH_VIEW_CACHE)
        c = self.counts()
        return dict(cache_count=c["cache"], arrays={k: self._keep[k].clone() for k in ("bt", "bm", "bi", "kt", "kf", "kd")})

    def restore(self, snap):
        self.synchronize()
        for k, t in snap["arrays"].items():
            self._keep[k].copy_(t)
        self.L.nh_bodies_changed(self.ctx)
        _check(self.L, self.L.nh_set_cache_count(self.ctx, snap["cache_count"]), "set_cache_count")

    # ---- variable membership (partitioned worlds) ----
    def set_counts(self, bodies, boxes, spheres):
        c = self.capacity
        if bodies > c["bodies"] or boxes > c["boxes"] or spheres > c["spheres"]:
            raise NudgeError(f"set_counts({bodies}, {boxes}, {spheres}) exceeds the capacity {c}")
        self.nb, self.nbox, self.nsph = bodies, boxes, spheres
        self.L.nh_bodies_changed(self.ctx)            # (the caller has rewritten body records, idle counters included)
        self.bodies.count = bodies
        self.colliders.boxes.count = boxes
        self.colliders.spheres.count = spheres

    def set_first_ghost(self, first_ghost):
        """Contact ownership of a partitioned world (include/nudge_hip.h: nh_set_first_ghost_body): bodies >= first_ghost are ghosts; 0 = off."""
        _check(self.L, self.L.nh_set_first_ghost_body(self.ctx, int(first_ghost)), "nh_set_first_ghost_body")

    def records(self, name, record_bytes):
        """Device tensor behind one caller-owned array, as [capacity, record_bytes] uint8 (no copy)."""
        t = self._keep[name]
        n = t.numel() // record_bytes
        return t[:n * record_bytes].view(n, record_bytes)

    # ---- halo records of the partitioned world (include/nudge_hip.h: nh_halo_pack / nh_halo_unpack) ----
    def halo_pack(self, indices_i32):
        """indices_i32: int32 device tensor of body slots -> uint8 device tensor [len, 64] of their per-step records."""
        n = int(indices_i32.numel())
        out = self.torch.empty((n, HALO_RECORD_BYTES), dtype=self.torch.uint8, device=self.dev)
        _check(self.L, self.L.nh_halo_pack(self.ctx, C.byref(self.bodies), C.c_void_p(indices_i32.data_ptr() if n else 0), n,
                                           C.c_void_p(out.data_ptr() if n else 0)), "halo_pack")
        return out

    def halo_unpack(self, first_slot, records, same_bodies=False):
        """same_bodies: the records update the bodies already in those slots (per-step halo: nh_halo_update keeps the sleep prediction)."""
        n = int(records.shape[0])
        if n:
            assert records.is_contiguous() and records.shape[1] == HALO_RECORD_BYTES
            fn = self.L.nh_halo_update if same_bodies else self.L.nh_halo_unpack
            _check(self.L, fn(self.ctx, C.byref(self.bodies), first_slot, n, C.c_void_p(records.data_ptr())), "halo_unpack")

    # ---- state ----
    def synchronize(self):
        _check(self.L, self.L.nh_synchronize(self.ctx), "synchronize")

    def export_views(self, what=NH_VIEW_ALL):
        """The dense contact list / the contact cache in the caller's arrays brought up to date after still steps (include/nudge_hip.h note 9)."""
        _check(self.L, self.L.nh_export_views(self.ctx, what), "export_views")

    def counts(self):
        c = Counts()
        _check(self.L, self.L.nh_read_counts(self.ctx, C.byref(c)), "read_counts")
        return c.as_dict()

    def _down(self, name, dtype, count):
        t = self._keep[name]
        nbytes = np.dtype(dtype).itemsize * count
        return np.frombuffer(t[:nbytes].cpu().numpy().tobytes(), dtype=dtype, count=count).copy()

    def get_bodies(self):
        self.synchronize()
        return dict(transforms=self._down("bt", S.TRANSFORM, self.nb), momentum=self._down("bm", S.MOMENTUM, self.nb),
                    idle=self._down("bi", np.uint8, self.nb))

    def set_option(self, name, value=1):
        """nh_set_option on the live world (tests, A/B): include/nudge_hip.h lists the names."""
        _check(self.L, self.L.nh_set_option(self.ctx, name.encode(), int(value)), f"nh_set_option({name})")

    def set_bodies(self, transforms=None, momentum=None, idle=None):
        torch = self.torch
        for name, arr in (("bt", transforms), ("bm", momentum), ("bi", idle)):
            if arr is not None:
                raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
                self._keep[name][:raw.size] = torch.from_numpy(raw.copy()).to(self.dev)
        if idle is not None:
            self.L.nh_bodies_changed(self.ctx)

    def get_contacts(self):
        self.export_views(NH_VIEW_CONTACTS)
        c = self.counts()
        n, ns = c["contacts"], c["sleeping_pairs"]
        return dict(count=n, data=self._down("cd", S.CONTACT, n), bodies=self._down("cb", np.uint32, 2 * n).reshape(-1, 2),
                    tags=self._down("ct", np.uint64, n), features=self._down("cf", np.uint32, n),
                    sleeping_pairs=self._down("cs", np.uint64, ns))

    def get_active(self):
        self.export_views(NH_VIEW_ACTIVE)
        c = self.counts()
        return self._down("ai", np.uint32, c["active_bodies"])

    def get_cache(self):
        self.export_views(NH_VIEW_CACHE)
        c = self.counts()
        n = c["cache"]
        return dict(count=n, tags=self._down("kt", np.uint64, n), features=self._down("kf", np.uint32, n), data=self._down("kd", S.IMPULSE, n))

    def get_contact_impulses(self):
        if not self._imp:
            raise NudgeError("get_contact_impulses: no nh_ContactImpulseData handle -- step() went through nh_step, which keeps the handles inside the library; "
                             "set world.eight_calls = True (or call the eight entry points) to look at the per-contact impulses of a step")
        c = self.counts()
        n = c["contacts"]
        ptr = self.L.nh_contact_impulses_device(self._imp)
        off = ptr - self.arena_t.data_ptr()
        raw = self.arena_t[off:off + 16 * n].cpu().numpy().tobytes()
        return np.frombuffer(raw, dtype=S.IMPULSE, count=n).copy()

    # ---- state streaming (include/nudge_hip.h: nh_stream_state): body transforms into a pinned host ring every `every` steps, without stopping the world ----
    def stream_state(self, every, slots=4, count=None):
        torch = self.torch
        n = self.nb if count is None else count
        if every:
            self._stream_ring = torch.zeros((slots, n * 32), dtype=torch.uint8).pin_memory()
            self._stream_count = n
            _check(self.L, self.L.nh_stream_state(self.ctx, C.byref(self.bodies), n, C.c_void_p(self._stream_ring.data_ptr()), slots, every), "nh_stream_state")
        else:
            _check(self.L, self.L.nh_stream_state(self.ctx, None, 0, None, 0, 0), "nh_stream_state")

    def stream_latest(self):
        """(step, transforms) of the newest frame that has landed in the ring, or None; plus the stream's counters."""
        info = StreamInfo()
        _check(self.L, self.L.nh_stream_latest(self.ctx, C.byref(info)), "nh_stream_latest")
        stats = dict(frames=int(info.frames), dropped=int(info.dropped))
        if not info.valid:
            return None, stats
        raw = self._stream_ring[info.slot].numpy().tobytes()
        return (int(info.step), np.frombuffer(raw, dtype=S.TRANSFORM, count=self._stream_count).copy()), stats

    # ---- scene queries (include/nudge_hip.h, "scene queries"): observers of the world, they change nothing about stepping ----
    def query_build(self):
        """Build the ray-cast hierarchy over every collider from the current transforms (nh_query_build; enqueued, no synchronisation)."""
        _check(self.L, self.L.nh_query_build(self.ctx, C.byref(self.bodies), C.byref(self.colliders)), "nh_query_build")

    def query_refit(self):
        """Make the hierarchy of the last query_build() current: the same tree, every record and box from the current transforms (nh_query_refit;
        enqueued, no synchronisation).  Every query then answers exactly as after a query_build() now; only its speed may differ."""
        _check(self.L, self.L.nh_query_refit(self.ctx, C.byref(self.bodies), C.byref(self.colliders)), "nh_query_refit")

    def query_stats(self):
        """Diagnostics of the last query_build()'s tree (nh_query_stats; waits for the stream): colliders, run_length, runs, top_nodes, top_depth."""
        st = QueryStats()
        _check(self.L, self.L.nh_query_stats(self.ctx, C.byref(st)), "nh_query_stats")
        return {k: int(getattr(st, k)) for k, _ in QueryStats._fields_}

    def _layer_words(self, name, words, count):
        """`words` (None, numpy or torch, `count` values below 2^32) as an int32 device tensor of their bits, or None."""
        torch = self.torch
        if words is None:
            return None
        if not torch.is_tensor(words):
            words = torch.from_numpy(np.ascontiguousarray(words).astype(np.int64))
        t = words.to(device=self.dev).reshape(-1)
        if t.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
            t = (((t.to(torch.int64) & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000).to(torch.int32)
        t = t.contiguous()
        if t.numel() != count:
            raise ValueError(f"{name}: {t.numel()} words for {count}")
        return t

    def query_set_layers(self, box_layers=None, sphere_layers=None):
        """Give every collider of the last query_build() its word of layer bits (nh_query_set_layers; enqueued): `box_layers` / `sphere_layers` are
        numpy arrays or torch tensors of nbox / nsph values below 2^32, None for all ones; both None forgets the layers.  A query with mask m (see
        query_filter) sees collider c iff layers[c] & m != 0.  The words are copied: the arguments are not kept."""
        b = self._layer_words("query_set_layers: box_layers", box_layers, self.colliders.boxes.count)
        s = self._layer_words("query_set_layers: sphere_layers", sphere_layers, self.colliders.spheres.count)
        # (a shape without colliders has no words to give: its NULL must not read as "forget" while the other shape has some)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None      # noqa: E731
        pb, ps = ptr(b), ptr(s)
        if (b is not None or s is not None) and pb is None and ps is None:
            return
        _check(self.L, self.L.nh_query_set_layers(self.ctx, pb, ps), "nh_query_set_layers")
        # (the copy is enqueued on the library's stream; torch frees on its own: keep the sources until the next call)
        self._layer_sources = (b, s)

    def query_filter(self, mask=None):
        """The filter every later query call reads (nh_query_filter): None -- off; an int -- every query uses that mask; a uint32 / int32 device
        tensor -- query i of each later call uses mask[i] (it must hold as many words as the call has queries; the World keeps a reference, the
        library the pointer, and the words are read when a query runs)."""
        torch = self.torch
        if mask is None:
            rc = self.L.nh_query_filter(self.ctx, NH_FILTER_OFF, 0, None)
            keep = None
        elif torch.is_tensor(mask):
            if mask.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not mask.is_contiguous() or mask.device != torch.device(self.dev):
                raise ValueError("query_filter: per-query masks must be a contiguous uint32 / int32 tensor on the world's device")
            rc = self.L.nh_query_filter(self.ctx, NH_FILTER_PER_QUERY, 0, C.c_void_p(mask.data_ptr()))
            keep = mask
        else:
            rc = self.L.nh_query_filter(self.ctx, NH_FILTER_UNIFORM, int(mask) & 0xFFFFFFFF, None)
            keep = None
        _check(self.L, rc, "nh_query_filter")
        self._filter_masks = keep

    def query_layer_info(self):
        """Whether layers are in force and the OR of every collider's word (nh_query_layer_info; waits for the stream): set, colliders, any_layers."""
        st = QueryLayerInfo()
        _check(self.L, self.L.nh_query_layer_info(self.ctx, C.byref(st)), "nh_query_layer_info")
        return {k: int(getattr(st, k)) for k, _ in QueryLayerInfo._fields_ if k != "reserved"}

    def _ignore_bits(self, ignore_body):
        """`ignore_body` (None, a body index, or n of them) as the uint32 bits in an int32 tensor."""
        torch = self.torch
        ign = 0xFFFFFFFF if ignore_body is None else ignore_body
        ign = torch.as_tensor(ign, dtype=torch.int64, device=self.dev)
        return (((ign & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000).to(torch.int32)

    def _cast_head(self, name, origins, directions, max_t, ignore_body, width):
        """New cast records of `width` floats with the words every cast starts with (nh_Ray) filled in: (records, n).  Wider records start as
        zeros: the kernel reads their padding as part of 16-byte words."""
        torch = self.torch
        o = torch.as_tensor(origins, dtype=torch.float32, device=self.dev).reshape(-1, 3)
        d = torch.as_tensor(directions, dtype=torch.float32, device=self.dev).reshape(-1, 3)
        n = o.shape[0]
        if d.shape[0] != n:
            raise ValueError(f"{name}: {n} origins but {d.shape[0]} directions")
        casts = (torch.zeros if width > 8 else torch.empty)((n, width), dtype=torch.float32, device=self.dev)
        casts[:, 0:3] = o
        casts[:, 3] = torch.as_tensor(max_t, dtype=torch.float32, device=self.dev)
        casts[:, 4:7] = d
        casts.view(torch.int32)[:, 7] = self._ignore_bits(ignore_body)
        return casts, n

    def _records(self, name, in_bytes, out_bytes, records, results, flags=0):
        """The C call `name`(ctx, records, count, results, flags) of the one-result-per-record queries: `records` a contiguous device tensor of
        count x in_bytes bytes (any dtype).  Returns the count x out_bytes uint8 device tensor of its results (`results`, or a new one)."""
        n = records.numel() * records.element_size() // in_bytes
        if results is None:
            results = self.torch.empty((n, out_bytes), dtype=self.torch.uint8, device=self.dev)
        _check(self.L, getattr(self.L, name)(self.ctx, C.c_void_p(records.data_ptr() if n else 0), n, C.c_void_p(results.data_ptr() if n else 0), flags), name)
        return results

    def _ray_hits(self, raw, synchronize, **first):
        """The dict the casts return: `first`, then the fields of the nh_RayHit records `raw` and `raw` itself."""
        torch = self.torch
        f = raw.view(torch.float32).reshape(-1, 8)
        u = raw.view(torch.int32).reshape(-1, 8).to(torch.int64) & 0xFFFFFFFF
        if synchronize:
            torch.cuda.current_stream(self.dev).synchronize()
        return dict(first, t=f[:, 0], normal=f[:, 1:4], body=u[:, 4], collider=u[:, 5], shape=u[:, 6], tag=u[:, 7], raw=raw)

    def raycast_records(self, rays, any_hit=False, hits=None):
        """nh_raycast on records already laid out as nh_Ray: `rays` a contiguous device tensor of count x 32 bytes (any dtype).  Returns the
        count x 32-byte uint8 device tensor of nh_RayHit records (`hits`, or a new one)."""
        return self._records("nh_raycast", 32, 32, rays, hits, NH_RAY_ANY_HIT if any_hit else 0)

    def raycast(self, origins, directions, max_t=float("inf"), ignore_body=None, any_hit=False, synchronize=False):
        """Closest-hit (or any-hit) ray casts against the last query_build().  `origins` / `directions`: (n, 3) torch tensors or arrays (uploaded once);
        `max_t`: a number or n values; `ignore_body`: None, a body index, or n of them.  Returns a dict of device tensors: t (n), normal (n, 3), body,
        collider, shape, tag (n, int64; 0xffffffff = none) and `raw`, the nh_RayHit records.  Nothing waits for the device unless `synchronize`."""
        rays, _ = self._cast_head("raycast", origins, directions, max_t, ignore_body, 8)
        return self._ray_hits(self.raycast_records(rays, any_hit=any_hit), synchronize)

    def spherecast_records(self, casts, any_hit=False, hits=None):
        """nh_spherecast on records already laid out as nh_SphereCast: `casts` a contiguous device tensor of count x 48 bytes (any dtype).  Returns the
        count x 32-byte uint8 device tensor of nh_RayHit records (`hits`, or a new one)."""
        return self._records("nh_spherecast", 48, 32, casts, hits, NH_RAY_ANY_HIT if any_hit else 0)

    def spherecast(self, origins, directions, radii, max_t=float("inf"), ignore_body=None, any_hit=False, synchronize=False):
        """Closest-hit (or any-hit) sphere casts against the last query_build(): the ball of radius `radii` (a number or n values) swept from `origins`
        along `directions` ((n, 3) each).  `max_t`, `ignore_body` and the result are raycast()'s: t, normal (from the collider to the ball's centre; the
        contact point is origin + t * direction - radius * normal), body, collider, shape, tag and `raw`.  Nothing waits unless `synchronize`."""
        torch = self.torch
        casts, _ = self._cast_head("spherecast", origins, directions, max_t, ignore_body, 12)
        casts[:, 8] = torch.as_tensor(radii, dtype=torch.float32, device=self.dev).reshape(-1)
        return self._ray_hits(self.spherecast_records(casts, any_hit=any_hit), synchronize)

    def _list_records(self, name, in_bytes, out_bytes, records, offsets, hits, capacity):
        """The C call `name`(ctx, records, count, offsets, hits, capacity, 0) of the queries that write variable-length lists: `records` a contiguous
        device tensor of count x in_bytes bytes (any dtype), `hits` None or at least capacity x out_bytes bytes.  Returns (offsets, hits): the
        count + 1 offsets as an int32 device tensor holding the uint32 bits (`offsets`, or a new one) and `hits` as given."""
        n = records.numel() * records.element_size() // in_bytes
        if offsets is None:
            offsets = self.torch.empty(n + 1, dtype=self.torch.int32, device=self.dev)
        if hits is not None and hits.numel() * hits.element_size() < out_bytes * capacity:
            raise ValueError(f"{name[3:]}_records: hits holds {hits.numel() * hits.element_size()} bytes, capacity {capacity} needs {out_bytes * capacity}")
        _check(self.L, getattr(self.L, name)(self.ctx, C.c_void_p(records.data_ptr() if n else 0), n, C.c_void_p(offsets.data_ptr()),
                                             C.c_void_p(hits.data_ptr() if hits is not None else 0), capacity, 0), name)
        return offsets, hits

    def raycast_all_records(self, rays, offsets=None, hits=None, capacity=0):
        """nh_raycast_all on records already laid out as nh_Ray: `rays` a contiguous device tensor of count x 32 bytes (any dtype).  Returns
        (offsets, hits) as overlap_records does: the count + 1 offsets as an int32 device tensor holding the uint32 bits and `hits` as given.  With
        hits = None and capacity = 0 only the offsets are written (count only); otherwise `hits` must hold `capacity` x 32 bytes (nh_RayHit), and the
        records of ray i are written iff offsets[i + 1] <= capacity.  Enqueued; nothing waits (but a capacity larger than any before grows the scratch)."""
        return self._list_records("nh_raycast_all", 32, 32, rays, offsets, hits, capacity)

    def spherecast_all_records(self, casts, offsets=None, hits=None, capacity=0):
        """nh_spherecast_all on records already laid out as nh_SphereCast (count x 48 bytes): raycast_all_records for swept balls."""
        return self._list_records("nh_spherecast_all", 48, 32, casts, offsets, hits, capacity)

    def _castall(self, records, casts, n, capacity, synchronize):
        offsets, hits, n, capacity = self._overlap_lists(records, casts, n, capacity, 32)
        return self._ray_hits(hits, synchronize, **self._list_index(offsets, n, capacity))

    def raycast_all(self, origins, directions, max_t=float("inf"), ignore_body=None, capacity=None, synchronize=False):
        """Every collider each of n rays passes through, ordered along the ray (nh_raycast_all), against the last query_build().  The arguments are
        raycast()'s.  capacity=None: a count call, then the total is read -- this WAITS for the device -- and an exactly sized list call.  A capacity:
        one call, and nothing waits; only the segments that fit are listed (offsets[i + 1] <= capacity).
        Returns a dict of device tensors: offsets (n + 1, int64; offsets[n] = 0xffffffff when the total is 2^32 - 1 or more), `written` (0-d: the
        records listed, a prefix of whole segments), and per record slot (capacity of them; the first `written` are meaningful) query, t, normal
        ((capacity, 3)), body, collider, shape, tag (int64) and `raw`, the nh_RayHit records (capacity x 32 bytes).  Within a ray the records come
        in ascending t, ties by combined collider index; the first is raycast()'s closest hit."""
        rays, n = self._cast_head("raycast_all", origins, directions, max_t, ignore_body, 8)
        return self._castall(self.raycast_all_records, rays, n, capacity, synchronize)

    def spherecast_all(self, origins, directions, radii, max_t=float("inf"), ignore_body=None, capacity=None, synchronize=False):
        """Every collider each of n swept balls touches, ordered along the cast (nh_spherecast_all): spherecast()'s arguments, raycast_all()'s
        capacity rule and result (normal: from the collider to the ball's centre); the first record of a cast is spherecast()'s closest hit."""
        torch = self.torch
        casts, n = self._cast_head("spherecast_all", origins, directions, max_t, ignore_body, 12)
        casts[:, 8] = torch.as_tensor(radii, dtype=torch.float32, device=self.dev).reshape(-1)
        return self._castall(self.spherecast_all_records, casts, n, capacity, synchronize)

    def _box_casts(self, name, origins, directions, half_extents, rotations, max_t, ignore_body):
        """(records, n): nh_BoxCast records from boxcast()'s arguments."""
        torch = self.torch
        casts, n = self._cast_head(name, origins, directions, max_t, ignore_body, 16)
        if rotations is None:
            casts[:, 11] = 1.0
        else:
            casts[:, 8:12] = torch.as_tensor(rotations, dtype=torch.float32, device=self.dev).reshape(-1, 4)
        casts[:, 12:15] = torch.as_tensor(half_extents, dtype=torch.float32, device=self.dev).reshape(-1, 3)
        return casts, n

    def _capsule_casts(self, name, origins, directions, radii, half_heights, rotations, max_t, ignore_body):
        """(records, n): nh_CapsuleCast records from capsulecast()'s arguments."""
        torch = self.torch
        casts, n = self._cast_head(name, origins, directions, max_t, ignore_body, 16)
        if rotations is None:
            casts[:, 11] = 1.0
        else:
            casts[:, 8:12] = torch.as_tensor(rotations, dtype=torch.float32, device=self.dev).reshape(-1, 4)
        casts[:, 12] = torch.as_tensor(radii, dtype=torch.float32, device=self.dev).reshape(-1)
        casts[:, 13] = torch.as_tensor(half_heights, dtype=torch.float32, device=self.dev).reshape(-1)
        return casts, n

    def boxcast_records(self, casts, any_hit=False, hits=None):
        """nh_boxcast on records already laid out as nh_BoxCast: `casts` a contiguous device tensor of count x 64 bytes (any dtype).  Returns the
        count x 32-byte uint8 device tensor of nh_RayHit records (`hits`, or a new one)."""
        return self._records("nh_boxcast", 64, 32, casts, hits, NH_RAY_ANY_HIT if any_hit else 0)

    def boxcast(self, origins, directions, half_extents, rotations=None, max_t=float("inf"), ignore_body=None, any_hit=False, synchronize=False):
        """Closest-hit (or any-hit) box casts against the last query_build(): the oriented box of `half_extents` ((n, 3) or (3,)) and `rotations`
        ((n, 4) or (4,) quaternions (x, y, z, s); None = identity) swept, without turning, from `origins` along `directions` ((n, 3) each).  `max_t`,
        `ignore_body` and the result are raycast()'s: t, normal (from the collider to the cast box), body, collider, shape, tag and `raw`.  Nothing
        waits unless `synchronize`."""
        casts, _ = self._box_casts("boxcast", origins, directions, half_extents, rotations, max_t, ignore_body)
        return self._ray_hits(self.boxcast_records(casts, any_hit=any_hit), synchronize)

    def capsulecast_records(self, casts, any_hit=False, hits=None):
        """nh_capsulecast on records already laid out as nh_CapsuleCast: `casts` a contiguous device tensor of count x 64 bytes (any dtype).  Returns
        the count x 32-byte uint8 device tensor of nh_RayHit records (`hits`, or a new one)."""
        return self._records("nh_capsulecast", 64, 32, casts, hits, NH_RAY_ANY_HIT if any_hit else 0)

    def capsulecast(self, origins, directions, radii, half_heights, rotations=None, max_t=float("inf"), ignore_body=None, any_hit=False,
                    synchronize=False):
        """Closest-hit (or any-hit) capsule casts against the last query_build(): the capsule of `radii` and `half_heights` (numbers or n values) about
        its local y axis, turned by `rotations` ((n, 4) or (4,) quaternions (x, y, z, s); None = identity, upright), swept without turning from
        `origins` along `directions` ((n, 3) each).  `max_t`, `ignore_body` and the result are raycast()'s: t, normal (from the collider to the
        capsule), body, collider, shape, tag and `raw`.  Nothing waits unless `synchronize`."""
        casts, _ = self._capsule_casts("capsulecast", origins, directions, radii, half_heights, rotations, max_t, ignore_body)
        return self._ray_hits(self.capsulecast_records(casts, any_hit=any_hit), synchronize)

    def boxcast_all_records(self, casts, offsets=None, hits=None, capacity=0):
        """nh_boxcast_all on records already laid out as nh_BoxCast (count x 64 bytes): raycast_all_records for swept oriented boxes."""
        return self._list_records("nh_boxcast_all", 64, 32, casts, offsets, hits, capacity)

    def capsulecast_all_records(self, casts, offsets=None, hits=None, capacity=0):
        """nh_capsulecast_all on records already laid out as nh_CapsuleCast (count x 64 bytes): raycast_all_records for swept capsules."""
        return self._list_records("nh_capsulecast_all", 64, 32, casts, offsets, hits, capacity)

    def boxcast_all(self, origins, directions, half_extents, rotations=None, max_t=float("inf"), ignore_body=None, capacity=None, synchronize=False):
        """Every collider each of n swept oriented boxes touches, ordered along the cast (nh_boxcast_all): boxcast()'s arguments, raycast_all()'s
        capacity rule and result (normal: from the collider to the cast box); the first record of a cast is boxcast()'s closest hit."""
        casts, n = self._box_casts("boxcast_all", origins, directions, half_extents, rotations, max_t, ignore_body)
        return self._castall(self.boxcast_all_records, casts, n, capacity, synchronize)

    def capsulecast_all(self, origins, directions, radii, half_heights, rotations=None, max_t=float("inf"), ignore_body=None, capacity=None,
                        synchronize=False):
        """Every collider each of n swept capsules touches, ordered along the cast (nh_capsulecast_all): capsulecast()'s arguments, raycast_all()'s
        capacity rule and result (normal: from the collider to the capsule); the first record of a cast is capsulecast()'s closest hit."""
        casts, n = self._capsule_casts("capsulecast_all", origins, directions, radii, half_heights, rotations, max_t, ignore_body)
        return self._castall(self.capsulecast_all_records, casts, n, capacity, synchronize)

    def _castk_records(self, name, size, casts, k, counts, hits):
        torch = self.torch
        n = casts.numel() * casts.element_size() // size
        if counts is None:
            counts = torch.empty(n, dtype=torch.int32, device=self.dev)
        if hits is None:
            hits = torch.empty((n, max(int(k), 0), 32), dtype=torch.uint8, device=self.dev)
        _check(self.L, getattr(self.L, name)(self.ctx, C.c_void_p(casts.data_ptr() if n else 0), n, k, C.c_void_p(counts.data_ptr() if n else 0),
                                             C.c_void_p(hits.data_ptr() if n else 0), 0), name)
        return counts, hits

    def raycast_k_records(self, rays, k, counts=None, hits=None):
        """nh_raycast_k on records already laid out as nh_Ray: `rays` a contiguous device tensor of count x 32 bytes (any dtype).  Returns
        (counts, hits): the count words as an int32 device tensor (`counts`, or a new one) and the count x k x 32-byte uint8 device tensor of
        nh_RayHit records (`hits`, or a new one), the k of a cast in ascending t, misses behind them.  Enqueued; nothing waits or allocates."""
        return self._castk_records("nh_raycast_k", 32, rays, k, counts, hits)

    def spherecast_k_records(self, casts, k, counts=None, hits=None):
        """nh_spherecast_k on records already laid out as nh_SphereCast (count x 48 bytes): raycast_k_records for swept balls."""
        return self._castk_records("nh_spherecast_k", 48, casts, k, counts, hits)

    def boxcast_k_records(self, casts, k, counts=None, hits=None):
        """nh_boxcast_k on records already laid out as nh_BoxCast (count x 64 bytes): raycast_k_records for swept oriented boxes."""
        return self._castk_records("nh_boxcast_k", 64, casts, k, counts, hits)

    def capsulecast_k_records(self, casts, k, counts=None, hits=None):
        """nh_capsulecast_k on records already laid out as nh_CapsuleCast (count x 64 bytes): raycast_k_records for swept capsules."""
        return self._castk_records("nh_capsulecast_k", 64, casts, k, counts, hits)

    def _castk(self, records, casts, n, k, synchronize):
        counts, raw = records(casts, k)
        hits = self._ray_hits(raw, synchronize)
        return counts.to(self.torch.int64), {name: v if name == "raw" else v.reshape((n, k) + tuple(v.shape[1:])) for name, v in hits.items()}

    def raycast_k(self, origins, directions, k, max_t=float("inf"), ignore_body=None, synchronize=False):
        """The first `k` (1 .. 32) colliders along each of n rays (nh_raycast_k), against the last query_build(); the other arguments are raycast()'s.
        Returns (counts, hits): counts (n, int64: how many of the k slots of a ray hold a hit) and raycast()'s dict shaped (n, k) -- t, normal
        ((n, k, 3)), body, collider, shape, tag (0xffffffff in the slots behind the count, whose t is max_t) and `raw`, the nh_RayHit records
        (n x k x 32 bytes) -- in ascending t, ties by combined collider index; the first is raycast()'s closest hit.  One launch, whatever the
        casts pierce; nothing waits for the device unless `synchronize`."""
        rays, n = self._cast_head("raycast_k", origins, directions, max_t, ignore_body, 8)
        return self._castk(self.raycast_k_records, rays, n, k, synchronize)

    def spherecast_k(self, origins, directions, radii, k, max_t=float("inf"), ignore_body=None, synchronize=False):
        """The first `k` colliders each of n swept balls touches (nh_spherecast_k): spherecast()'s arguments, raycast_k()'s result."""
        torch = self.torch
        casts, n = self._cast_head("spherecast_k", origins, directions, max_t, ignore_body, 12)
        casts[:, 8] = torch.as_tensor(radii, dtype=torch.float32, device=self.dev).reshape(-1)
        return self._castk(self.spherecast_k_records, casts, n, k, synchronize)

    def boxcast_k(self, origins, directions, half_extents, k, rotations=None, max_t=float("inf"), ignore_body=None, synchronize=False):
        """The first `k` colliders each of n swept oriented boxes touches (nh_boxcast_k): boxcast()'s arguments, raycast_k()'s result."""
        casts, n = self._box_casts("boxcast_k", origins, directions, half_extents, rotations, max_t, ignore_body)
        return self._castk(self.boxcast_k_records, casts, n, k, synchronize)

    def capsulecast_k(self, origins, directions, radii, half_heights, k, rotations=None, max_t=float("inf"), ignore_body=None, synchronize=False):
        """The first `k` colliders each of n swept capsules touches (nh_capsulecast_k): capsulecast()'s arguments, raycast_k()'s result."""
        casts, n = self._capsule_casts("capsulecast_k", origins, directions, radii, half_heights, rotations, max_t, ignore_body)
        return self._castk(self.capsulecast_k_records, casts, n, k, synchronize)

    def closest_records(self, queries, hits=None):
        """nh_closest on records already laid out as nh_PointQuery: `queries` a contiguous device tensor of count x 32 bytes (any dtype).  Returns
        the count x 48-byte uint8 device tensor of nh_PointHit records (`hits`, or a new one)."""
        return self._records("nh_closest", 32, 48, queries, hits)

    def _point_queries(self, points, max_distance, ignore_body):
        """The nh_PointQuery records (n x 8 float32 words on the device) of closest() / closest_k()'s arguments: (records, n)."""
        torch = self.torch
        p = torch.as_tensor(points, dtype=torch.float32, device=self.dev).reshape(-1, 3)
        n = p.shape[0]
        queries = torch.zeros((n, 8), dtype=torch.float32, device=self.dev)
        queries[:, 0:3] = p
        queries[:, 3] = torch.as_tensor(max_distance, dtype=torch.float32, device=self.dev)
        queries.view(torch.int32)[:, 4] = self._ignore_bits(ignore_body)
        return queries, n

    def closest(self, points, max_distance=float("inf"), ignore_body=None, synchronize=False):
        """The nearest collider to each of `points` ((n, 3)) in the last query_build(), within `max_distance` (a number or n values; inf: anywhere),
        skipping the colliders of `ignore_body` (None, a body index, or n of them).  Returns a dict of device tensors: distance (n; negative inside),
        normal (n, 3; out of the collider), point (n, 3; on its surface), body, collider, shape, tag (n, int64; 0xffffffff = none) and `raw`, the
        nh_PointHit records.  Nothing waits for the device unless `synchronize`."""
        torch = self.torch
        queries, n = self._point_queries(points, max_distance, ignore_body)
        raw = self.closest_records(queries)
        f = raw.view(torch.float32).reshape(n, 12)
        u = raw.view(torch.int32).reshape(n, 12).to(torch.int64) & 0xFFFFFFFF
        out = dict(distance=f[:, 0], normal=f[:, 1:4], point=f[:, 4:7], body=u[:, 7], collider=u[:, 8], shape=u[:, 9], tag=u[:, 10], raw=raw)
        if synchronize:
            torch.cuda.current_stream(self.dev).synchronize()
        return out

    def closest_k_records(self, queries, k, counts=None, hits=None):
        """nh_closest_k on records already laid out as nh_PointQuery: `queries` a contiguous device tensor of count x 32 bytes (any dtype).  Returns
        (counts, hits): the count words as an int32 device tensor (`counts`, or a new one) and the count x k x 48-byte uint8 device tensor of
        nh_PointHit records (`hits`, or a new one), the k of a query nearest first."""
        torch = self.torch
        n = queries.numel() * queries.element_size() // 32
        if counts is None:
            counts = torch.empty(n, dtype=torch.int32, device=self.dev)
        if hits is None:
            hits = torch.empty((n, max(int(k), 0), 48), dtype=torch.uint8, device=self.dev)
        _check(self.L, self.L.nh_closest_k(self.ctx, C.c_void_p(queries.data_ptr() if n else 0), n, k, C.c_void_p(counts.data_ptr() if n else 0),
                                           C.c_void_p(hits.data_ptr() if n else 0), 0), "nh_closest_k")
        return counts, hits

    def closest_k(self, points, k, max_distance=float("inf"), ignore_body=None, synchronize=False):
        """The `k` (1 .. 32) nearest colliders to each of `points` ((n, 3)) in the last query_build(), nearest first; `max_distance` and `ignore_body`
        are closest()'s.  Returns a dict of device tensors: count (n, int64: how many of the k slots of a point hold a collider), distance (n, k),
        normal (n, k, 3), point (n, k, 3), body, collider, shape, tag ((n, k), int64; 0xffffffff in the slots behind `count`) and `raw`, the
        nh_PointHit records (n x k x 48 bytes).  Nothing waits for the device unless `synchronize`."""
        torch = self.torch
        queries, n = self._point_queries(points, max_distance, ignore_body)
        counts, raw = self.closest_k_records(queries, k)
        f = raw.view(torch.float32).reshape(n, k, 12)
        u = raw.view(torch.int32).reshape(n, k, 12).to(torch.int64) & 0xFFFFFFFF
        out = dict(count=counts.to(torch.int64), distance=f[..., 0], normal=f[..., 1:4], point=f[..., 4:7], body=u[..., 7], collider=u[..., 8],
                   shape=u[..., 9], tag=u[..., 10], raw=raw)
        if synchronize:
            torch.cuda.current_stream(self.dev).synchronize()
        return out

    def distance_records(self, queries, hits=None):
        """nh_distance on records already laid out as nh_DistanceQuery: `queries` a contiguous device tensor of count x 64 bytes (any dtype).  Returns
        the count x 48-byte uint8 device tensor of nh_PointHit records (`hits`, or a new one)."""
        return self._records("nh_distance", 64, 48, queries, hits)

    def distance(self, centres, radii=None, half_extents=None, rotations=None, half_heights=None, max_distance=float("inf"), ignore_body=None,
                 synchronize=False):
        """How far each of n spheres, oriented boxes or capsules (overlap()'s shape arguments) is from the nearest collider of the last query_build(),
        within `max_distance` (a number or n values; inf: anywhere), skipping the colliders of `ignore_body`.  Returns closest()'s dict: distance
        (n; 0 where the shape touches a collider), normal (n, 3; a unit vector from the collider towards the shape, 0 where they touch), point
        (n, 3; on the collider's surface -- the shape's own nearest point is point + distance * normal), body, collider, shape, tag (n, int64;
        0xffffffff = none) and `raw`, the nh_PointHit records.  Nothing waits for the device unless `synchronize`."""
        torch = self.torch
        q, n = self._overlap_queries("distance", centres, radii, half_extents, rotations, ignore_body, half_heights)
        queries = torch.zeros((n, 16), dtype=torch.float32, device=self.dev)
        queries[:, 0:12] = q
        queries[:, 12] = torch.as_tensor(max_distance, dtype=torch.float32, device=self.dev)
        raw = self.distance_records(queries)
        f = raw.view(torch.float32).reshape(n, 12)
        u = raw.view(torch.int32).reshape(n, 12).to(torch.int64) & 0xFFFFFFFF
        out = dict(distance=f[:, 0], normal=f[:, 1:4], point=f[:, 4:7], body=u[:, 7], collider=u[:, 8], shape=u[:, 9], tag=u[:, 10], raw=raw)
        if synchronize:
            torch.cuda.current_stream(self.dev).synchronize()
        return out

    def move_records(self, records, results=None):
        """nh_move on records already laid out as nh_Move: `records` a contiguous device tensor of count x 64 bytes (any dtype).  Returns the
        count x 64-byte uint8 device tensor of nh_MoveResult records (`results`, or a new one)."""
        return self._records("nh_move", 64, 64, records, results)

    def move(self, origins, displacements, radius, half_height=0.0, rotations=None, skin=0.01, max_slides=4, ignore_body=None, synchronize=False, touched=None):
        """Collide-and-slide (nh_move) against the last query_build(): each of n capsules of `radius` and `half_height` (numbers or n values; half
        height 0 is a ball) and `rotations` ((n, 4) or (4,) quaternions (x, y, z, s); None = identity, upright) is moved from `origins` by
        `displacements` ((n, 3) each), sliding along what it hits, at most `max_slides` (0 .. NH_MOVE_MAX_SLIDES; a number or n values) times, and
        keeping `skin` (a number or n values, in world units: scale it to the scene) clear of it.  `ignore_body`: None, a body index, or n of them.
        Returns a dict of device tensors: position (n, 3), remaining (n, 3; the displacement not used), flags (n, int64; NH_MOVE_*), slides (n,
        int64), `last_hit` (capsulecast()'s dict for the last cast each move made) and `raw`, the nh_MoveResult records.  Nothing waits for the
        device unless `synchronize`.
        `touched` = k (1 .. NH_MOVE_MAX_TOUCHES): the call is nh_move_touched, and the dict gains `touch_count` (n, int64: every collider a cast of the
        move found, whatever k is) and `touches`, a dict of (n, k, ...) views of the nh_Touch records: capsulecast()'s fields of each touch's hit, and
        origin, direction (n, k, 3), phase, cast (n, k, int64) and `raw`.  Slots at or behind touch_count hold whatever the tensor held: they are not
        written."""
        return self._move("move", origins, displacements, (radius, half_height), rotations, skin, max_slides, ignore_body, synchronize, touched)

    def _mover_head(self, name, origins, displacements, shape, rotations, skin, max_slides, ignore_body):
        """The 64-byte records nh_Move (`name` move, walk; `shape` = (radius, half_height)) or nh_BoxMove (boxmove, boxwalk; (half_extents,)): the
        shape's cast records with `skin` at max_t and `max_slides` in the word behind the shape: (records, n)."""
        torch = self.torch
        pack, column = (self._box_casts, 15) if name.startswith("box") else (self._capsule_casts, 14)
        head, n = pack(name, origins, displacements, *shape, rotations, skin, ignore_body)
        head.view(torch.int32)[:, column] = torch.as_tensor(max_slides, dtype=torch.int64, device=self.dev).to(torch.int32)
        return head, n

    def _touched_records(self, name, in_bytes, out_bytes, records, k, results, counts, touches):
        """The C call `name`(ctx, records, count, results, k, counts, touches, 0) of the movers' _touched forms: `records` a contiguous device tensor
        of count x in_bytes bytes (any dtype).  Returns (results, counts, touches): the count x out_bytes uint8 result records, the count words as an
        int32 device tensor and the count x k x 64-byte uint8 tensor of nh_Touch records (each the one given, or a new one).  Of record i's k slots
        only the first min(counts[i], k) are written.  Enqueued; nothing waits, and nothing allocates where all three are given."""
        torch = self.torch
        n = records.numel() * records.element_size() // in_bytes
        if results is None:
            results = torch.empty((n, out_bytes), dtype=torch.uint8, device=self.dev)
        if counts is None:
            counts = torch.empty(n, dtype=torch.int32, device=self.dev)
        if touches is None:
            touches = torch.empty((n, max(int(k), 0), 64), dtype=torch.uint8, device=self.dev)
        _check(self.L, getattr(self.L, name)(self.ctx, C.c_void_p(records.data_ptr() if n else 0), n, C.c_void_p(results.data_ptr() if n else 0), k,
                                             C.c_void_p(counts.data_ptr() if n else 0), C.c_void_p(touches.data_ptr() if n else 0), 0), name)
        return results, counts, touches

    def move_touched_records(self, records, k, results=None, counts=None, touches=None):
        """nh_move_touched on records already laid out as nh_Move (count x 64 bytes): (results, counts, touches) -- move_records()'s nh_MoveResult
        records, the touches per move (int32) and the count x k x 64-byte nh_Touch records, k in 1 .. NH_MOVE_MAX_TOUCHES.  Slots at or behind a
        move's count are not written."""
        return self._touched_records("nh_move_touched", 64, 64, records, k, results, counts, touches)

    def boxmove_touched_records(self, records, k, results=None, counts=None, touches=None):
        """nh_boxmove_touched on records already laid out as nh_BoxMove (count x 64 bytes): move_touched_records()'s arguments and result."""
        return self._touched_records("nh_boxmove_touched", 64, 64, records, k, results, counts, touches)

    def walk_touched_records(self, records, k, results=None, counts=None, touches=None):
        """nh_walk_touched on records already laid out as nh_Walk (count x 96 bytes): (results, counts, touches) -- walk_records()'s nh_WalkResult
        records, the touches per walk (int32) and the count x k x 64-byte nh_Touch records, k in 1 .. NH_WALK_MAX_TOUCHES.  Slots at or behind a
        walk's count are not written."""
        return self._touched_records("nh_walk_touched", 96, 112, records, k, results, counts, touches)

    def boxwalk_touched_records(self, records, k, results=None, counts=None, touches=None):
        """nh_boxwalk_touched on records already laid out as nh_BoxWalk (count x 96 bytes): walk_touched_records()'s arguments and result."""
        return self._touched_records("nh_boxwalk_touched", 96, 112, records, k, results, counts, touches)

    def _mover_call(self, name, rec, touched, out):
        """The mover nh_`name` on the packed records `rec`: its result records, from the plain call or, with `touched` = k, from the _touched form,
        which also puts `touch_count` and `touches` into `out`."""
        torch = self.torch
        if touched is None:
            return getattr(self, name + "_records")(rec)
        raw, counts, touches = getattr(self, name + "_touched_records")(rec, touched)
        n, k = touches.shape[0], touches.shape[1]
        f = touches.view(torch.float32).reshape(n, k, 16)
        u = touches.view(torch.int32).reshape(n, k, 16).to(torch.int64) & 0xFFFFFFFF
        out["touch_count"] = counts.to(torch.int64)
        out["touches"] = dict(t=f[:, :, 0], normal=f[:, :, 1:4], body=u[:, :, 4], collider=u[:, :, 5], shape=u[:, :, 6], tag=u[:, :, 7], origin=f[:, :, 8:11],
                              phase=u[:, :, 11], direction=f[:, :, 12:15], cast=u[:, :, 15], raw=touches)
        return raw

    def _move(self, name, origins, displacements, shape, rotations, skin, max_slides, ignore_body, synchronize, touched=None):
        """move() and boxmove(): the dict they return, from the nh_MoveResult records of the call nh_`name` (nh_`name`_touched with `touched` = k)."""
        torch = self.torch
        rec, n = self._mover_head(name, origins, displacements, shape, rotations, skin, max_slides, ignore_body)
        more = {}
        raw = self._mover_call(name, rec, touched, more)
        f = raw.view(torch.float32).reshape(n, 16)
        u = raw.view(torch.int32).reshape(n, 16).to(torch.int64) & 0xFFFFFFFF
        out = dict(position=f[:, 0:3], remaining=f[:, 4:7], flags=u[:, 3], slides=u[:, 7], last_hit=self._ray_hits(raw.reshape(n, 64)[:, 32:].contiguous(), False),
                   raw=raw, **more)
        if synchronize:
            torch.cuda.current_stream(self.dev).synchronize()
        return out

    def boxmove_records(self, records, results=None):
        """nh_boxmove on records already laid out as nh_BoxMove: `records` a contiguous device tensor of count x 64 bytes (any dtype).  Returns the
        count x 64-byte uint8 device tensor of nh_MoveResult records (`results`, or a new one)."""
        return self._records("nh_boxmove", 64, 64, records, results)

    def boxmove(self, origins, displacements, half_extents, rotations=None, skin=0.01, max_slides=4, ignore_body=None, synchronize=False, touched=None):
        """Collide-and-slide for oriented boxes (nh_boxmove) against the last query_build(): move() with boxcast()'s shape -- `half_extents` ((n, 3)
        or (3,)) and `rotations` ((n, 4) or (4,) quaternions (x, y, z, s); None = identity, axis-aligned); the box does not turn while it moves.
        `skin`, `max_slides`, `ignore_body`, `touched` (nh_boxmove_touched) and the returned dict are move()'s, with boxcast()'s dict as `last_hit`.
        Nothing waits for the device unless `synchronize`."""
        return self._move("boxmove", origins, displacements, (half_extents,), rotations, skin, max_slides, ignore_body, synchronize, touched)

    def walk_records(self, records, results=None):
        """nh_walk on records already laid out as nh_Walk: `records` a contiguous device tensor of count x 96 bytes (any dtype).  Returns the
        count x 112-byte uint8 device tensor of nh_WalkResult records (`results`, or a new one)."""
        return self._records("nh_walk", 96, 112, records, results)

    def walk(self, origins, displacements, radius, half_height=0.0, rotations=None, skin=0.01, max_slides=4, ignore_body=None, up=(0.0, 1.0, 0.0),
             step_height=0.0, snap_distance=0.0, max_slope_degrees=None, min_ground_up=None, probe_only=False, synchronize=False, touched=None):
        """A grounded character step (nh_walk) against the last query_build(): move()'s capsules, moved from `origins` by `displacements` with move()'s
        `skin`, `max_slides` and `ignore_body`, climbing risers up to `step_height`, treating faces steeper than the slope limit as walls, and
        following ground found within `snap_distance` below.  `up`: the unit vector against gravity ((3,) or (n, 3)).  The slope limit is
        `max_slope_degrees` (the steepest ground, in degrees) or `min_ground_up` (its cosine); give one, or neither for no limit.  `step_height`,
        `snap_distance`, the limit and `probe_only` (look for ground, do not move onto it) are numbers or n values.
        Returns move()'s dict for the slide that was kept -- position, remaining, flags (NH_MOVE_* and NH_WALK_*), slides, last_hit -- plus `ground`
        (capsulecast()'s dict of what the capsule stands on), step_up, drop (n, float32), casts (n, int64) and `raw`, the nh_WalkResult records.
        Nothing waits for the device unless `synchronize`.
        `touched` = k (1 .. NH_WALK_MAX_TOUCHES): the call is nh_walk_touched, and the dict gains move()'s `touch_count` and `touches` for everything the
        walk probed, kept or not (phase: NH_TOUCH_*; with NH_WALK_STEPPED set UP, FORWARD and DOWN are the path taken, without it SLIDE and PROBE).
        Slots at or behind touch_count hold whatever the tensor held: they are not written."""
        return self._walk("walk", origins, displacements, (radius, half_height), rotations, skin, max_slides, ignore_body, up, step_height,
                          snap_distance, max_slope_degrees, min_ground_up, probe_only, synchronize, touched)

    def _walk(self, name, origins, displacements, shape, rotations, skin, max_slides, ignore_body, up, step_height, snap_distance, max_slope_degrees,
              min_ground_up, probe_only, synchronize, touched=None):
        """walk() and boxwalk(): nh_Walk / nh_BoxWalk records -- the 64-byte head followed by walk()'s rules -- and the dict they return, from the
        nh_WalkResult records of the call nh_`name` (nh_`name`_touched with `touched` = k)."""
        torch = self.torch
        if max_slope_degrees is not None and min_ground_up is not None:
            raise ValueError(f"{name}: give max_slope_degrees or min_ground_up, not both")
        head, n = self._mover_head(name, origins, displacements, shape, rotations, skin, max_slides, ignore_body)
        rec = torch.zeros((n, 24), dtype=torch.float32, device=self.dev)
        rec[:, 0:16] = head
        rec[:, 16:19] = torch.as_tensor(up, dtype=torch.float32, device=self.dev).reshape(-1, 3)
        rec[:, 19] = torch.as_tensor(step_height, dtype=torch.float32, device=self.dev).reshape(-1)
        rec[:, 20] = torch.as_tensor(snap_distance, dtype=torch.float32, device=self.dev).reshape(-1)
        if max_slope_degrees is not None:
            min_ground_up = torch.cos(torch.deg2rad(torch.as_tensor(max_slope_degrees, dtype=torch.float64, device=self.dev)))
        rec[:, 21] = torch.as_tensor(0.0 if min_ground_up is None else min_ground_up, device=self.dev).to(torch.float32).reshape(-1)
        rec.view(torch.int32)[:, 22] = torch.as_tensor(probe_only, device=self.dev).to(torch.int32).reshape(-1) & 1
        more = {}
        raw = self._mover_call(name, rec, touched, more)
        f = raw.view(torch.float32).reshape(n, 28)
        u = raw.view(torch.int32).reshape(n, 28).to(torch.int64) & 0xFFFFFFFF
        bytes_ = raw.reshape(n, 112)
        out = dict(position=f[:, 0:3], remaining=f[:, 4:7], flags=u[:, 3], slides=u[:, 7], last_hit=self._ray_hits(bytes_[:, 32:64].contiguous(), False),
                   ground=self._ray_hits(bytes_[:, 64:96].contiguous(), False), step_up=f[:, 24], drop=f[:, 25], casts=u[:, 26], raw=raw, **more)
        if synchronize:
            torch.cuda.current_stream(self.dev).synchronize()
        return out

    def boxwalk_records(self, records, results=None):
        """nh_boxwalk on records already laid out as nh_BoxWalk: `records` a contiguous device tensor of count x 96 bytes (any dtype).  Returns the
        count x 112-byte uint8 device tensor of nh_WalkResult records (`results`, or a new one)."""
        return self._records("nh_boxwalk", 96, 112, records, results)

    def boxwalk(self, origins, displacements, half_extents, rotations=None, skin=0.01, max_slides=4, ignore_body=None, up=(0.0, 1.0, 0.0),
                step_height=0.0, snap_distance=0.0, max_slope_degrees=None, min_ground_up=None, probe_only=False, synchronize=False, touched=None):
        """A grounded step for oriented boxes (nh_boxwalk) against the last query_build(): walk() with boxmove()'s shape (`half_extents`, `rotations`;
        None = identity: an axis-aligned character).  Every other argument (`touched`: nh_boxwalk_touched) and the returned dict are walk()'s, with
        boxcast()'s dicts as `last_hit` and `ground`.  Nothing waits for the device unless `synchronize`."""
        return self._walk("boxwalk", origins, displacements, (half_extents,), rotations, skin, max_slides, ignore_body, up, step_height,
                          snap_distance, max_slope_degrees, min_ground_up, probe_only, synchronize, touched)

    def recover_records(self, records, results=None):
        """nh_recover on records already laid out as nh_Recover: `records` a contiguous device tensor of count x 64 bytes (any dtype).  Returns the
        count x 64-byte uint8 device tensor of nh_RecoverResult records (`results`, or a new one)."""
        return self._records("nh_recover", 64, 64, records, results)

    def recover(self, centres, radii=None, half_extents=None, rotations=None, half_heights=None, skin=0.01, max_iterations=4, ignore_body=None,
                synchronize=False):
        """Push each of n spheres, oriented boxes or capsules (overlap()'s shape arguments) out of everything it overlaps in the last query_build()
        (nh_recover): at most `max_iterations` (0 .. NH_RECOVER_MAX_ITERATIONS; a number or n values) pushes, each out of the deepest collider and
        `skin` (a number or n values, in world units: scale it to the scene) further.  `ignore_body`: None, a body index, or n of them.
        Returns a dict of device tensors: position (n, 3), push (n, 3; position - centre), flags (n, int64; NH_RECOVER_*: without OVERLAPPING,
        TOUCHING and INVALID the shape is free at `position`), iterations (n, int64), `last` (the deepest pair of the last walk that found one:
        normal, depth, body, collider, shape, tag; 0xffffffff = none) and `raw`, the nh_RecoverResult records.  Nothing waits for the device
        unless `synchronize`."""
        torch = self.torch
        q, n = self._overlap_queries("recover", centres, radii, half_extents, rotations, ignore_body, half_heights)
        rec = torch.zeros((n, 16), dtype=torch.float32, device=self.dev)
        rec[:, 0:12] = q
        rec[:, 12] = torch.as_tensor(skin, dtype=torch.float32, device=self.dev)
        rec.view(torch.int32)[:, 13] = torch.as_tensor(max_iterations, dtype=torch.int64, device=self.dev).to(torch.int32)
        raw = self.recover_records(rec)
        f = raw.view(torch.float32).reshape(n, 16)
        u = raw.view(torch.int32).reshape(n, 16).to(torch.int64) & 0xFFFFFFFF
        last = dict(normal=f[:, 8:11], depth=f[:, 11], body=u[:, 12], collider=u[:, 13], shape=u[:, 14], tag=u[:, 15])
        out = dict(position=f[:, 0:3], push=f[:, 4:7], flags=u[:, 3], iterations=u[:, 7], last=last, raw=raw)
        if synchronize:
            torch.cuda.current_stream(self.dev).synchronize()
        return out

    def overlap_records(self, queries, offsets=None, hits=None, capacity=0):
        """nh_overlap on records already laid out as nh_OverlapQuery: `queries` a contiguous device tensor of count x 48 bytes (any dtype).  Returns
        (offsets, hits): the count + 1 offsets as an int32 device tensor holding the uint32 bits (`offsets`, or a new one) and `hits` as given.  With
        hits = None and capacity = 0 only the offsets are written (count only); otherwise `hits` must hold `capacity` x 16 bytes, and the records of
        query i are written iff offsets[i + 1] <= capacity.  Enqueued; nothing waits (but a capacity larger than any before grows the scratch)."""
        return self._list_records("nh_overlap", 48, 16, queries, offsets, hits, capacity)

    def _overlap_queries(self, what, centres, radii, half_extents, rotations, ignore_body, half_heights):
        """The nh_OverlapQuery records (n x 12 float32 words on the device) of overlap() / penetration()'s arguments."""
        torch = self.torch
        if (radii is None) == (half_extents is None):
            raise ValueError(f"{what}: give exactly one of radii / half_extents")
        if half_heights is not None and radii is None:
            raise ValueError(f"{what}: half_heights go with radii (a capsule)")
        c = torch.as_tensor(centres, dtype=torch.float32, device=self.dev).reshape(-1, 3)
        n = c.shape[0]
        q = torch.zeros((n, 12), dtype=torch.float32, device=self.dev)
        qi = q.view(torch.int32)
        q[:, 0:3] = c
        if half_heights is not None:
            qi[:, 3] = NH_SHAPE_CAPSULE
            q[:, 8] = torch.as_tensor(radii, dtype=torch.float32, device=self.dev).reshape(-1)
            q[:, 9] = torch.as_tensor(half_heights, dtype=torch.float32, device=self.dev).reshape(-1)
            if rotations is None:
                q[:, 7] = 1.0
            else:
                q[:, 4:8] = torch.as_tensor(rotations, dtype=torch.float32, device=self.dev).reshape(-1, 4)
        elif radii is not None:
            qi[:, 3] = NH_SHAPE_SPHERE
            q[:, 8] = torch.as_tensor(radii, dtype=torch.float32, device=self.dev).reshape(-1)
            q[:, 7] = 1.0
        else:
            qi[:, 3] = NH_SHAPE_BOX
            q[:, 8:11] = torch.as_tensor(half_extents, dtype=torch.float32, device=self.dev).reshape(-1, 3)
            if rotations is None:
                q[:, 7] = 1.0
            else:
                q[:, 4:8] = torch.as_tensor(rotations, dtype=torch.float32, device=self.dev).reshape(-1, 4)
        qi[:, 11] = self._ignore_bits(ignore_body)
        return q, n

    def _overlap_lists(self, records, q, n, capacity, size):
        """The count-then-list path (capacity=None) or the one call with a capacity, through `records` (overlap_records / penetration_records) with
        records of `size` bytes: (int32 offsets, hits, n, the capacity of `hits`), what _list_index and the unpackers take."""
        torch = self.torch
        if capacity is None:
            offsets, _ = records(q)
            total = int(offsets[n].item()) & 0xFFFFFFFF if n else 0          # (a synchronisation)
            capacity = 0 if total == NH_OVERLAP_OVERFLOW else total
            hits = torch.empty((capacity, size), dtype=torch.uint8, device=self.dev)
            if capacity:
                records(q, offsets=offsets, hits=hits, capacity=capacity)
        else:
            hits = torch.empty((capacity, size), dtype=torch.uint8, device=self.dev)
            offsets, _ = records(q, hits=hits if capacity else None, capacity=capacity)
        return offsets, hits, n, capacity

    def _list_index(self, offsets, n, capacity):
        """What every list dict starts with, from a list's int32 offsets (n + 1) and capacity: offsets (int64), written, the query of every record slot."""
        torch = self.torch
        off = offsets.to(torch.int64) & 0xFFFFFFFF
        # the written prefix: the largest offset <= capacity (offsets are monotone unless the total overflowed, and then nothing is written)
        last = torch.searchsorted(off, torch.tensor([capacity], dtype=torch.int64, device=self.dev), right=True) - 1
        written = torch.where(off[n] == NH_OVERLAP_OVERFLOW, torch.zeros_like(last), off[last.clamp(min=0)])[0]
        j = torch.arange(capacity, dtype=torch.int64, device=self.dev)
        query = (torch.searchsorted(off[1:], j, right=True) if n else j).clamp(max=max(n - 1, 0))
        return dict(offsets=off, written=written, query=query)

    def _list_dict(self, offsets, hits, n, capacity, synchronize=False):
        """overlap()'s dict of a list: int32 offsets (n + 1), the nh_OverlapHit records (capacity x 16 bytes)."""
        torch = self.torch
        u = hits.view(torch.int32).reshape(-1, 4).to(torch.int64) & 0xFFFFFFFF
        r = dict(self._list_index(offsets, n, capacity), body=u[:, 0], collider=u[:, 1], shape=u[:, 2], tag=u[:, 3], raw=hits)
        if synchronize:
            torch.cuda.current_stream(self.dev).synchronize()
        return r

    def _penetration_dict(self, offsets, hits, n, capacity, synchronize=False):
        """penetration()'s dict of a list: int32 offsets (n + 1), the nh_PenetrationHit records (capacity x 32 bytes)."""
        torch = self.torch
        f = hits.view(torch.float32).reshape(-1, 8)
        u = hits.view(torch.int32).reshape(-1, 8).to(torch.int64) & 0xFFFFFFFF
        r = dict(self._list_index(offsets, n, capacity), normal=f[:, 0:3], depth=f[:, 3], body=u[:, 4], collider=u[:, 5], shape=u[:, 6], tag=u[:, 7], raw=hits)
        if synchronize:
            torch.cuda.current_stream(self.dev).synchronize()
        return r

    def overlap(self, centres, radii=None, half_extents=None, rotations=None, ignore_body=None, capacity=None, synchronize=False, half_heights=None):
        """The colliders touching each of n spheres (`radii`: a number or n values), n oriented boxes (`half_extents` (n, 3) or (3,), `rotations`
        (n, 4) or (4,) quaternions (x, y, z, s), default identity) or n capsules (`radii` with `half_heights`, numbers or n values, and `rotations`;
        the axis is the local y axis), against the last query_build().  Give exactly one of radii / half_extents; mixed batches go through
        overlap_records.  `ignore_body`: None, a body index, or n of them.
        capacity=None: a count call, then the total is read -- this WAITS for the device -- and an exactly sized list call.  A capacity: one call, and
        nothing waits; only the segments that fit are listed (offsets[i + 1] <= capacity).
        Returns a dict of device tensors: offsets (n + 1, int64; offsets[n] = 0xffffffff when the total is 2^32 - 1 or more), `written` (0-d: the
        records listed, a prefix of whole segments), and per record slot (capacity of them; the first `written` are meaningful) query, body,
        collider, shape, tag (int64) and `raw`, the nh_OverlapHit records (capacity x 16 bytes)."""
        q, n = self._overlap_queries("overlap", centres, radii, half_extents, rotations, ignore_body, half_heights)
        return self._list_dict(*self._overlap_lists(self.overlap_records, q, n, capacity, 16), synchronize)

    def penetration_records(self, queries, offsets=None, hits=None, capacity=0):
        """nh_penetration on records already laid out as nh_OverlapQuery: overlap_records with 32-byte nh_PenetrationHit records -- `hits` must hold
        `capacity` x 32 bytes.  The offsets, the set, the order and the capacity rule are nh_overlap's.  Enqueued; nothing waits (but a capacity
        larger than any before grows the scratch)."""
        return self._list_records("nh_penetration", 48, 32, queries, offsets, hits, capacity)

    def penetration(self, centres, radii=None, half_extents=None, rotations=None, ignore_body=None, capacity=None, synchronize=False, half_heights=None):
        """The push that frees a shape: for every collider that each of n spheres, oriented boxes or capsules touches (overlap()'s arguments, set,
        order and count-then-list path), the least translation of the shape after which the two only touch.
        Returns overlap()'s dict with, per record slot, `normal` ((capacity, 3) float32: a unit vector from the collider towards the shape) and
        `depth` (float32, >= 0: the shape moved by depth * normal touches the collider); `raw` holds the nh_PenetrationHit records
        (capacity x 32 bytes)."""
        q, n = self._overlap_queries("penetration", centres, radii, half_extents, rotations, ignore_body, half_heights)
        return self._penetration_dict(*self._overlap_lists(self.penetration_records, q, n, capacity, 32), synchronize)

    # ---- the wide forms: nh_overlap's and nh_penetration's bytes, the work of one query spread over the GPU (include/nudge_hip.h, "nh_overlap_wide") ----
    def overlap_wide_records(self, queries, offsets=None, hits=None, capacity=0):
        """nh_overlap_wide on nh_OverlapQuery records: overlap_records' arguments, rules and bytes.  Enqueued; nothing waits (but a capacity or a
        count larger than any before grows the scratch)."""
        return self._list_records("nh_overlap_wide", 48, 16, queries, offsets, hits, capacity)

    def penetration_wide_records(self, queries, offsets=None, hits=None, capacity=0):
        """nh_penetration_wide on nh_OverlapQuery records: penetration_records' arguments, rules and bytes (32-byte records)."""
        return self._list_records("nh_penetration_wide", 48, 32, queries, offsets, hits, capacity)

    def overlap_wide(self, centres, radii=None, half_extents=None, rotations=None, ignore_body=None, capacity=None, synchronize=False, half_heights=None):
        """overlap() for LARGE volumes -- an explosion radius, a trigger volume, an area of interest: the same arguments and the same dict, byte for
        byte, through nh_overlap_wide, which spreads the work of one query over the GPU where overlap() gives it one lane.  Which of the two is faster
        depends on the size alone (header, "which call for which question"); a mixed batch is the caller's to split."""
        q, n = self._overlap_queries("overlap_wide", centres, radii, half_extents, rotations, ignore_body, half_heights)
        return self._list_dict(*self._overlap_lists(self.overlap_wide_records, q, n, capacity, 16), synchronize)

    def penetration_wide(self, centres, radii=None, half_extents=None, rotations=None, ignore_body=None, capacity=None, synchronize=False, half_heights=None):
        """penetration() for large volumes: the same arguments and the same dict, byte for byte, through nh_penetration_wide (see overlap_wide)."""
        q, n = self._overlap_queries("penetration_wide", centres, radii, half_extents, rotations, ignore_body, half_heights)
        return self._penetration_dict(*self._overlap_lists(self.penetration_wide_records, q, n, capacity, 32), synchronize)

    def region_records(self, regions, offsets=None, hits=None, capacity=0):
        """nh_region on records already laid out as nh_Region: `regions` a contiguous device tensor of count x 144 bytes (any dtype).  Returns
        (offsets, hits) as overlap_records does, under the same count-only and capacity rules, with 16-byte nh_OverlapHit records.  Enqueued; nothing
        waits (but a capacity or a count larger than any before grows the scratch)."""
        return self._list_records("nh_region", 144, 16, regions, offsets, hits, capacity)

    def region(self, planes, plane_counts=None, ignore_body=None, capacity=None, synchronize=False):
        """The colliders inside each of n convex regions, against the last query_build() / query_refit(): `planes` is (n, P, 4) or (P, 4) with P <= 8,
        plane (nx, ny, nz, d) keeping the side where n.x + d >= 0 (engine.frustum_planes gives a camera's six); `plane_counts` (a number or n values,
        default P) says how many of a region's planes count; `ignore_body`: None, a body index, or n of them.  The test is the plane-by-plane frustum
        test: it never misses a collider that reaches into the region and may list one just outside an edge or corner.
        `capacity` and the returned dict are overlap()'s: offsets, written, and per record slot query (the region), body, collider, shape, tag, raw."""
        torch = self.torch
        pl = torch.as_tensor(planes, dtype=torch.float32, device=self.dev)
        if pl.dim() == 2:
            pl = pl[None]
        if pl.dim() != 3 or pl.shape[2] != 4 or pl.shape[1] > NH_REGION_MAX_PLANES:
            raise ValueError(f"region: planes must be (n, P, 4) or (P, 4) with P <= {NH_REGION_MAX_PLANES}, not {tuple(pl.shape)}")
        n, P = pl.shape[0], pl.shape[1]
        q = torch.zeros((n, 36), dtype=torch.float32, device=self.dev)
        qi = q.view(torch.int32)
        q[:, :4 * P] = pl.reshape(n, 4 * P)
        qi[:, 32] = torch.as_tensor(P if plane_counts is None else plane_counts, dtype=torch.int32, device=self.dev)
        qi[:, 33] = self._ignore_bits(ignore_body)
        return self._list_dict(*self._overlap_lists(self.region_records, q, n, capacity, 16), synchronize)

    # ---- sensors: depth / id images from poses and one shared beam pattern (include/nudge_hip.h, "sensors") ----
    def _sense_counts(self, what, sensors, beams):
        ns, nb = sensors.numel() * sensors.element_size(), beams.numel() * beams.element_size()
        if ns % 48 or nb % 16:
            raise ValueError(f"{what}: sensors hold {ns} bytes (48 a record), beams {nb} (16 a record)")
        return ns // 48, nb // 16

    def sense_records(self, sensors, beams, t=None, body=None, tag=None, hits=None, any_hit=False, mounted=True):
        """nh_sense on records already laid out: `sensors` a contiguous device tensor of count x 48 bytes (nh_Sensor, engine.SENSOR), `beams` one of
        beam_count x 16 bytes (nh_Beam, engine.BEAM), any dtype.  Each channel is None (not asked for, costs nothing), True (a new tensor) or a device
        tensor of at least count * beam_count records to write into: t float32, body and tag int32 holding the uint32 bits, hits 32-byte nh_RayHit
        records as uint8.  mounted=False passes no bodies: every sensor is in the world frame and its `body` word is not read.  Returns the dict of
        the channels asked for.  Enqueued; nothing waits."""
        torch = self.torch
        count, beam_count = self._sense_counts("sense_records", sensors, beams)
        n = count * beam_count
        new = dict(t=lambda: torch.empty(n, dtype=torch.float32, device=self.dev), body=lambda: torch.empty(n, dtype=torch.int32, device=self.dev),
                   tag=lambda: torch.empty(n, dtype=torch.int32, device=self.dev), hits=lambda: torch.empty((n, 32), dtype=torch.uint8, device=self.dev))
        size = dict(t=4, body=4, tag=4, hits=32)
        out = {}
        for name, given in (("t", t), ("body", body), ("tag", tag), ("hits", hits)):
            if given is None or given is False:
                continue
            out[name] = new[name]() if given is True else given
            if out[name].numel() * out[name].element_size() < n * size[name]:
                raise ValueError(f"sense_records: {name} holds {out[name].numel() * out[name].element_size()} bytes, {n} rays need {n * size[name]}")
        so = SenseOut(*[out[k].data_ptr() if k in out and n else None for k in SENSE_CHANNELS])
        rc = self.L.nh_sense(self.ctx, C.byref(self.bodies) if mounted else None, C.c_void_p(sensors.data_ptr() if n else 0), count,
                             C.c_void_p(beams.data_ptr() if n else 0), beam_count, C.byref(so), NH_RAY_ANY_HIT if any_hit else 0)
        _check(self.L, rc, "nh_sense")
        return out

    def sense_rays_records(self, sensors, beams, rays=None, mounted=True):
        """nh_sense_rays: the nh_Ray record of every (sensor, beam) of sense_records' arguments, ray s * beam_count + j for beam j of sensor s.  Returns
        the count * beam_count x 32-byte uint8 device tensor (`rays`, or a new one)."""
        count, beam_count = self._sense_counts("sense_rays_records", sensors, beams)
        n = count * beam_count
        if rays is None:
            rays = self.torch.empty((n, 32), dtype=self.torch.uint8, device=self.dev)
        rc = self.L.nh_sense_rays(self.ctx, C.byref(self.bodies) if mounted else None, C.c_void_p(sensors.data_ptr() if n else 0), count,
                                  C.c_void_p(beams.data_ptr() if n else 0), beam_count, C.c_void_p(rays.data_ptr() if n else 0), 0)
        _check(self.L, rc, "nh_sense_rays")
        return rays

    def sense(self, positions, rotations, beams, bodies=None, ignore_body=None, channels=("t", "body"), any_hit=False, synchronize=False):
        """Depth / id images of n sensors that share one pattern, against the last query_build() / query_refit().  `positions` (n, 3) and `rotations`
        (n, 4; x, y, z, w) are the sensors' poses: in the world frame where `bodies` is None, else local to the body each rides on (`bodies`: a body
        index or n of them; 0xffffffff = that sensor is in the world frame) -- call query_refit() after stepping, the mounts read today's transforms.
        `beams`: engine.BEAM records (pinhole_beams, lidar_beams) or a (m, 4) array / tensor of (direction, range).  `ignore_body`: None, a body
        index, or n of them (a lidar's own vehicle).  `channels`: any of "t", "body", "tag", "hits".  Returns a dict of (n, m) device tensors: t
        (float32; the beam's range at a miss, NaN for an invalid ray), body and tag (int64; 0xffffffff = none), and for "hits" normal (n, m, 3),
        collider, shape and `raw`, the (n, m, 32) nh_RayHit records.  Nothing waits for the device unless `synchronize`."""
        torch = self.torch
        unknown = set(channels) - set(SENSE_CHANNELS)
        if unknown or not channels:
            raise ValueError(f"sense: channels must be some of {SENSE_CHANNELS}, not {tuple(channels)}")
        p = torch.as_tensor(positions, dtype=torch.float32, device=self.dev).reshape(-1, 3)
        q = torch.as_tensor(rotations, dtype=torch.float32, device=self.dev).reshape(-1, 4)
        n = p.shape[0]
        if q.shape[0] != n:
            raise ValueError(f"sense: {n} positions but {q.shape[0]} rotations")
        if isinstance(beams, np.ndarray) and beams.dtype == BEAM:
            beams = np.ascontiguousarray(beams).view(np.float32).reshape(-1, 4)
        bt = torch.as_tensor(beams, dtype=torch.float32, device=self.dev).reshape(-1, 4).contiguous()
        m = bt.shape[0]
        rec = torch.zeros((n, 12), dtype=torch.float32, device=self.dev)
        ri = rec.view(torch.int32)
        rec[:, 0:3], rec[:, 4:8] = p, q
        ri[:, 3] = self._ignore_bits(bodies)               # (None: 0xffffffff, the world frame)
        ri[:, 8] = self._ignore_bits(ignore_body)
        got = self.sense_records(rec, bt, any_hit=any_hit, mounted=bodies is not None, **{c: True for c in channels})
        out = {}
        if "t" in got:
            out["t"] = got["t"].reshape(n, m)
        for c in ("body", "tag"):
            if c in got:
                out[c] = (got[c].to(torch.int64) & 0xFFFFFFFF).reshape(n, m)
        if "hits" in got:
            raw = got["hits"]
            f, u = raw.view(torch.float32).reshape(n, m, 8), raw.view(torch.int32).reshape(n, m, 8).to(torch.int64) & 0xFFFFFFFF
            out.update(normal=f[:, :, 1:4], collider=u[:, :, 5], shape=u[:, :, 6], raw=raw.reshape(n, m, 32))
            out.setdefault("t", f[:, :, 0]); out.setdefault("body", u[:, :, 4]); out.setdefault("tag", u[:, :, 7])
        if synchronize:
            torch.cuda.current_stream(self.dev).synchronize()
        return out

    # ---- trigger events: what entered and what left each overlap volume (include/nudge_hip.h, "trigger events") ----
    def _hit_list(self, what, n, offsets, hits, capacity):
        """The nh_HitList of (offsets, hits, capacity): `offsets` an int32 device tensor of n + 1 words, `hits` None or capacity x 16 bytes."""
        if offsets.numel() * offsets.element_size() != 4 * (n + 1):
            raise ValueError(f"{what}: offsets holds {offsets.numel() * offsets.element_size()} bytes, {n} volumes need {4 * (n + 1)}")
        if hits is not None and hits.numel() * hits.element_size() < 16 * capacity:
            raise ValueError(f"{what}: hits holds {hits.numel() * hits.element_size()} bytes, capacity {capacity} needs {16 * capacity}")
        return HitList(offsets.data_ptr(), hits.data_ptr() if hits is not None and capacity else 0, capacity, 0)

    def overlap_bodies_records(self, n, src, offsets=None, hits=None, capacity=0):
        """nh_overlap_bodies: one record per distinct body of every present segment of the list `src` = (offsets, hits, capacity) that a list call of
        overlap_records / region_records wrote for n volumes (int32 offsets, 16-byte records, the capacity that call was given).  Returns (offsets,
        hits) as overlap_records does, under the same count-only and capacity rules.  Enqueued; nothing waits (but a capacity larger than any
        before grows the scratch)."""
        if offsets is None:
            offsets = self.torch.empty(n + 1, dtype=self.torch.int32, device=self.dev)
        a, b = self._hit_list("overlap_bodies_records (src)", n, *src), self._hit_list("overlap_bodies_records", n, offsets, hits, capacity)
        _check(self.L, self.L.nh_overlap_bodies(self.ctx, n, C.byref(a), C.byref(b), 0), "nh_overlap_bodies")
        return offsets, hits

    def overlap_events_records(self, n, prev, cur, entered=None, left=None, by_body=False):
        """nh_overlap_events on lists for n volumes, each (offsets, hits, capacity): `prev` (or None: the first frame) and `cur` as a list call or
        overlap_bodies_records wrote them, `entered` and `left` the outputs (None: count only, with new offsets).  Returns (entered offsets, left
        offsets).  Enqueued; nothing waits (but capacities larger than any before grow the scratch)."""
        torch = self.torch
        entered, left = (o if o is not None else (torch.empty(n + 1, dtype=torch.int32, device=self.dev), None, 0) for o in (entered, left))
        p = None if prev is None else self._hit_list("overlap_events_records (prev)", n, *prev)
        c, e, l = (self._hit_list(f"overlap_events_records ({k})", n, *v) for k, v in (("cur", cur), ("entered", entered), ("left", left)))
        _check(self.L, self.L.nh_overlap_events(self.ctx, n, C.byref(p) if p is not None else None, C.byref(c), C.byref(e), C.byref(l),
                                                NH_EVENTS_BY_BODY if by_body else 0), "nh_overlap_events")
        return entered[0], left[0]

    def overlap_events(self, prev, cur, by_body=False, capacity=None, synchronize=False):
        """What entered and what left each volume between two lists: `prev` and `cur` are the dicts overlap() / region() returned for the same n
        volumes on the last step and on this one (`prev` None: the first frame -- everything listed has entered).  by_body=True: one event per body,
        not per collider (overlap_bodies on both lists first).  A volume whose segment either list's capacity cut off gives no event.
        capacity=None: each output gets room for every record of its input -- nothing waits.  A capacity: both outputs list only the segments that
        fit it.  Returns dict(entered=..., left=...), each in overlap()'s layout: `entered` holds records of `cur`, `left` records of `prev`."""
        torch = self.torch
        n = cur["offsets"].numel() - 1
        if prev is not None and prev["offsets"].numel() != n + 1:
            raise ValueError(f"overlap_events: prev lists {prev['offsets'].numel() - 1} volumes, cur {n}")
        lists = []
        for d in (prev, cur):
            if d is None:
                lists.append(None)
                continue
            cap = d["raw"].shape[0]
            lst = (d["offsets"].to(torch.int32), d["raw"] if cap else None, cap)          # (int64 -> int32 keeps the low 32 bits: the marker too)
            if by_body and n:
                offsets = torch.empty(n + 1, dtype=torch.int32, device=self.dev)
                hits = torch.empty((cap, 16), dtype=torch.uint8, device=self.dev)
                self.overlap_bodies_records(n, lst, offsets=offsets, hits=hits if cap else None, capacity=cap)
                lst = (offsets, hits if cap else None, cap)
            lists.append(lst)
        out = []
        for src in lists:
            cap = (src[2] if src is not None else 0) if capacity is None else capacity
            out.append((torch.zeros(n + 1, dtype=torch.int32, device=self.dev), torch.empty((cap, 16), dtype=torch.uint8, device=self.dev), cap))
        left, entered = out
        if n:
            self.overlap_events_records(n, lists[0], lists[1], entered=(entered[0], entered[1] if entered[2] else None, entered[2]),
                                        left=(left[0], left[1] if left[2] else None, left[2]), by_body=by_body)
        r = dict(entered=self._list_dict(entered[0], entered[1], n, entered[2]), left=self._list_dict(left[0], left[1], n, left[2]))
        if synchronize:
            torch.cuda.current_stream(self.dev).synchronize()
        return r

    # ---- contact events: which body pairs touch, began and stopped touching (include/nudge_hip.h, "contact events") ----
    def _pair_list(self, what, count, pairs, capacity):
        """The nh_PairList of (count, pairs, capacity): `count` a device tensor of one 32-bit word, `pairs` None or at least capacity x 64 bytes."""
        if count.numel() * count.element_size() < 4:
            raise ValueError(f"{what}: count holds {count.numel() * count.element_size()} bytes, not a 32-bit word")
        if pairs is not None and pairs.numel() * pairs.element_size() < 64 * capacity:
            raise ValueError(f"{what}: pairs holds {pairs.numel() * pairs.element_size()} bytes, capacity {capacity} needs {64 * capacity}")
        return PairList(count.data_ptr(), pairs.data_ptr() if pairs is not None and capacity else 0, capacity, 0)

    def _pair_out(self, out, capacity=0):
        """`out` as given, or a new (count, pairs, capacity): a zero count word and capacity x 64 bytes (None where capacity is 0)."""
        if out is not None:
            return out
        torch = self.torch
        return (torch.zeros(1, dtype=torch.int32, device=self.dev),
                torch.empty((capacity, 64), dtype=torch.uint8, device=self.dev) if capacity else None, capacity)

    def contact_pairs_records(self, data, bodies, impulses=None, count=None, capacity=0, body_count=0, out=None):
        """nh_contact_pairs: one record per unordered body pair of a contact list of device tensors -- `data` 32-byte nh_Contact records, `bodies`
        (a, b) pairs, `impulses` 16-byte records or None (all zero), `count` a device word or None (`capacity` is the count).  `out` = (count, pairs,
        capacity): a device word, None or capacity x 64 bytes (E.CONTACT_PAIR), the capacity; None: count only, with a new word.  Returns `out`.
        Enqueued; nothing waits (but a capacity larger than any before grows the scratch)."""
        out = self._pair_out(out)
        lst = ContactList(data.data_ptr() if data is not None else 0, bodies.data_ptr() if bodies is not None else 0,
                          impulses.data_ptr() if impulses is not None else 0, count.data_ptr() if count is not None else 0, capacity, body_count)
        o = self._pair_list("contact_pairs_records", *out)
        _check(self.L, self.L.nh_contact_pairs(self.ctx, C.byref(lst), C.byref(o), 0), "nh_contact_pairs")
        return out

    def contact_events_records(self, prev, cur, began=None, ended=None):
        """nh_contact_events on pair lists, each (count, pairs, capacity): `prev` (or None: the first frame) and `cur` as contact_pairs_records /
        step_contact_pairs wrote them, `began` and `ended` the outputs (None: count only, with new words).  Returns (began, ended)."""
        began, ended = self._pair_out(began), self._pair_out(ended)
        p = None if prev is None else self._pair_list("contact_events_records (prev)", *prev)
        c, b, e = (self._pair_list(f"contact_events_records ({k})", *v) for k, v in (("cur", cur), ("began", began), ("ended", ended)))
        _check(self.L, self.L.nh_contact_events(self.ctx, C.byref(p) if p is not None else None, C.byref(c), C.byref(b), C.byref(e), 0), "nh_contact_events")
        return began, ended

    def step_contact_pairs(self, out=None, capacity=None, body_count=None):
        """nh_step_contact_pairs: the pair records of the world's own last step, with the solved impulses of its contact cache, without a download.
        `out` = (count, pairs, capacity) as in contact_pairs_records, or None: a new list of `capacity` records (None: room for one pair per
        contact the world can hold).  body_count=None: the world's.  Returns `out`.  Call it after step() or advance()."""
        out = self._pair_out(out, self.max_contacts if capacity is None else capacity)
        o = self._pair_list("step_contact_pairs", *out)
        _check(self.L, self.L.nh_step_contact_pairs(self.ctx, C.byref(self.contacts), C.byref(self.cache), self.bodies.count if body_count is None else body_count,
                                                    C.byref(o), 0), "nh_step_contact_pairs")
        return out

    def pair_records(self, lst):
        """The host's copy of a pair list (count, pairs, capacity): (true count, E.CONTACT_PAIR records -- none where the count exceeds the capacity).
        Waits for the stream."""
        n = int(lst[0].cpu().numpy().view(np.uint32)[0])
        if lst[1] is None or n > lst[2]:
            return n, np.zeros(0, dtype=CONTACT_PAIR)
        return n, np.frombuffer(lst[1].reshape(-1)[:64 * n].cpu().numpy().tobytes(), dtype=CONTACT_PAIR, count=n).copy()

    def contact_events(self, prev, cur, capacity=None, synchronize=False):
        """Which pairs began and which stopped touching between two pair lists: `prev` and `cur` are what step_contact_pairs / contact_pairs_records
        returned on the last step and on this one (`prev` None: the first frame -- every pair of `cur` has begun).  capacity=None: each output gets
        room for every record of its input -- nothing waits.  Returns dict(began=..., ended=...), each a (count, pairs, capacity) list: `began` holds
        records of `cur`, `ended` records of `prev` -- the values of the last step the pair touched.  Keep `cur` as the next frame's `prev`."""
        caps = [(src[2] if src is not None else 0) if capacity is None else capacity for src in (cur, prev)]
        began, ended = self.contact_events_records(prev, cur, began=self._pair_out(None, caps[0]), ended=self._pair_out(None, caps[1]))
        if synchronize:
            self.torch.cuda.current_stream(self.dev).synchronize()
        return dict(began=began, ended=ended)

    # ---- body impulses: push, blast and wake bodies on the device (include/nudge_hip.h, "body impulses") ----
    def _impulse_list(self, what, records, count, capacity):
        """The nh_ImpulseList of device tensors: `records` at least capacity x 32 bytes (E.BODY_IMPULSE) or None, `count` a device word or None."""
        if records is not None and records.numel() * records.element_size() < 32 * capacity:
            raise ValueError(f"{what}: records holds {records.numel() * records.element_size()} bytes, capacity {capacity} needs {32 * capacity}")
        return ImpulseList(records.data_ptr() if records is not None else 0, count.data_ptr() if count is not None else 0, capacity, 0)

    def impulse_sums_records(self, records, count=None, capacity=0, out=None, bodies=None):
        """nh_impulse_sums: one 32-byte E.IMPULSE_SUM record per distinct valid body of a list of E.BODY_IMPULSE records on the device, ascending by
        body.  `count` a device word or None (`capacity` is the count).  `out` = (count, sums, capacity): a device word, None or capacity x 32 bytes,
        the capacity; None: count only, with a new word.  `bodies`: another E.BodyData than the world's.  Returns `out`.  Enqueued; nothing waits
        (but a capacity larger than any before grows the scratch)."""
        torch = self.torch
        if out is None:
            out = (torch.zeros(1, dtype=torch.int32, device=self.dev), None, 0)
        if out[1] is not None and out[1].numel() * out[1].element_size() < 32 * out[2]:
            raise ValueError(f"impulse_sums_records: sums holds {out[1].numel() * out[1].element_size()} bytes, capacity {out[2]} needs {32 * out[2]}")
        lst = self._impulse_list("impulse_sums_records", records, count, capacity)
        o = ImpulseSumList(out[0].data_ptr(), out[1].data_ptr() if out[1] is not None and out[2] else 0, out[2], 0)
        _check(self.L, self.L.nh_impulse_sums(self.ctx, C.byref(self.bodies if bodies is None else bodies), C.byref(lst), C.byref(o), 0), "nh_impulse_sums")
        return out

    def body_impulses_records(self, records, count=None, capacity=0, wake=False):
        """nh_body_impulses: the list's impulses added to the bodies' momentum on the device; wake=True: NH_IMPULSE_WAKE.  Enqueued; nothing waits
        (but a capacity larger than any before grows the scratch)."""
        lst = self._impulse_list("body_impulses_records", records, count, capacity)
        _check(self.L, self.L.nh_body_impulses(self.ctx, C.byref(self.bodies), C.byref(lst), NH_IMPULSE_WAKE if wake else 0), "nh_body_impulses")

    def blast_impulses_records(self, blasts, n, src, out=None):
        """nh_blast_impulses: `blasts` n x 32 bytes (E.BLAST) on the device, `src` = (offsets, hits, capacity) a hit list for n volumes as
        overlap_records / overlap_wide_records / region_records / overlap_bodies_records wrote it; `out` capacity x 32 bytes or None: a new tensor
        filled with NH_IMPULSE_NO_BODY records (only the first min(offsets[n], capacity) are written).  Returns `out`."""
        torch = self.torch
        cap = src[2]
        if out is None:
            out = torch.zeros((max(cap, 1), 8), dtype=torch.int32, device=self.dev)
            out[:, 3] = -1
        elif out.numel() * out.element_size() < 32 * cap:
            raise ValueError(f"blast_impulses_records: out holds {out.numel() * out.element_size()} bytes, capacity {cap} needs {32 * cap}")
        if blasts.numel() * blasts.element_size() < 32 * n:
            raise ValueError(f"blast_impulses_records: blasts holds {blasts.numel() * blasts.element_size()} bytes, {n} blasts need {32 * n}")
        lst = self._hit_list("blast_impulses_records", n, *src)
        _check(self.L, self.L.nh_blast_impulses(self.ctx, C.byref(self.bodies), blasts.data_ptr(), n, C.byref(lst), out.data_ptr(), 0), "nh_blast_impulses")
        return out

    def touch_impulses_records(self, pushes, n, k, counts, touches, out=None):
        """nh_touch_impulses: `pushes` n x 16 bytes (E.PUSH), `counts` n words and `touches` n x k x 64 bytes as a *_touched_records call wrote them;
        `out` n x k x 32 bytes or None: a new tensor.  Returns `out`: record i * k + j is slot j of mover i, NH_IMPULSE_NO_BODY where nothing pushes."""
        torch = self.torch
        for name, t, size in (("pushes", pushes, 16 * n), ("counts", counts, 4 * n), ("touches", touches, 64 * n * k)):
            if t.numel() * t.element_size() < size:
                raise ValueError(f"touch_impulses_records: {name} holds {t.numel() * t.element_size()} bytes, not {size}")
        if out is None:
            out = torch.empty((max(n * k, 1), 32), dtype=torch.uint8, device=self.dev)
        elif out.numel() * out.element_size() < 32 * n * k:
            raise ValueError(f"touch_impulses_records: out holds {out.numel() * out.element_size()} bytes, not {32 * n * k}")
        _check(self.L, self.L.nh_touch_impulses(self.ctx, pushes.data_ptr(), n, k, counts.data_ptr(), touches.data_ptr(), out.data_ptr(), 0), "nh_touch_impulses")
        return out

    def body_impulses(self, bodies, impulses, points=None, wake=True):
        """Push bodies: `impulses` (n, 3) added to the momentum of `bodies` (n indices), at the world-space `points` (n, 3) or, with points=None, at
        the bodies' centres (no angular part).  Several records may name one body; they are summed in list order (header, "body impulses").
        wake=True: the bodies' idle counters are zeroed as well, so that a sleeper -- and with the next step its whole set -- wakes."""
        torch = self.torch
        b = torch.as_tensor(bodies, device=self.dev).reshape(-1).to(torch.int64)
        n = b.shape[0]
        if n == 0:
            return self.body_impulses_records(None, capacity=0, wake=wake)
        rec = torch.zeros((n, 8), dtype=torch.float32, device=self.dev)
        ri = rec.view(torch.int32)
        ri[:, 3] = (b & 0xFFFFFFFF).to(torch.int32)          # (int64 -> int32 keeps the low 32 bits)
        rec[:, 4:7] = torch.as_tensor(impulses, dtype=torch.float32, device=self.dev).reshape(-1, 3)
        if points is None:
            ri[:, 7] = NH_IMPULSE_AT_CENTRE
        else:
            rec[:, 0:3] = torch.as_tensor(points, dtype=torch.float32, device=self.dev).reshape(-1, 3)
        self.body_impulses_records(rec, capacity=n, wake=wake)

    def blast(self, centres, radii, strengths, falloff=1.0, wake=True):
        """Explosions: every body with a collider inside the sphere (centre, radius) gets an impulse away from the centre through its own centre, of
        strength * (1 - falloff * distance / radius) where that is positive -- overlap_wide, overlap_bodies, blast_impulses, body_impulses against
        the last query_build(), with nothing downloaded and nothing waited for: each list gets room for one record per collider of the world.
        `radii`, `strengths`, `falloff`: numbers or n values.  Returns the impulse records (a device tensor, NH_IMPULSE_NO_BODY where nothing was pushed)."""
        torch = self.torch
        q, n = self._overlap_queries("blast", centres, radii, None, None, None, None)
        cap = max(n * (self.colliders.boxes.count + self.colliders.spheres.count), 1)
        b = torch.zeros((n, 8), dtype=torch.float32, device=self.dev)
        b[:, 0:3], b[:, 3] = q[:, 0:3], q[:, 8]
        b[:, 4] = torch.as_tensor(strengths, dtype=torch.float32, device=self.dev).reshape(-1)
        b[:, 5] = torch.as_tensor(falloff, dtype=torch.float32, device=self.dev).reshape(-1)
        hits, per_body = (torch.empty((cap, 16), dtype=torch.uint8, device=self.dev) for _ in range(2))
        offsets, _ = self.overlap_wide_records(q, hits=hits, capacity=cap)
        body_offsets, _ = self.overlap_bodies_records(n, (offsets, hits, cap), hits=per_body, capacity=cap)
        out = self.blast_impulses_records(b, n, (body_offsets, per_body, cap))
        self.body_impulses_records(out, capacity=cap, wake=wake)
        return out

    # ---- fast bodies: sweep what travels far along its velocity, stop it at the hit (include/nudge_hip.h, "fast bodies") ----
    def _sweep_list(self, lst):
        cap = lst["capacity"]
        return SweepList(lst["counts"].data_ptr(), *[lst[c].data_ptr() if lst.get(c) is not None and cap else 0 for c in SWEEP_CHANNELS], cap, 0)

    def sweep_records(self, time_step, min_travel=0.5, core=0.5, capacity=0, counts=None, colliders=None, casts=None, hits=None):
        """nh_sweep against the last query_build() / query_refit().  `counts`: a device tensor of two int32 words, or None for a new one.  Each channel
        is None (not asked for, costs nothing), True (a new tensor of `capacity` records) or a device tensor of at least that many to write into:
        colliders int32, casts 64-byte records (E.BOX_CAST; a sphere's: E.CAPSULE_CAST), hits 32-byte E.RAY_HIT records.  Returns the list as a dict:
        counts, the channels given, capacity -- what sweep_limit_records takes.  Enqueued; nothing waits (a tree larger than any before grows the
        scratch)."""
        torch = self.torch
        new = dict(colliders=lambda: torch.empty(capacity, dtype=torch.int32, device=self.dev), casts=lambda: torch.empty((capacity, 64), dtype=torch.uint8, device=self.dev),
                   hits=lambda: torch.empty((capacity, 32), dtype=torch.uint8, device=self.dev))
        size = dict(colliders=4, casts=64, hits=32)
        lst = dict(counts=torch.zeros(2, dtype=torch.int32, device=self.dev) if counts is None else counts, capacity=int(capacity))
        for name, given in (("colliders", colliders), ("casts", casts), ("hits", hits)):
            if given is None or given is False:
                continue
            lst[name] = new[name]() if given is True else given
            if lst[name].numel() * lst[name].element_size() < capacity * size[name]:
                raise ValueError(f"sweep_records: {name} holds {lst[name].numel() * lst[name].element_size()} bytes, capacity {capacity} needs {capacity * size[name]}")
        sl, sp = self._sweep_list(lst), SweepParams(time_step, min_travel, core, 0)
        _check(self.L, self.L.nh_sweep(self.ctx, C.byref(self.bodies), C.byref(sp), C.byref(sl), 0), "nh_sweep")
        return lst

    def sweep_limit_records(self, lst, factors=None):
        """nh_sweep_limit on a list sweep_records filled with colliders and hits: every body's velocity scaled to where its earliest sweep hit.
        `factors`: None, True (a new float32 tensor of the list's capacity) or a device tensor of at least that many.  Returns `factors`.  Enqueued."""
        if factors is True:
            factors = self.torch.empty(max(lst["capacity"], 1), dtype=self.torch.float32, device=self.dev)
        if factors is not None and factors.numel() * factors.element_size() < 4 * lst["capacity"]:
            raise ValueError(f"sweep_limit_records: factors holds {factors.numel() * factors.element_size()} bytes, capacity {lst['capacity']} needs {4 * lst['capacity']}")
        sl = self._sweep_list(lst)
        _check(self.L, self.L.nh_sweep_limit(self.ctx, C.byref(self.bodies), C.byref(sl), C.c_void_p(factors.data_ptr() if factors is not None else 0), 0), "nh_sweep_limit")
        return factors

    def sweep(self, time_step=None, min_travel=0.5, core=0.5, capacity=None, limit=False, synchronize=False):
        """The tunnelling guard of one step: call after step() and query_refit().  Every collider whose body would carry it further than `min_travel`
        times its smallest half extent in `time_step` (None: the world's) is swept, its inner `core` share, along that travel; limit=True then cuts
        the velocity of every body whose sweep hits to where the earliest one hits.  capacity=None: room for every collider -- nothing waits.
        Returns a dict of device tensors: counts (2,) int64 (selected boxes, selected spheres; above `capacity` together: nothing else was written),
        colliders (capacity,) int64 combined indices, casts (capacity, 16) float32 words of the cast records, t (capacity,), normal (capacity, 3),
        body / collider / shape / tag (capacity,) int64 of the hit records, `raw` the (capacity, 32) records, and with limit=True `factors`
        (capacity,).  Only the first counts.sum() rows are written."""
        torch = self.torch
        cap = self.colliders.boxes.count + self.colliders.spheres.count if capacity is None else int(capacity)
        dt = self.params["time_step"] if time_step is None else time_step
        lst = self.sweep_records(dt, min_travel, core, capacity=cap, colliders=True, casts=True, hits=True) if cap else self.sweep_records(dt, min_travel, core)
        out = dict(counts=lst["counts"].to(torch.int64) & 0xFFFFFFFF)
        if cap:
            raw = lst["hits"]
            f, u = raw.view(torch.float32).reshape(cap, 8), raw.view(torch.int32).reshape(cap, 8).to(torch.int64) & 0xFFFFFFFF
            out.update(colliders=lst["colliders"].to(torch.int64) & 0xFFFFFFFF, casts=lst["casts"].view(torch.float32).reshape(cap, 16), t=f[:, 0], normal=f[:, 1:4],
                       body=u[:, 4], collider=u[:, 5], shape=u[:, 6], tag=u[:, 7], raw=raw)
        if limit:
            factors = self.sweep_limit_records(lst, factors=True)
            out["factors"] = factors[:cap]
        if synchronize:
            torch.cuda.current_stream(self.dev).synchronize()
        return out

    # ---- joints: ball, distance and hinge joints between the calls of the step (include/nudge_hip.h, "joints") ----
    def joints_prepare(self, joints, offsets=None, connect=True, baumgarte=0.2, max_bias=4.0, warm=1.0):
        """nh_joints_prepare for a list of E.JOINT records (numpy) and, optionally, its cut points (`offsets`: assemblies + 1 ascending words from 0 to
        len(joints)); call it when the list changes, not per step.  Uploads the list, zeroes the accumulated impulses (E.JOINT_IMPULSE, kept on the
        device in self.joint_impulses), keeps the plan, and with connect=True installs the joints' body pairs behind the scene's own connections
        (nh_joint_connections), so that an assembly sleeps and wakes as one set.  `baumgarte`, `max_bias`, `warm`: what joints_setup passes as
        nh_JointParams beside the world's time step.  Enqueued; joint_status() reads the four status words."""
        torch = self.torch
        j = np.ascontiguousarray(joints, dtype=JOINT).reshape(-1)
        n = len(j)

        def up(a, dtype, min_bytes=16):
            raw = np.ascontiguousarray(a, dtype=dtype).view(np.uint8).reshape(-1)
            t = torch.zeros(max(raw.size, min_bytes), dtype=torch.uint8, device=self.dev)
            if raw.size:
                t[:raw.size] = torch.from_numpy(raw.copy()).to(self.dev)
            return t

        jt = dict(joints=up(j, JOINT), n=n, impulses=torch.zeros(max(32 * n, 32), dtype=torch.uint8, device=self.dev),
                  status=torch.zeros(4, dtype=torch.int32, device=self.dev), levels=torch.zeros(max(n, 1), dtype=torch.int32, device=self.dev),
                  order=torch.zeros(max(n, 1), dtype=torch.int32, device=self.dev), offsets=None, assemblies=0)
        if offsets is not None:
            off = np.ascontiguousarray(offsets, dtype=np.uint32).reshape(-1)
            jt["offsets"], jt["assemblies"] = up(off, np.uint32), len(off) - 1
        jt["list"] = JointList(jt["joints"].data_ptr(), jt["offsets"].data_ptr() if jt["offsets"] is not None else 0, n, jt["assemblies"])
        jt["plan"] = JointPlan(jt["status"].data_ptr(), jt["levels"].data_ptr(), jt["order"].data_ptr(), n, 0)
        jt["params"] = dict(baumgarte=baumgarte, max_bias=max_bias, warm=warm)
        _check(self.L, self.L.nh_joints_prepare(self.ctx, self.bodies.count, C.byref(jt["list"]), C.byref(jt["plan"])), "nh_joints_prepare")
        self._joints = jt
        self.joint_impulses = jt["impulses"]
        if connect:
            base = self._keep.setdefault("cn_scene", self._keep["cn"])
            nbase = self._scene_connections = getattr(self, "_scene_connections", self.connections.count)
            con = torch.zeros(max(8 * (nbase + n), 16), dtype=torch.uint8, device=self.dev)
            con[:8 * nbase] = base[:8 * nbase]
            _check(self.L, self.L.nh_joint_connections(self.ctx, C.byref(jt["list"]), C.c_void_p(con.data_ptr() + 8 * nbase)), "nh_joint_connections")
            self._keep["cn"] = con
            self.connections = BodyConnections(con.data_ptr(), nbase + n)

    def joint_status(self):
        """(error bits, valid joints, highest level, non-empty bins) of the last joints_prepare; waits for the stream."""
        return tuple(int(x) & 0xFFFFFFFF for x in self._joints["status"].cpu().tolist())

    def joints_setup(self, time_step=None, baumgarte=None, max_bias=None, warm=None):
        """nh_joints_setup: after setup(), before the first apply().  Parameters default to joints_prepare's and the world's time step."""
        jt = self._joints
        p = jt["params"]
        jp = JointParams(self.params["time_step"] if time_step is None else time_step, p["baumgarte"] if baumgarte is None else baumgarte,
                         p["max_bias"] if max_bias is None else max_bias, p["warm"] if warm is None else warm)
        _check(self.L, self.L.nh_joints_setup(self.ctx, C.byref(self.active), C.byref(self.bodies), C.byref(jt["list"]), C.byref(jt["plan"]), C.byref(jp),
                                              C.c_void_p(jt["impulses"].data_ptr())), "nh_joints_setup")

    def joints_apply(self, iterations=1):
        """nh_joints_apply: `iterations` sweeps over the joints in one launch."""
        jt = self._joints
        _check(self.L, self.L.nh_joints_apply(self.ctx, C.byref(self.bodies), C.byref(jt["list"]), C.byref(jt["plan"]), C.c_void_p(jt["impulses"].data_ptr()),
                                              iterations), "nh_joints_apply")

    def step_joints(self, steps=1, iterations=None):
        """`steps` sub-steps of a jointed world through the call-by-call ABI: the eight calls of step()'s loop with joints_setup() behind setup() and
        apply(1), joints_apply(1) per iteration -- where the sample says custom constraint impulses go (example/main.cpp:313-317).  Not for worlds
        created with NH_FLAG_SINGLE_APPLY or NH_FLAG_FUSED_STEP (one contact apply per step)."""
        it = self.params["iterations"] if iterations is None else iterations
        for _ in range(steps):
            self.collide()
            self.gravity()
            self.read_cache()
            self.setup()
            self.joints_setup()
            for _i in range(it):
                self.apply(1)
                self.joints_apply(1)
            self.update()
            self.write_cache()
            self.advance()
            self.step_done()

    # ---- measurement ----
    def enable_timing(self, on=True, only=None):
        self.L.nh_set_timing_filter(self.ctx, only.encode() if only else None)
        self.L.nh_enable_timing(self.ctx, 1 if on else 0)

    def kernel_times(self, reset=True):
        buf = (KernelTime * 128)()
        n = self.L.nh_kernel_times(self.ctx, buf, 128, 1 if reset else 0)
        return {buf[i].name.decode(): (buf[i].ms, int(buf[i].launches)) for i in range(n)}
