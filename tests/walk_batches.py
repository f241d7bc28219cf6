"""The scene and the batches of walks the nh_walk tests share (tests/test_cpu_walk.py, tests/test_gpu_walk.py): a small static terrain with one lane per
rule -- stairs, a high riser, three ramps, a ledge, a drop, a low ceiling over a step -- and capsules that stand one skin above walkable tops and are sent
horizontally, on the terrain and on the worlds of query_util.SMALL."""
import numpy as np

import hostcapsule_util as HC
import hostmover_util as HV
import move_batches as MB
from hostmover_util import CAPSULE as HW
from nudge_amd import engine as E
from nudge_amd import scenes as S

SKIN = 0.01
# what the generators draw from
STEP_HEIGHTS = (0.0, 0.4, 1.0, 2.2)
SNAPS = (0.0, 0.3)
LIMITS = (0.0, 30.0, 45.0, 50.0)
# the lanes of terrain(): z of the centre line; every feature starts at x = 2 and the floor's top is y = 0
LANE = dict(stairs=-20.0, riser=-15.0, ramp20=-10.0, ramp40=-5.0, ramp60=0.0, ledge=5.0, drop=10.0, ceiling=15.0, open=20.0)
RAMP_LENGTH, RAMP_THICK, LANE_HALF = 3.0, 0.1, 1.5
CEILING = 1.55          # the underside of the low ceiling: a capsule of r 0.25, hh 0.5 (1.5 tall) stands under it and cannot rise by a 0.3 step


def _ramp(angle, z):
    """(centre, half extents, rotation) of a slab whose top face rises from (x, y) = (2, 0) at `angle` degrees."""
    a = np.deg2rad(angle)
    c = np.array([2.0, 0.0]) + RAMP_LENGTH * np.array([np.cos(a), np.sin(a)]) - RAMP_THICK * np.array([-np.sin(a), np.cos(a)])
    return (c[0], c[1], z), (RAMP_LENGTH, RAMP_THICK, LANE_HALF), (0.0, 0.0, np.sin(a / 2), np.cos(a / 2))


def terrain():
    """The scene: 15 static boxes on body 0 (and one dynamic box far above, which nothing here steps)."""
    I = (0.0, 0.0, 0.0, 1.0)
    boxes = [((0.0, -0.5, 0.0), (60.0, 0.5, 60.0), I)]                                                    # the floor, top at y = 0
    for k in range(1, 6):                                                                                 # five stairs, risers of 0.3, treads of 1
        boxes.append((((1.0 + k + 8.0) / 2, 0.15 * k, LANE["stairs"]), ((8.0 - (1.0 + k)) / 2, 0.15 * k, LANE_HALF), I))
    boxes.append(((4.0, 0.4, LANE["riser"]), (2.0, 0.4, LANE_HALF), I))                                   # a riser of 0.8
    for angle in (20, 40, 60):
        boxes.append(_ramp(angle, LANE["ramp%d" % angle]))
    boxes.append(((-2.0, 0.1, LANE["ledge"]), (4.0, 0.1, LANE_HALF), I))                                  # a platform 0.2 high that ends at x = 2
    boxes.append(((-2.0, 1.0, LANE["drop"]), (4.0, 1.0, LANE_HALF), I))                                   # one 2 high
    boxes.append(((4.0, 0.15, LANE["ceiling"]), (2.0, 0.15, LANE_HALF), I))                               # a step of 0.3 ...
    boxes.append(((2.0, CEILING + 0.25, LANE["ceiling"]), (4.0, 0.25, LANE_HALF), I))                     # ... under a low ceiling
    st = S._identity_transforms(len(boxes))
    ssz = np.zeros((len(boxes), 3), dtype=np.float32)
    for k, (c, h, q) in enumerate(boxes):
        st["position"][k], st["rotation"][k], ssz[k] = c, q, h
    bt = S._identity_transforms(1)
    bt["position"][0] = (0.0, 500.0, 0.0)
    one = np.ones(1, dtype=np.float32)
    empty = S._identity_transforms(0)
    return S._assemble((st, ssz), (bt, np.ones((1, 3), dtype=np.float32), S._box_properties(one, one, one)),
                       (empty, np.zeros(0, np.float32), S._sphere_properties(np.zeros(0, np.float32))), dict(S.DEFAULT_PARAMS), name="terrain")


def stand(x, top, z, radius, half_height, skin=SKIN):
    """The centres ((n, 3)) of upright capsules that stand one skin above a top at height `top`."""
    return np.stack(np.broadcast_arrays(x, top + skin + radius + half_height, z), axis=-1).astype(np.float32).reshape(-1, 3)


def _draw_rules(rng, w, probe_share=0.1, snap_share=0.9):
    n = len(w)
    w["step_height"] = rng.choice(STEP_HEIGHTS, n)
    w["snap_distance"] = np.where(rng.random(n) < snap_share, SNAPS[1], SNAPS[0])
    w["min_ground_up"] = HV.cos_deg(rng.choice(LIMITS, n))
    w["options"] = (rng.random(n) < probe_share).astype(np.uint32) * E.NH_WALK_PROBE_ONLY
    w["max_slides"] = rng.integers(0, 9, n)
    return w


def terrain_walks(rng, n):
    """n nh_Walk records on terrain(): upright capsules (r 0.2 - 0.3, half height 0, 0.3 or 0.5) one skin above the floor in front of a lane's feature, on
    a stair's tread or near the end of a platform, sent 0.5 - 3 units along x (a tenth the other way) with a little z, a third of them with a
    downward component; step heights, snap distances, slope limits, slide counts and PROBE_ONLY drawn as the module's constants say."""
    lanes = ["stairs"] * 4 + ["riser"] * 2 + ["ramp20"] * 2 + ["ramp40"] * 2 + ["ramp60"] * 3 + ["ledge"] * 3 + ["drop"] * 4 + ["ceiling", "open"]
    lane = rng.choice(lanes, n)
    z = np.array([LANE[k] for k in lane]) + rng.uniform(-1.0, 1.0, n)
    x = rng.uniform(0.0, 1.6, n)
    top = np.zeros(n)
    tread = rng.integers(0, 4, n)                                          # (0: the floor in front of the stairs)
    on_stairs = (lane == "stairs") & (tread > 0)
    x = np.where(on_stairs, 2.0 + (tread - 1) + rng.uniform(0.35, 0.65, n), x)
    top = np.where(on_stairs, 0.3 * tread, top)
    top = np.where(lane == "ledge", 0.2, np.where(lane == "drop", 2.0, top))
    x = np.where(lane == "drop", rng.uniform(0.8, 1.8, n), x)
    r = rng.choice([0.2, 0.25, 0.3], n)
    hh = rng.choice([0.0, 0.3, 0.5], n)
    r = np.where(lane == "ceiling", 0.25, r)
    hh = np.where(lane == "ceiling", 0.5, hh)
    d = np.zeros((n, 3))
    d[:, 0] = rng.uniform(0.5, 3.0, n) * np.where(rng.random(n) < 0.1, -1.0, 1.0)
    d[:, 2] = rng.uniform(-0.2, 0.2, n)
    d[:, 1] = np.where(rng.random(n) < 0.33, -rng.uniform(0.05, 0.3, n), 0.0)
    w = HW.walks(stand(x, top, z, r, hh), d, r, hh, skin=SKIN)
    return _draw_rules(rng, w, snap_share=0.96)


def _tops(rec, nbox):
    """The height of the highest point of every collider: p.y + the y extent of its box, or its radius."""
    q = rec["q"].astype(np.float64)
    x, y, z, s = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    row = np.stack([2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)], axis=1)          # the y row of the rotation matrix
    box = (np.abs(row) * rec["h"].astype(np.float64)).sum(axis=1)
    return rec["p"][:, 1].astype(np.float64) + np.where(np.arange(len(rec)) < nbox, box, rec["h"][:, 0])


def world_walks(rng, rec, nbox, n, slab_share=0.7, free_share=0.9):
    """n nh_Walk records on a world of query_util.SMALL: upright capsules (r 0.15 - 0.4, half height 0 - 0.5, a fifth exactly 0) that stand one skin above the
    ground slab (collider 0) within 2 units of a body, or above the top of a body, and are sent 0.3 - 2.5 units horizontally (of those on the slab nine
    in ten towards their body), a third with a downward component.  Four times as many are drawn and those that start free of every collider are taken first, up to `free_share` of the batch."""
    m = 4 * n
    p = rec["p"].astype(np.float64)
    live = np.nonzero(np.isfinite(p).all(axis=1))[0]
    live = live[live != 0]
    tops = _tops(rec, nbox)
    at = rng.choice(live, size=m)
    on_slab = rng.random(m) < slab_share
    r = rng.uniform(0.15, 0.4, m)
    hh = rng.uniform(0.0, 0.5, m)
    hh[rng.random(m) < 0.2] = 0.0
    reach = np.where(on_slab, 2.0, 0.3)
    x = p[at, 0] + rng.uniform(-1.0, 1.0, m) * reach
    z = p[at, 2] + rng.uniform(-1.0, 1.0, m) * reach
    top = np.where(on_slab, tops[0], tops[at])
    ang = rng.uniform(0.0, 2 * np.pi, m)
    aimed = on_slab & (rng.random(m) < 0.9)                                # most of those on the slab walk towards their body
    ang = np.where(aimed, np.arctan2(p[at, 2] - z, p[at, 0] - x), ang)
    length = rng.uniform(0.3, 2.5, m)
    d = np.stack([np.cos(ang) * length, np.where(rng.random(m) < 0.33, -rng.uniform(0.05, 0.3, m), 0.0), np.sin(ang) * length], axis=1)
    cand = _draw_rules(rng, HW.walks(stand(x, top, z, r, hh), d, r, hh, skin=SKIN))
    free = np.diff(HC.overlap(rec, nbox, HW.overlap_queries(cand))[0].astype(np.int64)) == 0
    return MB.take_free(rng, cand, free, n, free_share)
