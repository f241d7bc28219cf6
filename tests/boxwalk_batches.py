"""The batches of box walks the nh_boxwalk tests share (tests/test_cpu_boxwalk.py, tests/test_gpu_boxwalk.py): walk_batches' terrain and rules, with
boxes that stand one skin above walkable tops on their bottom faces -- axis-aligned, or turned about `up` -- and are sent horizontally."""
import numpy as np

import move_batches as MB
from hostmover_util import BOX as HBW
import hostoverlap_util as HO
import walk_batches as WB
from walk_batches import LANE, SKIN, terrain      # noqa: F401

NONE = 0xFFFFFFFF
BOX = (0.25, 0.75, 0.25)          # the upright box of the hand-built answers: 1.5 tall, as walk_batches' capsule under the low ceiling


def stand(x, top, z, hy, skin=SKIN):
    """The centres ((n, 3)) of boxes of half height `hy` that stand one skin above a top at height `top`."""
    return np.stack(np.broadcast_arrays(x, top + skin + hy, z), axis=-1).astype(np.float32).reshape(-1, 3)


def _yaw(rng, n, share):
    """Identity rotations, a `share` of them turned about y by a random angle."""
    a = np.where(rng.random(n) < share, rng.uniform(0.0, 2 * np.pi, n), 0.0)
    q = np.zeros((n, 4), dtype=np.float32)
    q[:, 1], q[:, 3] = np.sin(a / 2), np.cos(a / 2)
    return q


def terrain_walks(rng, n):
    """n nh_BoxWalk records on terrain(): boxes (half width 0.2 - 0.3, half height 0.25 - 0.75, a third turned about y) one skin above the floor in
    front of a lane's feature, on a stair's tread or near the end of a platform, sent 0.5 - 3 units along x (a tenth the other way) with a little z, a
    third of them with a downward component; the rules drawn as walk_batches draws them."""
    lanes = ["stairs"] * 4 + ["riser"] * 2 + ["ramp20"] * 2 + ["ramp40"] * 2 + ["ramp60"] * 3 + ["ledge"] * 3 + ["drop"] * 4 + ["ceiling", "open"]
    lane = rng.choice(lanes, n)
    z = np.array([LANE[k] for k in lane]) + rng.uniform(-1.0, 1.0, n)
    x = rng.uniform(0.0, 1.5, n)
    top = np.zeros(n)
    tread = rng.integers(0, 4, n)                                          # (0: the floor in front of the stairs)
    on_stairs = (lane == "stairs") & (tread > 0)
    x = np.where(on_stairs, 2.0 + (tread - 1) + rng.uniform(0.45, 0.55, n), x)
    top = np.where(on_stairs, 0.3 * tread, top)
    top = np.where(lane == "ledge", 0.2, np.where(lane == "drop", 2.0, top))
    x = np.where(lane == "drop", rng.uniform(0.8, 1.8, n), x)
    hw = rng.choice([0.2, 0.25, 0.3], n)
    hy = rng.choice([0.25, 0.5, 0.75], n)
    hw = np.where(lane == "ceiling", BOX[0], hw)
    hy = np.where(lane == "ceiling", BOX[1], hy)
    d = np.zeros((n, 3))
    d[:, 0] = rng.uniform(0.5, 3.0, n) * np.where(rng.random(n) < 0.1, -1.0, 1.0)
    d[:, 2] = rng.uniform(-0.2, 0.2, n)
    d[:, 1] = np.where(rng.random(n) < 0.33, -rng.uniform(0.05, 0.3, n), 0.0)
    w = HBW.walks(stand(x, top, z, hy), d, np.stack([hw, hy, hw], axis=1), rotations=_yaw(rng, n, 1.0 / 3), skin=SKIN)
    return WB._draw_rules(rng, w, snap_share=0.96)


def world_walks(rng, rec, nbox, n, slab_share=0.7, free_share=0.9):
    """n nh_BoxWalk records on a world of query_util.SMALL, placed and sent as walk_batches.world_walks places its capsules: boxes (half width
    0.15 - 0.4, half height 0.15 - 0.9, a third turned about y) one skin above the ground slab within 2 units of a body, or above the top of a body.
    Four times as many are drawn and those that start free of every collider (the box predicates of nh_overlap) are taken first, up to `free_share`."""
    m = 4 * n
    p = rec["p"].astype(np.float64)
    live = np.nonzero(np.isfinite(p).all(axis=1))[0]
    live = live[live != 0]
    tops = WB._tops(rec, nbox)
    at = rng.choice(live, size=m)
    on_slab = rng.random(m) < slab_share
    hw = rng.uniform(0.15, 0.4, m)
    hy = rng.uniform(0.15, 0.9, m)
    reach = np.where(on_slab, 2.0, 0.3)
    x = p[at, 0] + rng.uniform(-1.0, 1.0, m) * reach
    z = p[at, 2] + rng.uniform(-1.0, 1.0, m) * reach
    top = np.where(on_slab, tops[0], tops[at])
    ang = rng.uniform(0.0, 2 * np.pi, m)
    aimed = on_slab & (rng.random(m) < 0.9)                                # most of those on the slab walk towards their body
    ang = np.where(aimed, np.arctan2(p[at, 2] - z, p[at, 0] - x), ang)
    length = rng.uniform(0.3, 2.5, m)
    d = np.stack([np.cos(ang) * length, np.where(rng.random(m) < 0.33, -rng.uniform(0.05, 0.3, m), 0.0), np.sin(ang) * length], axis=1)
    cand = WB._draw_rules(rng, HBW.walks(stand(x, top, z, hy), d, np.stack([hw, hy, hw], axis=1), rotations=_yaw(rng, m, 1.0 / 3), skin=SKIN))
    free = np.diff(HO.overlap(rec, nbox, HBW.overlap_queries(cand))[0].astype(np.int64)) == 0
    return MB.take_free(rng, cand, free, n, free_share)
