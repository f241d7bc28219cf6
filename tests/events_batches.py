"""The batches of overlap volumes the trigger-event tests share (tests/test_cpu_events.py, tests/test_gpu_events.py): sphere and box volumes around a
world's colliders at positions A and at A + shift, so that between the two lists a good share of the volumes sees a collider enter, a good share sees
one leave, and some see both.  tests/test_cpu_events.py asserts those shares on the host overlap oracle with the GPU tests' seeds, so that a byte
comparison of event lists cannot pass on empty ones."""
import numpy as np

import hostlib
from query_util import unit_quats
from nudge_amd import engine as E

NONE = 0xFFFFFFFF
COUNT = 2048
# the seed of each small world's batch
SEEDS = {"pile": 900, "compound": 901, "stacks": 902, "grid_tiles": 903, "ball_pit": 904}
# how far each volume moves between the two lists, in a direction of its own: from one body's size up, until the conditions below hold
SHIFT = {"pile": 2.0, "compound": 1.0, "stacks": 1.0, "grid_tiles": 1.0, "ball_pit": 1.0}
# the size of the volumes (1: about a body's): larger where the bodies stand apart, so that a volume holds more than the ground
SCALE = {"pile": 2.0, "compound": 1.0, "stacks": 2.0, "grid_tiles": 2.0, "ball_pit": 1.0}
# the conditions (shares of the volumes): an entry, an exit, both; on `compound`, the share of non-empty segments that hold a body twice
ENTERED, LEFT, BOTH, COMPOUND = 0.25, 0.25, 0.10, 0.10


def initial_records(scene):
    """The collider records of a scene before its first step."""
    return hostlib.records(scene["body_transforms"], scene)


def volumes(rng, rec, n=COUNT, scale=1.0):
    """n nh_OverlapQuery records: spheres (even indices, radius 0.5 .. 1.5 x scale) and oriented boxes (odd ones, half extents 0.4 .. 1.2 x scale each),
    three in four centred within a body's size of a collider, the others anywhere in the colliders' bounds; every 16th ignores the body of the
    collider it stands on."""
    live = np.nonzero(np.isfinite(rec["p"]).all(axis=1))[0]
    p = rec["p"][live].astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    at = rng.choice(live, size=n)
    q = np.zeros(n, dtype=E.OVERLAP_QUERY)
    near = rng.random(n) < 0.75
    q["center"] = np.where(near[:, None], rec["p"][at].astype(np.float64) + rng.normal(scale=0.5 * scale, size=(n, 3)), rng.uniform(lo, hi, size=(n, 3)))
    q["shape"] = np.where(np.arange(n) % 2 == 0, E.NH_SHAPE_SPHERE, E.NH_SHAPE_BOX)
    q["size"] = rng.uniform(0.4, 1.2, size=(n, 3)) * scale
    q["size"][::2, 0] = rng.uniform(0.5, 1.5, size=len(q[::2])) * scale
    q["rotation"] = unit_quats(rng, n)
    q["ignore_body"] = NONE
    q["ignore_body"][::16] = rec["body"][at[::16]]
    return q


def shifted(rng, q, shift):
    """The volumes moved by `shift` each, in random directions."""
    d = rng.normal(size=(len(q), 3))
    out = q.copy()
    out["center"] = (q["center"].astype(np.float64) + shift * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return out


def batch(name, rec):
    """(volumes at A, volumes at A + shift) of the small world `name` whose colliders stand at `rec`."""
    rng = np.random.default_rng(SEEDS[name])
    a = volumes(rng, rec, scale=SCALE[name])
    return a, shifted(rng, a, SHIFT[name])


def shares(entered_offsets, left_offsets):
    """(share of volumes with an entry, with an exit, with both) of two event offsets arrays."""
    e, l = np.diff(entered_offsets.astype(np.int64)) > 0, np.diff(left_offsets.astype(np.int64)) > 0
    return float(e.mean()), float(l.mean()), float((e & l).mean())
