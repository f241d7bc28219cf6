"""The batches of recover records the nh_recover tests share (tests/test_cpu_recover.py, tests/test_gpu_recover.py): spheres, oriented boxes, capsules and
capsules of half height 0 placed within their own size of a collider's surface, so that most start in overlap, a good share needs a second push because the
first lands them in a neighbour, some run out of iterations and some start free."""
import numpy as np

import hostrecover_util as HR
from query_util import unit_quats
from nudge_amd import engine as E

NONE = 0xFFFFFFFF
SKIN = 0.01
# the seeds of the GPU test's batches per small scene (before stepping, after stepping); tests/test_cpu_recover.py checks the share conditions on them
SEEDS = {"pile": (800, 810), "compound": (801, 811), "stacks": (802, 812), "grid_tiles": (803, 813), "ball_pit": (804, 814)}
# the conditions of a batch that a bit-for-bit comparison must not pass on idle lanes: (share with iterations >= 1, share with iterations >= 2)
PUSHED_ONCE, PUSHED_TWICE = 0.25, 0.02


def _rotate(q, v):
    """v rotated by the unit quaternions q = (x, y, z, s), in float64."""
    u, s = q[:, :3], q[:, 3:4]
    t = 2.0 * np.cross(u, v)
    return v + s * t + np.cross(u, t)


def recovers(rng, rec, nbox, n, skin=SKIN, scale=1.0, bodies=64, far_share=0.1, invalid=True):
    """n nh_Recover records around the colliders of `rec` with a finite pose.  Each picks a collider and a point of its surface (a box: a point of its
    faces, through its rotation; a sphere: a point at its radius) and stands within its own size of it -- the centre is that point plus a random
    offset of up to the shape's size; a `far_share` of them 1 - 3 sizes away, where most are free.  A third each are spheres (radius 0.1 - 0.6 x
    `scale`), boxes (half extents 0.1 - 0.6 each, random rotations) and capsules (radius 0.1 - 0.6, half height 0 - 0.8, a quarter exactly 0 with a NaN
    rotation, which is not read).  max_iterations from 0 .. 8, one in ten with skin 0, every fourth ignoring one of the first `bodies` bodies, and
    with `invalid` one in 64 invalid in one of seven ways."""
    p = rec["p"].astype(np.float64)
    live = np.nonzero(np.isfinite(p).all(axis=1))[0]
    at = rng.choice(live, size=n)
    h = rec["h"][at].astype(np.float64)
    u = rng.uniform(-1.0, 1.0, size=(n, 3))
    box = at < nbox
    u[box] /= np.abs(u[box]).max(axis=1, keepdims=True)                      # a point of the box's faces, in its frame
    u[~box] /= np.linalg.norm(u[~box], axis=1, keepdims=True)              # a point of the sphere (h = (R, R, R))
    surface = p[at] + _rotate(rec["q"][at].astype(np.float64), u * h)
    shape = rng.choice([E.NH_SHAPE_SPHERE, E.NH_SHAPE_BOX, E.NH_SHAPE_CAPSULE], size=n)
    size = rng.uniform(0.1, 0.6, size=(n, 3)) * scale
    size[shape == E.NH_SHAPE_CAPSULE, 1] = rng.uniform(0.0, 0.8, size=int((shape == E.NH_SHAPE_CAPSULE).sum())) * scale
    flat = (shape == E.NH_SHAPE_CAPSULE) & (rng.random(n) < 0.25)
    size[flat, 1] = 0.0
    extent = np.where(shape == E.NH_SHAPE_BOX, np.linalg.norm(size, axis=1), np.where(shape == E.NH_SHAPE_CAPSULE, size[:, 0] + size[:, 1], size[:, 0]))
    off = rng.normal(size=(n, 3))
    far = rng.random(n) < far_share
    off *= np.where(far, rng.uniform(1.0, 3.0, size=n), rng.uniform(0.0, 1.0, size=n))[:, None] * extent[:, None] / np.linalg.norm(off, axis=1, keepdims=True)
    m = np.zeros(n, dtype=E.RECOVER)
    m["center"], m["shape"], m["size"], m["rotation"] = surface + off, shape, size, unit_quats(rng, n)
    m["rotation"][::5] = HR.IDENTITY                                         # (axis-aligned against axis-aligned colliders: parallel edges)
    m["rotation"][flat] = np.nan
    m["skin"] = np.where(rng.random(n) < 0.1, 0.0, skin * scale)
    m["max_iterations"] = rng.integers(0, 9, size=n)
    m["ignore_body"] = NONE
    m["ignore_body"][::4] = rng.integers(0, bodies, size=len(m[::4]))
    if invalid:
        bad = rng.choice(np.nonzero(~flat)[0], size=max(1, n // 64), replace=False)
        for j, b in enumerate(bad):
            k = j % 7
            if k == 0:
                m["shape"][b] = 7
            elif k == 1:
                m["center"][b, 1] = np.nan
            elif k == 2:
                m["size"][b, 0] = -0.5
            elif k == 3:
                m["size"][b, 1], m["shape"][b] = np.inf, E.NH_SHAPE_BOX
            elif k == 4:
                m["rotation"][b, 0], m["shape"][b] = np.nan, E.NH_SHAPE_BOX
            elif k == 5:
                m["skin"][b] = (-0.01, np.nan, np.inf)[(j // 7) % 3]
            else:
                m["max_iterations"][b] = 9 + (j // 7) * 1000
    return m


def shares(results):
    """Of a batch's results: (share with iterations >= 1, share with iterations >= 2, how many ended OVERLAPPING, how many are free without a push)."""
    return (float((results["iterations"] >= 1).mean()), float((results["iterations"] >= 2).mean()),
            int(((results["flags"] & E.NH_RECOVER_OVERLAPPING) != 0).sum()), int(((results["flags"] == 0) & (results["iterations"] == 0)).sum()))


def shares_hold(results):
    once, twice, overlapping, free = shares(results)
    return once >= PUSHED_ONCE and twice >= PUSHED_TWICE and overlapping >= 1 and free >= 1
