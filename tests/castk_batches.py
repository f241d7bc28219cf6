"""The cast batches the first-k tests share (tests/test_cpu_castk.py, tests/test_gpu_castk.py): the mixed rays of tests/test_gpu_castall.py under each
of the four shapes -- sizes from 0 to several bodies, identity and random rotations, finite and infinite max_t, ignore_body, start overlaps, zero
directions and invalid records -- and the shares of a batch that keep a comparison at k from being empty."""
import numpy as np

from query_util import bounds
from test_cpu_castall_shapes import box_casts, capsule_casts
from test_gpu_castall import _mixed
from nudge_amd import engine as E

SHAPES = ("ray", "sphere", "box", "capsule")
RADII = np.float32([0.0, 0.05, 0.75, 0.3])


def sphere_casts(rays, radii=RADII, invalid=True):
    """nh_SphereCast records on the rays' heads: the radii in turn, and a few invalid ones."""
    c = np.zeros(len(rays), dtype=E.SPHERE_CAST)
    for k in ("origin", "max_t", "direction", "ignore_body"):
        c[k] = rays[k]
    c["radius"] = radii[np.arange(len(rays)) % len(radii)]
    if invalid:
        c["radius"][10::97], c["radius"][11::97], c["radius"][12::97], c["radius"][13::97] = -0.5, np.nan, np.inf, -0.0
    return c


def rays(rng, n, rec):
    """test_gpu_castall's mixed rays, every fourth of them turned straight down through the centre of a collider (a little off): random rays through
    a sparse world seldom pierce more than three colliders, a ray down a stack or through a compound body does.  The heads keep their max_t and
    ignore_body."""
    lo, hi = bounds(rec)
    r = _mixed(rng, n, rec, lo, hi)
    live = np.nonzero(np.isfinite(rec["p"]).all(axis=1))[0]
    down = np.nonzero((np.arange(n) % 4 == 3) & np.isfinite(r["origin"]).all(axis=1) & np.isfinite(r["direction"]).all(axis=1) & r["direction"].any(axis=1))[0]
    r["origin"][down] = rec["p"][rng.choice(live, size=len(down))] + rng.normal(scale=0.05, size=(len(down), 3)).astype(np.float32)
    r["origin"][down, 1] = hi[1] + 5.0
    r["direction"][down] = (0.0, -1.0, 0.0)
    # ... and every fourth cut short, to a few body sizes or to a twentieth of the world, where a long cast through a pile would list many: rows
    # that hits and misses share
    span = float(np.linalg.norm(hi - lo))
    for phase, reach in ((1, 2.0), (5, 0.05 * span)):
        short = np.nonzero((np.arange(n) % 8 == phase) & ~np.isnan(r["max_t"]))[0]
        r["max_t"][short] = rng.uniform(0.0, reach, size=len(short))
    return r


def batches(rng, n, rec):
    """{shape: n casts} around the colliders of `rec`."""
    return {"ray": rays(rng, n, rec), "sphere": sphere_casts(rays(rng, n, rec)),
            "box": box_casts(rng, rays(rng, n, rec)), "capsule": capsule_casts(rng, rays(rng, n, rec))}


def shares(offsets, k):
    """Of a batch's all-hits offsets: the shares of casts that list more than k, between 1 and k - 1, and nothing."""
    size = np.diff(offsets.astype(np.int64))
    return float((size > k).mean()), float(((size > 0) & (size < k)).mean()), float((size == 0).mean())


def assert_not_empty(offsets, what):
    """At k = 3: at least 10 % of the casts evict (|S| > k), at least 10 % share a row between hits and misses (0 < |S| < k), some list nothing.
    Where thin shapes pierce too little of a sparse world for the first share at k = 3 (rays through the compound bodies), the k is 2, which the
    tests run as well: the shares are the same.  Returns the k."""
    seen = []
    for k in (3, 2):
        more, fewer, none = shares(offsets, k)
        if more >= 0.10 and fewer >= 0.10 and none > 0.0:
            return k
        seen.append((k, more, fewer, none))
    raise AssertionError((what, seen))
