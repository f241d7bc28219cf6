"""The cast batches the first-k tests share (tests/test_cpu_castk.py, tests/test_gpu_castk.py): cast_util's mixed rays under each of the four shapes
-- sizes from 0 to several bodies, identity and random rotations, finite and infinite max_t, ignore_body, start overlaps, zero directions and invalid
records -- and the shares of a batch that keep a comparison at k from being empty."""
import numpy as np

from cast_util import box_casts, capsule_casts, k_rays as rays, sphere_casts

SHAPES = ("ray", "sphere", "box", "capsule")


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
