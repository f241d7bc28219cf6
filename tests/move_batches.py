"""The batches of moves the nh_move tests share (tests/test_gpu_move.py): capsules that start 1 - 3 units from a collider's centre and are sent 0.5 - 4
units towards one of the colliders nearest to them, so that a good share slides once and some slide from one collider onto the next."""
import numpy as np

import hostcapsule_util as HC
from hostmover_util import CAPSULE as HM
from query_util import unit_quats

SKIN = 0.01


def moves(rng, rec, nbox, n, skin=SKIN, scale=1.0, bodies=64, free_share=0.85):
    """n nh_Move records around the colliders of `rec` with a finite pose: origins at collider centres plus offsets of 1 - 3 (x `scale`) units,
    displacements 0.5 - 4 (x `scale`) long aimed, with some scatter, at one of the four colliders nearest to the origin, radius 0.1 - 0.6 and half height
    0 - 0.8 (x `scale`; a fifth exactly 0: balls), random rotations, max_slides from 0 .. 8, and every third move ignoring one of the first `bodies`
    bodies.  Four times as many are drawn, and those that start free of every collider (nh_overlap's capsule predicates on the host) are taken first, up
    to `free_share` of the batch: in a packed scene most random starts are inside something, and a move that starts in overlap never slides."""
    cand = _draw(rng, rec, 4 * n, skin, scale, bodies)
    free = np.diff(HC.overlap(rec, nbox, HM.overlap_queries(cand))[0].astype(np.int64)) == 0
    return take_free(rng, cand, free, n, free_share)


def take_free(rng, cand, free, n, free_share):
    """n of the candidates `cand` in a shuffled order: those that start free first, up to `free_share` of the n, then the others."""
    first = np.nonzero(free)[0][:int(free_share * n)]
    rest = np.setdiff1d(np.arange(len(cand)), first)[:n - len(first)]
    pick = np.concatenate([first, rest])
    rng.shuffle(pick)
    return cand[pick]


def _draw(rng, rec, n, skin, scale, bodies):
    p = rec["p"].astype(np.float64)
    live = np.nonzero(np.isfinite(p).all(axis=1))[0]
    at = rng.choice(live, size=n)
    off = rng.normal(size=(n, 3))
    off *= rng.uniform(1.0, 3.0, size=(n, 1)) * scale / np.linalg.norm(off, axis=1, keepdims=True)
    o = (p[at] + off).astype(np.float32)
    # the four nearest centres of each origin (its own collider's among them), in chunks that keep the distance matrix small
    near = np.zeros((n, 4), dtype=np.int64)
    k = min(4, len(live))
    for lo in range(0, n, 1024):
        d2 = ((o[lo:lo + 1024, None, :].astype(np.float64) - p[live][None, :, :]) ** 2).sum(axis=2)
        near[lo:lo + 1024, :k] = live[np.argsort(d2, axis=1)[:, :k]]
        near[lo:lo + 1024, k:] = near[lo:lo + 1024, :1]
    aim = p[near[np.arange(n), rng.integers(0, 4, size=n)]] + rng.normal(size=(n, 3)) * 0.3 * scale - o
    aim /= np.maximum(np.linalg.norm(aim, axis=1, keepdims=True), 1e-9 * scale)
    d = (aim * rng.uniform(0.5, 4.0, size=(n, 1)) * scale).astype(np.float32)
    hh = rng.uniform(0.0, 0.8, size=n) * scale
    hh[rng.random(n) < 0.2] = 0.0
    m = HM.moves(o, d, rng.uniform(0.1, 0.6, size=n) * scale, hh, rotations=unit_quats(rng, n), skin=skin * scale, max_slides=rng.integers(0, 9, size=n))
    m["ignore_body"][::3] = rng.integers(0, bodies, size=len(m[::3]))
    return m


def shares(results):
    """(share with slides >= 1, share with slides >= 2) of a batch's results."""
    return float((results["slides"] >= 1).mean()), float((results["slides"] >= 2).mean())
