"""The batches of box moves the nh_boxmove tests share (tests/test_cpu_boxmove.py, tests/test_gpu_boxmove.py): move_batches' origins, displacements,
rotations, slide counts and ignored bodies, with oriented boxes in place of the capsules."""
import numpy as np

from hostmover_util import BOX as HBM
import hostoverlap_util as HO
import move_batches as MB
from move_batches import shares      # noqa: F401

NONE = 0xFFFFFFFF
SKIN = MB.SKIN


def moves(rng, rec, nbox, n, skin=SKIN, scale=1.0, bodies=64, free_share=0.85, draw=4):
    """n nh_BoxMove records around the colliders of `rec` with a finite pose: move_batches._draw's origins (1 - 3 x `scale` from a collider's centre),
    displacements (0.5 - 4 x `scale`, aimed at one of the four nearest colliders), random rotations, max_slides from 0 .. 8 and ignored bodies, for
    boxes of half extents 0.1 - 0.6 (x `scale`) per axis; one in sixteen has one half extent exactly 0 (a plate) and one in thirty-two all three (a
    ray).  `draw` times as many are drawn, and those that start free of every collider (nh_overlap's box predicates on the host) are taken first, up
    to `free_share` of the batch: a move that starts in overlap never slides."""
    c = MB._draw(rng, rec, draw * n, skin, scale, bodies)
    size = rng.uniform(0.1, 0.6, size=(len(c), 3)) * scale
    plate = rng.random(len(c)) < 1.0 / 16
    size[plate, rng.integers(0, 3, size=int(plate.sum()))] = 0.0
    size[rng.random(len(c)) < 1.0 / 32] = 0.0
    cand = HBM.moves(c["origin"], c["displacement"], size, rotations=c["rotation"], skin=c["skin"], max_slides=c["max_slides"], ignore_body=c["ignore_body"])
    free = np.diff(HO.overlap(rec, nbox, HBM.overlap_queries(cand))[0].astype(np.int64)) == 0
    return MB.take_free(rng, cand, free, n, free_share)
