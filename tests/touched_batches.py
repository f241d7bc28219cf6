"""The batches the touched movers' tests share (tests/test_cpu_touched.py, tests/test_gpu_touched.py): the generators AND the seeds of the plain movers'
tests, per shape, so that the shares those tests hold of a batch (slides, STEPPED, GROUNDED) bound the touches of the same batch from below, and what the
CPU file asserts of a batch holds for the batch the GPU file runs."""
import numpy as np

import boxmove_batches as BMB
import boxwalk_batches as BWB
import hosttouch_util as HT
import move_batches as MB
import walk_batches as WB
from query_util import SMALL
from test_cpu_boxmove import BATCH_SEED as BOX_MOVE_SEED, DRAW
from test_cpu_boxwalk import TERRAIN_SEED as BOX_TERRAIN_SEED
from test_cpu_walk import TERRAIN_SEED

MOVE_SEED = 700                          # tests/test_gpu_move.py's batches on SMALL: 700 + the world's place among the sorted names
SHAPES = dict(capsule=HT.CAPSULE, box=HT.BOX)


def world_moves(shape, name, rec, nbox, n=4096, seed=0):
    """n move records of `shape` ("capsule", "box") on the world `name` of SMALL whose colliders stand as `rec`: the batch of test_gpu_move /
    test_gpu_boxmove on that world as built (`seed` 0), or another draw of the same generator."""
    at = sorted(SMALL).index(name) + seed
    if shape == "box":
        return BMB.moves(np.random.default_rng(BOX_MOVE_SEED + at), rec, nbox, n, draw=DRAW.get(name, 4))
    return MB.moves(np.random.default_rng(MOVE_SEED + at), rec, nbox, n)


def terrain_walks(shape, n=2048, seed=0):
    """n walk records of `shape` on walk_batches.terrain(): the batch of test_cpu_walk / test_cpu_boxwalk (`seed` 0), or another draw."""
    if shape == "box":
        return BWB.terrain_walks(np.random.default_rng(BOX_TERRAIN_SEED + seed), n)
    return WB.terrain_walks(np.random.default_rng(TERRAIN_SEED + seed), n)


def phases(counts, touches):
    """Per record: how many different phases its written touches have."""
    w = HT.written(counts, touches.shape[1])
    return sum(((touches["phase"] == p) & w).any(axis=1).astype(np.int64) for p in range(5))
