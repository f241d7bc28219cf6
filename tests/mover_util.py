"""The plumbing the mover tests share (tests/test_{cpu,gpu}_{move,boxmove,walk,boxwalk}.py): the GPU calls on numpy records, the byte comparison of
result records, a world's collider records, the terrain world, and the miss record."""
import numpy as np

import walk_batches as WB
from query_util import FUSED, NONE, records, upload      # noqa: F401
from nudge_amd import engine as E

SENTINEL = 0xA5


def _call(name, result):
    def call(w, records):
        raw = getattr(w, name + "_records")(upload(w, records))
        return np.frombuffer(raw.cpu().numpy().tobytes(), dtype=result).copy()
    call.__doc__ = f"World.{name}_records on the numpy records `records`: its result records, back on the host."
    return call


move, boxmove = _call("move", E.MOVE_RESULT), _call("boxmove", E.MOVE_RESULT)
walk, boxwalk = _call("walk", E.WALK_RESULT), _call("boxwalk", E.WALK_RESULT)
capsulecast, boxcast = _call("capsulecast", E.RAY_HIT), _call("boxcast", E.RAY_HIT)


def same(got, ref, what):
    """The result records `got` (nh_MoveResult or nh_WalkResult) are `ref`, byte for byte."""
    size, kind = ref.dtype.itemsize, "walk" if ref.dtype == E.WALK_RESULT else "move"
    bad = (got.view(np.uint8).reshape(-1, size) != ref.view(np.uint8).reshape(-1, size)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(ref)} {kind} results differ, first at {int(np.argmax(bad))}: {got[np.argmax(bad)]} != {ref[np.argmax(bad)]}"


def terrain_world():
    """(world, scene, collider records) of walk_batches.terrain(), built."""
    scene = WB.terrain()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    return w, scene, records(w, scene)


def miss(t=1.0):
    """The nh_RayHit record of a cast that missed."""
    m = np.zeros(1, dtype=E.RAY_HIT)
    m["t"], m["body"], m["collider"], m["shape"], m["tag"] = t, NONE, NONE, NONE, NONE
    return m[0]
