"""What the GPU tests of the list calls share (nh_overlap, nh_penetration, their wide forms, nh_region, the all-hits casts): one call into buffers filled
with a sentinel, the comparison with a brute force -- count-only offsets, list offsets, every byte of `hits`, the sentinel behind the written prefix
included -- and the two observer loops: queries between nh_step calls and between every call of the fused step must change nothing."""
import numpy as np

from query_util import FUSED, NONE, same_stepped_world, upload
from nudge_amd import engine as E

SENTINEL = 0xA5
CALLS = ("collide", "gravity", "read_cache", "setup", "apply", "update", "write_cache", "advance")


def sentinel_hits(capacity, dtype):
    """max(capacity, 1) records of `dtype` with every byte the sentinel: the host's `hits` as gpu_list() has them."""
    return np.frombuffer(bytes([SENTINEL]) * dtype.itemsize * max(capacity, 1), dtype=dtype).copy()


def gpu_list(w, call, records, capacity, dtype):
    """(offsets as uint32, hits): one call of World.<call> on the numpy `records`, offsets pre-filled with -1 and `hits` with the sentinel
    (max(capacity, 1) records of `dtype`; capacity None = count only, hits None)."""
    import torch
    ot = torch.full((len(records) + 1,), -1, dtype=torch.int32, device=w.dev)
    ht = None if capacity is None else torch.full((max(capacity, 1), dtype.itemsize), SENTINEL, dtype=torch.uint8, device=w.dev)
    getattr(w, call)(upload(w, records), offsets=ot, hits=ht, capacity=capacity or 0)
    off = ot.cpu().numpy().view(np.uint32).copy()
    hits = None if ht is None else np.frombuffer(ht.cpu().numpy().tobytes(), dtype=dtype).copy()
    return off, hits


def differ(a, b):
    """How many records of two equally long lists differ in any byte."""
    size = a.dtype.itemsize
    return int((a.view(np.uint8).reshape(-1, size) != b.view(np.uint8).reshape(-1, size)).any(axis=1).sum())


def same_lists(w, call, brute, rec, records, dtype, what, capacity=None, with_hits=False):
    """The count-only call, then a list call with `capacity` (None: exactly the total, or 0 at the overflow marker), against
    brute(rec, nbox, records, capacity=, hits=) -> (offsets, hits, total).  Returns the host's (offsets, total), or (offsets, hits, total)."""
    cnt, _ = gpu_list(w, call, records, None, dtype)
    ref_cnt, _, total = brute(rec, w.nbox, records, capacity=0)
    assert cnt.tobytes() == ref_cnt.tobytes(), f"{what}: count-only offsets differ in {int((cnt != ref_cnt).sum())} of {len(cnt)}"
    cap = (0 if total >= NONE else total) if capacity is None else capacity
    off, hits = gpu_list(w, call, records, cap, dtype)
    ref_off, ref_hits, _ = brute(rec, w.nbox, records, capacity=cap, hits=sentinel_hits(cap, dtype))
    assert off.tobytes() == cnt.tobytes(), f"{what}: list-mode offsets differ from count-only ones"
    assert off.tobytes() == ref_off.tobytes(), f"{what}: offsets differ"
    assert hits.tobytes() == ref_hits.tobytes(), f"{what}: {differ(hits, ref_hits)} of {len(hits)} records differ"
    return (ref_off, ref_hits, total) if with_hits else (ref_off, total)


# ---- observers ------------------------------------------------------------------------------------------------------------------------------
# scene(): the scene; make_batch(a, scene): the device buffers of the queries, made once on world a; query(a, *batch): a build and the calls under test.
def queries_between_nh_step_calls_change_nothing(scene, make_batch, query, what, still=False):
    """300 steps in nh_step calls of 1 to 8, the queries before each and after the last; still: the world must have taken still steps.  Returns the
    batch."""
    scene = scene()
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    batch = make_batch(a, scene)
    done = 0
    for k in [1, 2, 3, 5, 7, 4, 8] * 10:
        k = min(k, 300 - done)
        if k <= 0:
            break
        query(a, *batch)
        a.step(k)
        b.step(k)
        done += k
    query(a, *batch)
    assert done == 300
    same_stepped_world(a, b, f"{what} nh_step")
    if still:
        assert a.counts()["still_steps"] > 0, a.counts()
    a.close(); b.close()
    return batch


def queries_between_every_call_of_the_fused_step_change_nothing(scene, make_batch, query, what, still=False, steps=300):
    """`steps` steps as the eight calls of the fused step, the queries before each call and after the last."""
    scene = scene()
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    batch = make_batch(a, scene)
    for s in range(steps):
        for call in CALLS:
            query(a, *batch)
            getattr(a, call)()
            getattr(b, call)()
        a.step_done(); b.step_done()
    query(a, *batch)
    same_stepped_world(a, b, f"{what} call by call")
    if still:
        assert a.counts()["still_steps"] > 0, a.counts()
    a.close(); b.close()
    return batch
