"""nh_overlap_wide and nh_penetration_wide on the GPU (pytest -m gpu): include/nudge_hip.h, "nh_overlap_wide".

The contract is one sentence: for the same queries on the same build or refit the wide calls write exactly the bytes nh_overlap and nh_penetration
write.  Every comparison here is byte for byte against TWO references -- the host brute force over every collider (tests/hostoverlap_util.overlap with
capsules, tests/hostpen_util.penetration) and what nh_overlap / nh_penetration write for the same queries on the same context -- and each is the
count-only call, then a list call into a buffer filled with the sentinel 0xA5, then the sentinel behind the written prefix.  Nothing is skipped and
nothing is tolerated: the share left out is zero.  The worlds are the smallest at which the (query, entry node) decomposition can go wrong, those of
tests/test_gpu_region.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_util as F                      # noqa: E402
import hostlib as H                          # noqa: E402
import hostoverlap_util as O                 # noqa: E402
import hostpen_util as HP                    # noqa: E402
import list_util as LU                       # noqa: E402
from list_util import SENTINEL, differ, gpu_list as _gpu, same_lists      # noqa: E402
from query_util import FUSED, NONE, OBSERVED, SMALL, bounds as _bounds, unit_quats as _unit_quats, upload as _upload      # noqa: E402
from test_gpu_overlap import _capsule_queries, _coincident, _queries            # noqa: E402
from test_gpu_region import RUN, _rotated, _three_runs                          # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

# per call family: the wide wrapper, the plain one, the record, the brute force
KINDS = {
    "overlap": ("overlap_wide_records", "overlap_records", E.OVERLAP_HIT, lambda *a, **k: O.overlap(*a, capsules=True, **k)),
    "penetration": ("penetration_wide_records", "penetration_records", HP.HIT, HP.penetration),
}


# ---- queries --------------------------------------------------------------------------------------------------------------------------------
def _span(rec):
    lo, hi = _bounds(rec)
    return float(np.linalg.norm(np.maximum(hi - lo, 1.0)))


def _spoil(q, rng):
    """Every invalid kind of nh_overlap's list, in place at random slots (batches of 16 or more): an unknown shape, a NaN centre, a negative and an
    infinite size, a NaN box rotation; a capsule of negative / NaN half height, of a non-finite rotation, of a NaN centre.  All count 0."""
    if len(q) < 16:
        return
    at = rng.choice(len(q), size=9, replace=False)
    big = q["size"][:, 0].max() + 1.0
    for k, b in enumerate(at):
        q["ignore_body"][b] = NONE
        q["rotation"][b] = _unit_quats(rng, 1)[0]
        q["size"][b] = (big, 0.5 * big, big)                     # (each would list something were it valid)
        q["shape"][b] = E.NH_SHAPE_BOX if k < 5 else E.NH_SHAPE_CAPSULE
        if k == 0:
            q["shape"][b] = 7
        elif k == 1:
            q["center"][b, 1] = np.nan
        elif k == 2:
            q["size"][b, 0] = -0.5
        elif k == 3:
            q["size"][b, 2] = np.inf
        elif k == 4:
            q["rotation"][b, 0] = np.nan
        elif k == 5:
            q["size"][b, 1] = -0.5
        elif k == 6:
            q["size"][b, 1] = np.nan
        elif k == 7:
            q["rotation"][b, 2] = np.inf
        else:
            q["center"][b, 0] = np.nan


def _batch(rng, n, rec, spoil=True):
    """A mixed batch of n queries: spheres, boxes and capsules at random rotations, capsules of half height 0, radius-0 points on collider centres,
    `ignore_body`, at three sizes -- a body's (5 in 9), eight times that (3 in 9) and one that swallows the world (1 in 9, the first of the batch) --
    and every invalid kind."""
    world = _span(rec)
    q = np.zeros(n, dtype=E.OVERLAP_QUERY)
    for i, idx in enumerate(np.array_split(np.arange(n), min(n, 9))):
        scale = world if i == 0 else (8.0 if i % 3 == 1 else 1.0)
        m = len(idx)
        kind = i % 4
        if kind == 3:
            q[idx] = _queries(rng, m, rec, "point")
            continue
        part = _capsule_queries(rng, m, rec, scale) if kind == 1 else _queries(rng, m, rec, "mixed", scale)
        # (the helpers spoil one query of each batch they make; a batch of one or two stays valid here, and _spoil covers the kinds)
        if m < 16:
            fresh = _queries(rng, m, rec, "sphere" if kind else "box", scale)
            if kind == 1:
                fresh["shape"], fresh["size"][:, 1], fresh["rotation"] = E.NH_SHAPE_CAPSULE, rng.choice([0.0, 0.4]) * scale, _unit_quats(rng, m)
            part = fresh
        q[idx] = part
    if spoil:
        _spoil(q, rng)
    return q


def _swallow(rec):
    """A sphere, a rotated box and a rotated capsule that each hold the whole world, and a capsule of half height 0 that does."""
    lo, hi = _bounds(rec)
    r = 2.0 * _span(rec) + 10.0
    q = np.zeros(4, dtype=E.OVERLAP_QUERY)
    q["center"], q["ignore_body"] = 0.5 * (lo + hi), NONE
    q["rotation"] = _unit_quats(np.random.default_rng(5), 4)
    q["shape"] = (E.NH_SHAPE_SPHERE, E.NH_SHAPE_BOX, E.NH_SHAPE_CAPSULE, E.NH_SHAPE_CAPSULE)
    q["size"] = [(r, 0, 0), (r, r, r), (r, 0.5 * r, np.nan), (r, 0.0, np.nan)]
    return q


# ---- the comparison -------------------------------------------------------------------------------------------------------------------------
def _same(w, rec, queries, what, capacity=None, kinds=("overlap", "penetration")):
    """For each call family: the wide count-only call, then the wide list call with `capacity` (None: exactly the total), against the brute force
    (list_util.same_lists) and against the plain call -- offsets, records and the sentinel behind the written prefix, which the wide call's were
    just found to share with the brute force's byte for byte.  Returns the host offsets and the total."""
    for kind in kinds:
        wide, plain, dtype, brute = KINDS[kind]
        ref_off, ref_hits, total = same_lists(w, wide, brute, rec, queries, dtype, f"{what} / {kind}", capacity, with_hits=True)
        assert ref_off.tobytes() == _gpu(w, plain, queries, None, dtype)[0].tobytes(), f"{what} / {kind}: count-only offsets differ from the plain call's"
        plain_off, plain_hits = _gpu(w, plain, queries, (0 if total >= NONE else total) if capacity is None else capacity, dtype)
        assert ref_off.tobytes() == plain_off.tobytes(), f"{what} / {kind}: offsets differ from the plain call's"
        assert ref_hits.tobytes() == plain_hits.tobytes(), f"{what} / {kind}: {differ(ref_hits, plain_hits)} of {len(ref_hits)} records differ from the plain call's"
    return ref_off, total


def _records(w, scene, bodies=None):
    bt = w.get_bodies()["transforms"]
    return H.records(bt if bodies is None else bt[:bodies], scene, w.nbox, w.nsph)


def _check_world(w, scene, rng, what, sizes=(1, 3, 257), build=True, bodies=None):
    if build:
        w.query_build()
    rec = _records(w, scene, bodies)
    totals = [_same(w, rec, _batch(rng, n, rec), f"{what} / {n} queries")[1] for n in sizes]
    off, total = _same(w, rec, _swallow(rec), f"{what} / the whole world")
    assert total == 4 * int(np.isfinite(rec["p"]).all(axis=1).sum()) and (np.diff(off.astype(np.int64)) == total // 4).all()
    return rec, totals


# ---- worlds ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SMALL))
def test_wide_equals_the_brute_force_and_the_plain_call_before_and_after_stepping_with_a_refit(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(700 + sorted(SMALL).index(name))
    w = E.World(scene, flags=FUSED)
    _, totals = _check_world(w, scene, rng, f"{name} initial")
    assert totals[-1] > 1000, totals
    w.step(50)
    w.query_refit()                                                       # after a refit the bytes are those after a build
    rec, totals = _check_world(w, scene, rng, f"{name} refitted after 50 steps", build=False)
    assert totals[-1] > 1000, totals
    q = _batch(rng, 64, rec)
    refit = [_gpu(w, KINDS[k][0], q, 1 << 16, KINDS[k][2]) for k in KINDS]
    w.query_build()
    built = [_gpu(w, KINDS[k][0], q, 1 << 16, KINDS[k][2]) for k in KINDS]
    for a, b in zip(refit, built):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    _same(w, rec, q, f"{name} rebuilt", capacity=1 << 16)
    w.close()


def test_zero_one_and_two_colliders():
    scene = S.pile(4, 0, seed=3)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    rng = np.random.default_rng(71)
    q = _swallow(_records(w, scene))
    w.set_counts(nb, 0, 0)                                                # no collider: all-zero offsets
    w.query_build()
    assert len(_records(w, scene)) == 0
    for kind in KINDS:
        wide, _, dtype, _ = KINDS[kind]
        off, hits = _gpu(w, wide, q, 8, dtype)
        assert not off.any() and set(hits.tobytes()) == {SENTINEL}
        assert not _gpu(w, wide, q, None, dtype)[0].any()
    w.set_counts(nb, 1, 0)                                                # the ground slab alone (body 0): the root is a leaf
    _check_world(w, scene, rng, "one collider")
    off, hits = _gpu(w, "overlap_wide_records", q[:1], 4, E.OVERLAP_HIT)
    assert list(off) == [0, 1] and hits["body"][0] == 0 and hits["shape"][0] == E.NH_SHAPE_BOX
    w.set_counts(nb, 2, 0)
    _check_world(w, scene, rng, "two colliders")
    w.close()


def test_the_root_as_the_one_entry_and_the_first_top_list():
    for boxes in (RUN - 1, RUN):                                          # with the ground slab: NH_Q_RUN colliders, and NH_Q_RUN + 1
        scene = _rotated(S.pile(boxes, 0, seed=3), 72)
        w = E.World(scene, flags=FUSED)
        w.query_build()
        st = w.query_stats()
        assert st["colliders"] == boxes + 1 and (st["runs"] >= 2) == (boxes == RUN), st
        _check_world(w, scene, np.random.default_rng(73 + boxes), f"{boxes + 1} colliders", build=False)
        w.close()


def test_a_world_of_three_runs_with_boxes_and_spheres():
    scene = _three_runs()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    st = w.query_stats()
    assert st["colliders"] == 3001 and st["runs"] >= 2 and st["top_nodes"] > 0, st
    _check_world(w, scene, np.random.default_rng(75), "three runs", sizes=(1, 3, 257, 2000), build=False)
    w.close()


def test_only_spheres_and_only_boxes():
    scene = _rotated(S.pile(300, 300, seed=3), 76)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    rng = np.random.default_rng(77)
    w.set_counts(nb, 0, 300)
    _check_world(w, scene, rng, "spheres only")
    w.set_counts(nb, 301, 0)
    _check_world(w, scene, rng, "boxes only")
    w.close()


def test_four_thousand_boxes_at_one_position():
    scene = _coincident()
    w = E.World(scene, flags=FUSED)
    rec, _ = _check_world(w, scene, np.random.default_rng(78), "4096 coincident boxes")
    # spheres a hair on either side of touching the common box, and points at its centre
    q = np.zeros(6, dtype=E.OVERLAP_QUERY)
    q["shape"], q["rotation"], q["ignore_body"] = E.NH_SHAPE_SPHERE, (0, 0, 0, 1), NONE
    q["center"] = (0.25, 3.0, -0.5)
    q["center"][:5, 0] += 3.0
    q["size"][:5, 0] = 3.0 - rec["h"][1, 0] + np.float32([-1e-3, -1e-6, 0.0, 1e-6, 1e-3])
    _same(w, rec, q, "4096 coincident boxes / spheres about touching")
    w.close()


def test_colliders_of_a_body_that_does_not_exist():
    scene = _rotated(S.pile(200, 100, seed=3), 79)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    w.set_counts(nb - 40, w.nbox, w.nsph)                                 # the last 40 spheres belong to bodies that no longer exist: NaN poses
    rec, _ = _check_world(w, scene, np.random.default_rng(80), "40 colliders without a body", bodies=nb - 40)
    assert int((~np.isfinite(rec["p"]).all(axis=1)).sum()) == 40
    w.close()


# ---- batches, capacities, repeatability -----------------------------------------------------------------------------------------------------
def test_a_batch_whose_items_stride_the_grid():
    scene = S.grid_tiles(2, side=64, sphere_fraction=0.5, seed=2)
    w = E.World(scene, flags=FUSED)
    w.query_build()
    st = w.query_stats()
    assert st["colliders"] == 8194 and st["runs"] >= 7 and st["top_nodes"] > 0, st
    entries = st["top_nodes"] + 1
    rec = _records(w, scene)
    # the kernel deals (query, entry) items to 8192 waves in chunks of at most 64: more items than that and the waves come round again
    n = (8192 * 64) // entries + 300
    assert 2000 < n < 12000, (n, entries)
    rng = np.random.default_rng(81)
    q = np.concatenate([_queries(rng, n - n // 3, rec, "mixed"), _capsule_queries(rng, n // 3, rec)])
    q["size"][::50] *= 20.0                                               # some that reach many entries
    q = q[rng.permutation(n)]
    _, total = _same(w, rec, q, f"{n} queries x {entries} entries")
    assert total > n
    w.close()


def test_capacity_writes_whole_segments_and_nothing_behind_them():
    scene = _three_runs()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    q = _batch(np.random.default_rng(82), 257, rec)
    ref_off, _, total = O.overlap(rec, w.nbox, q, capacity=0, capsules=True)
    nz = np.nonzero(np.diff(ref_off.astype(np.int64)) > 1)[0]
    boundary = int(ref_off[nz[len(nz) // 2]])                  # the start of a segment of at least two records: a cut between two segments
    assert 0 < boundary < total
    for cap in (total, total - 1, boundary, boundary + 1, 0):
        _same(w, rec, q, f"capacity {cap} of {total}", capacity=cap)
    # capacity 0 with a non-null hits buffer: count only, the buffer untouched
    for kind in KINDS:
        off, hits = _gpu(w, KINDS[kind][0], q, 0, KINDS[kind][2])
        assert off.tobytes() == ref_off.tobytes() and set(hits.tobytes()) == {SENTINEL}
    w.close()


def test_two_identical_calls_give_identical_bytes():
    scene = _three_runs()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    q = _batch(np.random.default_rng(83), 257, rec)
    total = O.overlap(rec, w.nbox, q, capacity=0, capsules=True)[2]
    assert total > 10000
    for kind in KINDS:
        wide, _, dtype, _ = KINDS[kind]
        a, b = _gpu(w, wide, q, total, dtype), _gpu(w, wide, q, total, dtype)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    w.close()


def test_a_total_of_two_to_the_thirty_second_writes_the_marker_and_no_record():
    scene = _coincident()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    q = np.zeros(1 << 20, dtype=E.OVERLAP_QUERY)
    q["shape"], q["center"], q["rotation"], q["ignore_body"] = E.NH_SHAPE_SPHERE, (0.25, 3.0, -0.5), (0, 0, 0, 1), NONE
    assert O.overlap(rec, w.nbox, q[:1], capacity=0)[2] == 4096  # so 2^20 of them make exactly 2^32: the 32-bit scan wraps to 0
    for kind in KINDS:
        wide, plain, dtype, _ = KINDS[kind]
        cnt, _ = _gpu(w, wide, q, None, dtype)
        assert cnt[-1] == NONE and cnt.tobytes() == _gpu(w, plain, q, None, dtype)[0].tobytes()
    # 2^20 - 1 queries: 2^32 - 4096 records, no wrap
    cnt, _ = _gpu(w, "overlap_wide_records", q[1:], None, E.OVERLAP_HIT)
    assert int(cnt[-1]) == (1 << 32) - 4096 and (np.diff(cnt.astype(np.int64)) == 4096).all()
    w.close()


def test_the_python_wrappers():
    scene = _three_runs()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    centres = rec["p"][:5].astype(np.float64)
    body = int(rec["body"][7])
    for args in (dict(radii=6.0), dict(half_extents=(5.0, 2.0, 7.0), rotations=_unit_quats(np.random.default_rng(84), 5)),
                 dict(radii=2.0, half_heights=[0.0, 1.0, 5.0, 9.0, 2.0], rotations=_unit_quats(np.random.default_rng(85), 5), ignore_body=body)):
        for wide, plain in ((w.overlap_wide, w.overlap), (w.penetration_wide, w.penetration)):
            a, b = wide(centres, synchronize=True, **args), plain(centres, synchronize=True, **args)
            assert sorted(a) == sorted(b) and int(a["written"]) == int(b["written"]) > 5
            for k in a:
                assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
            c = wide(centres, capacity=int(a["written"]) + 7, **args)
            assert int(c["written"]) == int(a["written"]) and c["raw"].cpu().numpy()[:int(a["written"])].tobytes() == a["raw"].cpu().numpy().tobytes()
    assert body not in a["body"].cpu().numpy()
    with pytest.raises(ValueError):
        w.overlap_wide(centres)
    w.close()


# ---- layer masks ----------------------------------------------------------------------------------------------------------------------------
def test_the_filter_off_uniform_and_per_query_equals_the_unfiltered_call_on_the_masked_world():
    scene = _three_runs()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    rng = np.random.default_rng(86)
    q = _batch(rng, 257, rec)
    words = F.layers(len(rec), 87)
    assert (words == 0).any()
    whole_off, whole = _same(w, rec, q, "before any filter call")
    w.query_set_layers(words[:w.nbox], words[w.nbox:])
    _same(w, rec, q, "layers set, filter off")
    for mask in F.MASKS:
        w.query_filter(mask)
        off, total = _same(w, F.masked(rec, words, mask), q, f"uniform mask {mask:#x}")
        if mask == 0:
            assert total == 0 and not off.any()                           # mask 0 lists nothing
        elif mask != NONE:
            assert total < whole and (total > 0) == (mask != 0x80000000)  # (no collider carries bit 31)
    # per-query masks: query i under masks[i]
    values = (0, 1, 6, 0xFFFFFFFF)
    masks = rng.choice(np.uint32(values), size=len(q))
    w.query_filter(_upload(w, masks).view(w.torch.int32))
    for kind in KINDS:
        wide, plain, dtype, brute = KINDS[kind]
        cnt, _ = _gpu(w, wide, q, None, dtype)
        sizes = np.zeros(len(q), dtype=np.int64)
        parts = {}
        for v in values:
            o, h, _ = brute(F.masked(rec, words, v), w.nbox, q)
            sizes[masks == v] = np.diff(o.astype(np.int64))[masks == v]
            parts[v] = (o, h)
        ref_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
        ref_hits = np.concatenate([parts[int(masks[i])][1][int(parts[int(masks[i])][0][i]):int(parts[int(masks[i])][0][i + 1])] for i in range(len(q))])
        assert cnt.tobytes() == ref_off.tobytes(), kind
        off, hits = _gpu(w, wide, q, len(ref_hits) + 5, dtype)
        assert off.tobytes() == ref_off.tobytes() and hits[:len(ref_hits)].tobytes() == ref_hits.tobytes() and set(hits[len(ref_hits):].tobytes()) == {SENTINEL}, kind
        plain_off, plain_hits = _gpu(w, plain, q, len(ref_hits) + 5, dtype)
        assert off.tobytes() == plain_off.tobytes() and hits.tobytes() == plain_hits.tobytes(), kind
        assert any(ref_off.tobytes() != parts[v][0].tobytes() for v in values)
    # all-ones layers with a mask, and the filter off again, give the filter-off bytes
    w.query_filter(5)
    w.query_set_layers(np.full(w.nbox, NONE, dtype=np.uint32), np.full(w.nsph, NONE, dtype=np.uint32))
    assert _same(w, rec, q, "all-ones layers, mask 5")[0].tobytes() == whole_off.tobytes()
    w.query_set_layers(words[:w.nbox], words[w.nbox:])
    w.query_filter(None)
    assert _same(w, rec, q, "filter off again")[0].tobytes() == whole_off.tobytes()
    w.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_abi_edge_cases(kind):
    import torch
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    fn = getattr(w.L, "nh_" + kind + "_wide")
    dtype, brute = KINDS[kind][2], KINDS[kind][3]
    rec = _records(w, scene)
    q = _queries(np.random.default_rng(88), 1024, rec, "mixed")
    q[::7] = _capsule_queries(np.random.default_rng(89), len(q[::7]), rec)
    qt = _upload(w, q)
    buf = torch.zeros(4 * 1032, dtype=torch.int32, device=w.dev)
    ot = buf[:1025]
    ht = torch.zeros((4096, dtype.itemsize), dtype=torch.uint8, device=w.dev)
    qp, op, hp = C.c_void_p(qt.data_ptr()), C.c_void_p(ot.data_ptr()), C.c_void_p(ht.data_ptr())
    assert fn(w.ctx, qp, 1024, op, hp, 4096, 0) == 1                           # before any build: NH_ERR_INVALID
    assert fn(None, qp, 1024, op, hp, 4096, 0) == 1
    w.query_build()
    assert fn(w.ctx, qp, 1024, op, hp, 4096, 1) == 1                           # flags
    assert fn(w.ctx, None, 1024, op, hp, 4096, 0) == 1                         # null / unaligned queries
    assert fn(w.ctx, C.c_void_p(qt.data_ptr() + 4), 1023, op, hp, 4096, 0) == 1
    assert fn(w.ctx, qp, 1024, None, hp, 4096, 0) == 1                         # null / unaligned offsets
    assert fn(w.ctx, qp, 1024, C.c_void_p(ot.data_ptr() + 2), hp, 4096, 0) == 1
    assert fn(w.ctx, qp, 1024, op, None, 4096, 0) == 1                         # null hits with a capacity, unaligned hits
    assert fn(w.ctx, qp, 1024, op, C.c_void_p(ht.data_ptr() + 8), 4095, 0) == 1
    assert fn(w.ctx, qp, 1 << 30, op, hp, 4096, 0) == 1                        # count >= 2^30: refused on the host, nothing launched
    assert fn(w.ctx, qp, 0xFFFFFFFF, op, hp, 4096, 0) == 1
    assert fn(w.ctx, qp, 0, op, hp, 4096, 0) == 0                              # count 0: a no-op
    assert fn(w.ctx, None, 0, None, None, 0, 0) == 0
    # nh_overlap's order: a flag wins over a null pointer, the count bound over the pointers, count 0 over them all but the flag
    assert fn(w.ctx, None, 0, None, None, 0, 1) == 1 and fn(w.ctx, None, 1 << 30, None, None, 0, 0) == 1
    w.torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0 and int(ht.sum()) == 0                    # nothing was written
    # offsets need 4-byte alignment only
    ot4 = buf[1:1026]
    assert fn(w.ctx, qp, 1024, C.c_void_p(ot4.data_ptr()), hp, 4096, 0) == 0
    ref_hits = np.zeros(4096, dtype=dtype)
    ref_off, ref_hits, total = brute(rec, w.nbox, q, capacity=4096, hits=ref_hits)
    assert 0 < total <= 4096
    assert ot4.cpu().numpy().view(np.uint32).tobytes() == ref_off.tobytes()
    got = np.frombuffer(ht.cpu().numpy().tobytes(), dtype=dtype)
    assert got[:total].tobytes() == ref_hits[:total].tobytes() and not got[total:].view(np.uint8).any()
    assert int(buf[1026:].abs().sum()) == 0 and int(buf[0]) == 0               # count + 1 offsets and no word beside them
    w.close()


# ---- observers ------------------------------------------------------------------------------------------------------------------------------
def _observer_batch(a, scene):
    import torch
    a.query_build()
    rec = _records(a, scene)
    q = _batch(np.random.default_rng(90), 64, rec)
    return _upload(a, q), torch.empty(65, dtype=torch.int32, device=a.dev), torch.empty((1 << 15, 32), dtype=torch.uint8, device=a.dev)


def _query(w, qt, ot, ht):
    w.query_build()
    w.overlap_wide_records(qt, offsets=ot)
    w.overlap_wide_records(qt, offsets=ot, hits=ht, capacity=ht.shape[0])
    w.penetration_wide_records(qt, offsets=ot, hits=ht, capacity=ht.shape[0])


def test_wide_calls_between_nh_step_calls_change_nothing():
    LU.queries_between_nh_step_calls_change_nothing(OBSERVED["grid_tiles"], _observer_batch, _query, "grid_tiles", still=True)


def test_wide_calls_between_every_call_of_the_fused_step_change_nothing():
    LU.queries_between_every_call_of_the_fused_step_change_nothing(OBSERVED["pile"], _observer_batch, _query, "pile", steps=120)


# ---- trigger events fed by the wide lists ---------------------------------------------------------------------------------------------------
def test_two_wide_lists_give_the_events_of_the_two_plain_lists():
    scene = SMALL["pile"]()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    rng = np.random.default_rng(91)
    lo, hi = _bounds(rec)
    centres = rng.uniform(lo, hi, size=(48, 3))
    radii = rng.uniform(1.0, 0.5 * _span(rec), size=48)
    prev = [f(centres, radii=radii, synchronize=True) for f in (w.overlap_wide, w.overlap)]
    w.step(40)
    w.query_refit()
    cur = [f(centres, radii=radii, synchronize=True) for f in (w.overlap_wide, w.overlap)]
    for k in ("offsets", "raw"):
        assert prev[0][k].cpu().numpy().tobytes() == prev[1][k].cpu().numpy().tobytes() and cur[0][k].cpu().numpy().tobytes() == cur[1][k].cpu().numpy().tobytes()
    events = 0
    for by_body in (False, True):
        a, b = (w.overlap_events(prev[i], cur[i], by_body=by_body, synchronize=True) for i in (0, 1))
        for side in ("entered", "left"):
            n = int(a[side]["written"])
            assert n == int(b[side]["written"])
            assert a[side]["offsets"].cpu().numpy().tobytes() == b[side]["offsets"].cpu().numpy().tobytes()
            assert a[side]["raw"].cpu().numpy()[:n].tobytes() == b[side]["raw"].cpu().numpy()[:n].tobytes()
            events += n
    assert events > 0
    w.close()
