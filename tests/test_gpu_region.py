"""Region queries on the GPU (pytest -m gpu): nh_region (include/nudge_hip.h, "scene queries").

The oracle is a brute force over every collider on the host with the same per-plane predicates (nudge_amd/csrc/nh_query.h, "region", through
tests/hostregion_util.py).  The answer is defined without reference to the tree -- per region the colliders in ascending combined index, laid out by
the exclusive scan of the counts -- so offsets and records must equal the brute force byte for byte, and so must every byte of `hits` behind the
written prefix (a sentinel there stays the sentinel).  Every comparison is the count-only call, then a list call, then the sentinel check."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_util as F                      # noqa: E402
import hostregion_util as R                  # noqa: E402
import list_util as LU                       # noqa: E402
from list_util import SENTINEL, gpu_list, same_lists, sentinel_hits      # noqa: E402
from query_util import FUSED, NONE, OBSERVED, SMALL, bounds as _bounds, unit_quats as _unit_quats, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

RUN = 1024                                   # NH_Q_RUN


# ---- regions -------------------------------------------------------------------------------------------------------------------------------
def _frusta(rng, n, rec):
    """n camera frusta (engine.frustum_planes of perspective x look-at matrices): eyes around the scene, each looking at a collider."""
    lo, hi = _bounds(rec)
    span = np.maximum(hi - lo, 4.0)
    live = np.nonzero(np.isfinite(rec["p"]).all(axis=1))[0]
    out = np.zeros((n, 6, 4), dtype=np.float32)
    for k in range(n):
        eye = rng.uniform(lo - 0.5 * span, hi + 0.5 * span)
        fwd = rec["p"][rng.choice(live)].astype(np.float64) + rng.normal(scale=0.5, size=3) - eye
        fwd /= max(np.linalg.norm(fwd), 1e-9)
        up = np.cross(np.cross(fwd, rng.normal(size=3)), fwd)
        up /= max(np.linalg.norm(up), 1e-9)
        right = np.cross(fwd, up)
        view = np.eye(4)
        view[0, :3], view[1, :3], view[2, :3] = right, up, -fwd
        view[:3, 3] = -view[:3, :3] @ eye
        f, aspect, near = 1.0 / np.tan(np.radians(rng.uniform(20, 100)) / 2), rng.uniform(1.0, 2.0), rng.uniform(0.1, 2.0)
        far = near + rng.uniform(0.2, 2.0) * float(np.linalg.norm(span))
        proj = np.array([[f / aspect, 0, 0, 0], [0, f, 0, 0], [0, 0, (far + near) / (near - far), 2 * far * near / (near - far)], [0, 0, -1, 0]])
        out[k] = E.frustum_planes(proj @ view)
    return out


def _cubes(rng, n, rec, half):
    """n axis-aligned cubes of half size `half` around collider centres, as six planes each."""
    live = np.nonzero(np.isfinite(rec["p"]).all(axis=1))[0]
    c = rec["p"][rng.choice(live, size=n)].astype(np.float64) + rng.normal(scale=half, size=(n, 3))
    out = np.zeros((n, 6, 4), dtype=np.float32)
    for k in range(3):
        out[:, 2 * k, k], out[:, 2 * k, 3] = 1.0, -(c[:, k] - half)
        out[:, 2 * k + 1, k], out[:, 2 * k + 1, 3] = -1.0, c[:, k] + half
    return out


def _invalid(regs, rng):
    """Spoil about one region in eight, in place: plane counts 0 and 9, a NaN, an infinity, a zero normal, a normal whose square overflows."""
    bad = rng.choice(len(regs), size=len(regs) // 8 if len(regs) >= 8 else min(len(regs) - 1, 1), replace=False)      # (a batch of one stays valid)
    for j, b in enumerate(bad):
        kind, pc = j % 6, max(int(regs["plane_count"][b]), 1)
        k = int(rng.integers(pc))
        if kind == 0:
            regs["plane_count"][b] = 0
        elif kind == 1:
            regs["plane_count"][b] = 9
        elif kind == 2:
            regs["planes"][b, k, int(rng.integers(4))] = np.nan
        elif kind == 3:
            regs["planes"][b, k, int(rng.integers(4))] = np.inf * rng.choice([-1.0, 1.0])
        elif kind == 4:
            regs["planes"][b, k, :3] = 0.0
        else:
            regs["planes"][b, k, :3] = (1e20, -1e19, 0.0)
    return bad


def _regions(rng, n, rec):
    """A mixed batch of n regions: frusta, one far-away plane that keeps everything, two opposed half-spaces with a gap, a single plane through the
    scene, eight planes, normals scaled by 2^+-10, small cubes; one in four ignores a body; one in eight is invalid; garbage behind plane_count."""
    lo, hi = _bounds(rec)
    live = np.nonzero(np.isfinite(rec["p"]).all(axis=1))[0]
    regs = np.zeros(n, dtype=E.REGION)
    regs["planes"] = rng.normal(size=(n, 8, 4)) * 1e3                    # never read behind plane_count
    regs["planes"][rng.random((n, 8, 4)) < 0.1] = np.nan
    regs["reserved"] = rng.integers(0, 1 << 32, size=(n, 2), dtype=np.uint64).astype(np.uint32)
    regs["ignore_body"] = NONE
    fr = _frusta(rng, n, rec)
    cu = _cubes(rng, n, rec, 1.5)
    for i in range(n):
        kind = i % 7
        through = rec["p"][rng.choice(live)].astype(np.float64)
        nrm = rng.normal(size=3)
        if kind == 0:
            regs["planes"][i, :6], regs["plane_count"][i] = fr[i], 6
        elif kind == 1:                                                   # keeps everything
            regs["planes"][i, 0], regs["plane_count"][i] = (0.0, 1.0, 0.0, 1e6), 1
        elif kind == 2:                                                   # x <= a and x >= a + gap: nothing
            a = rng.uniform(lo[0], hi[0])
            regs["planes"][i, :2], regs["plane_count"][i] = [(-1.0, 0.0, 0.0, a), (1.0, 0.0, 0.0, -(a + 1e4))], 2
        elif kind == 3:                                                   # a single plane through a collider's centre
            regs["planes"][i, 0], regs["plane_count"][i] = (*nrm, -float(nrm @ through)), 1
        elif kind == 4:                                                   # eight planes: a frustum and a slab across it
            regs["planes"][i, :6] = fr[i]
            regs["planes"][i, 6:8] = [(*nrm, -float(nrm @ through) + 3.0 * np.linalg.norm(nrm)), (*(-nrm), float(nrm @ through) + 3.0 * np.linalg.norm(nrm))]
            regs["plane_count"][i] = 8
        elif kind == 5:                                                   # un-normalised: each plane scaled by 2^+-10
            regs["planes"][i, :6] = fr[i] * rng.choice(np.float32([2.0 ** -10, 2.0 ** 10]), size=(6, 1))
            regs["plane_count"][i] = 6
        else:
            regs["planes"][i, :6], regs["plane_count"][i] = cu[i], 6
    ign = rng.random(n) < 0.25
    regs["ignore_body"][ign] = rec["body"][rng.choice(live, size=int(ign.sum()))]
    _invalid(regs, rng)
    return regs


# ---- the comparison -------------------------------------------------------------------------------------------------------------------------
def _gpu(w, regs, capacity):
    """(offsets, hits): one nh_region call with `hits` pre-filled with the sentinel (capacity records; None = count only)."""
    return gpu_list(w, "region_records", regs, capacity, E.OVERLAP_HIT)


def _same(w, rec, regs, what, capacity=None):
    """The count-only call, then a list call with `capacity` (None: exactly the total), against the brute force -- the sentinel behind the written
    prefix included; returns the host offsets and the total."""
    return same_lists(w, "region_records", R.region, rec, regs, E.OVERLAP_HIT, what, capacity)


def _records(w, scene, bodies=None):
    bt = w.get_bodies()["transforms"]
    return R.records(bt if bodies is None else bt[:bodies], scene, w.nbox, w.nsph)


def _check_world(w, scene, rng, what, sizes=(1, 3, 257), build=True, bodies=None):
    if build:
        w.query_build()
    rec = _records(w, scene, bodies)
    totals = [_same(w, rec, _regions(rng, n, rec), f"{what} / {n} regions")[1] for n in sizes]
    # the far-away plane: everything but the NaN poses
    every = R.regions([[(0.0, 1.0, 0.0, 1e6)]])
    off, total = _same(w, rec, every, f"{what} / everything")
    assert total == int(np.isfinite(rec["p"]).all(axis=1).sum()) == int(off[1])
    # two opposed half-spaces with a gap between them: nothing
    if len(rec):
        a = float(_bounds(rec)[0][0])
        _, total = _same(w, rec, R.regions([[(-1.0, 0.0, 0.0, a), (1.0, 0.0, 0.0, -(a + 1e4))]]), f"{what} / a gap")
        assert total == 0
    return rec, totals


def _rotated(scene, seed):
    """The scene with every body but the static world turned by a random unit quaternion."""
    scene["body_transforms"]["rotation"][1:] = _unit_quats(np.random.default_rng(seed), len(scene["body_transforms"]) - 1)
    return scene


# ---- worlds ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SMALL))
def test_regions_equal_the_brute_force_before_and_after_stepping_with_a_refit(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(500 + sorted(SMALL).index(name))
    w = E.World(scene, flags=FUSED)
    _, totals = _check_world(w, scene, rng, f"{name} initial")
    assert totals[-1] > 1000, totals
    w.step(50)
    w.query_refit()                                                       # after a refit the bytes are those after a build
    rec, totals = _check_world(w, scene, rng, f"{name} refitted after 50 steps", build=False)
    assert totals[-1] > 1000, totals
    regs = _regions(rng, 64, rec)
    refit = _gpu(w, regs, 1 << 16)
    w.query_build()
    built = _gpu(w, regs, 1 << 16)
    assert refit[0].tobytes() == built[0].tobytes() and refit[1].tobytes() == built[1].tobytes()
    w.close()


def test_zero_one_and_two_colliders():
    scene = S.pile(4, 0, seed=3)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    rng = np.random.default_rng(41)
    w.set_counts(nb, 0, 0)                                                # no collider: all-zero offsets
    w.query_build()
    rec = _records(w, scene)
    assert len(rec) == 0
    regs = R.regions(np.tile(np.float32([(0.0, 1.0, 0.0, 1e6)]), (5, 1, 1)))
    off, hits = _gpu(w, regs, 8)
    assert not off.any() and set(hits.tobytes()) == {SENTINEL}
    assert not _gpu(w, regs, None)[0].any()
    w.set_counts(nb, 1, 0)                                                # the ground slab alone (body 0): the root is a leaf
    rec, _ = _check_world(w, scene, rng, "one collider")
    off, hits = _gpu(w, R.regions([[(0.0, 1.0, 0.0, 1e6)]]), 4)
    assert list(off) == [0, 1] and hits["body"][0] == 0 and hits["shape"][0] == E.NH_SHAPE_BOX
    w.set_counts(nb, 2, 0)
    _check_world(w, scene, rng, "two colliders")
    w.close()


def test_a_second_run_of_one_leaf():
    scene = _rotated(S.pile(RUN, 0, seed=3), 42)                          # the ground slab and 1024 boxes: NH_Q_RUN + 1 colliders
    w = E.World(scene, flags=FUSED)
    w.query_build()
    st = w.query_stats()
    assert st["colliders"] == RUN + 1 and st["runs"] == 2
    _check_world(w, scene, np.random.default_rng(43), "1025 colliders", build=False)
    w.close()


def _three_runs():
    return _rotated(S.pile(2000, 1000, seed=3), 44)


def test_a_world_of_three_runs_with_boxes_and_spheres():
    scene = _three_runs()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    st = w.query_stats()
    assert st["colliders"] == 3001 and st["runs"] >= 2 and st["top_nodes"] > 0, st
    rng = np.random.default_rng(45)
    rec, _ = _check_world(w, scene, rng, "three runs", sizes=(1, 3, 257, 2000), build=False)
    # camera frusta alone, and cubes alone
    _same(w, rec, R.regions(_frusta(rng, 257, rec)), "three runs / frusta")
    _same(w, rec, R.regions(_cubes(rng, 257, rec, 3.0)), "three runs / cubes")
    w.close()


def test_only_spheres_and_only_boxes():
    scene = _rotated(S.pile(300, 300, seed=3), 46)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    rng = np.random.default_rng(47)
    w.set_counts(nb, 0, 300)
    _check_world(w, scene, rng, "spheres only")
    w.set_counts(nb, 301, 0)
    _check_world(w, scene, rng, "boxes only")
    w.close()


def test_four_thousand_boxes_at_one_position():
    scene = S.pile(4096, 0, seed=3)
    scene["body_transforms"]["position"][1:] = (0.25, 3.0, -0.5)        # every box at one position; the ground slab elsewhere
    w = E.World(scene, flags=FUSED)
    rec, _ = _check_world(w, scene, np.random.default_rng(48), "4096 coincident boxes")
    # one plane a hair on either side of the common centre
    regs = R.regions([[(1.0, 0.0, 0.0, -0.25 + e)] for e in (-3.0, -1e-3, 0.0, 1e-3, 3.0)])
    _same(w, rec, regs, "4096 coincident boxes / planes about the centre")
    w.close()


def test_colliders_of_a_body_that_does_not_exist():
    scene = _rotated(S.pile(200, 100, seed=3), 49)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    w.set_counts(nb - 40, w.nbox, w.nsph)                                 # the last 40 spheres belong to bodies that no longer exist: NaN poses
    rec, _ = _check_world(w, scene, np.random.default_rng(50), "40 colliders without a body", bodies=nb - 40)
    assert int((~np.isfinite(rec["p"]).all(axis=1)).sum()) == 40
    w.close()


def _lattice(side=12):
    """side^3 unit boxes at integer centres, identity rotation, half extents 0.5 (and the ground slab far below)."""
    scene = S.pile(side ** 3, 0, seed=3)
    k = np.arange(side ** 3)
    scene["body_transforms"]["position"][1:] = np.stack([k % side, (k // side) % side, k // (side * side)], axis=1)
    scene["box_data"]["size"][1:] = 0.5
    return scene


def test_lattice_aligned_slabs_whose_planes_touch_box_faces_exactly():
    side = 12
    scene = _lattice(side)
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    planes = []
    for axis in range(3):
        e = np.eye(3)[axis]
        for a in range(0, side - 1, 2):
            for b in range(a, side, 3):
                # a + 0.5 <= x <= b + 0.5 on the axis: the boxes centred at a and at b + 1 touch it with a face, s + r == 0
                planes.append([(*e, -(a + 0.5)), (*(-e), b + 0.5)])
    regs = R.regions(np.float32(planes))
    off, total = _same(w, rec, regs, "lattice slabs")
    i = 0
    for axis in range(3):
        for a in range(0, side - 1, 2):
            for b in range(a, side, 3):
                # (the ground slab, 800 wide and 20 thick around y = -20, reaches into the slabs across x and across z)
                assert int(off[i + 1]) - int(off[i]) == (min(b + 1, side - 1) - a + 1) * side * side + (axis != 1), (axis, a, b)
                i += 1
    # a quarter off the faces: the touching layers drop out
    regs["planes"][:, 0, 3] -= 0.25
    regs["planes"][:, 1, 3] -= 0.25
    off2, _ = _same(w, rec, regs, "lattice slabs, a quarter inside")
    assert (np.diff(off2.astype(np.int64)) < np.diff(off.astype(np.int64))).all()
    w.close()


# ---- batches, capacities, repeatability ---------------------------------------------------------------------------------------------------------
def test_a_batch_whose_items_stride_the_grid():
    scene = S.grid_tiles(2, side=64, sphere_fraction=0.5, seed=2)
    w = E.World(scene, flags=FUSED)
    w.query_build()
    st = w.query_stats()
    assert st["runs"] >= 7 and st["top_nodes"] > 0
    entries = st["top_nodes"] + 1
    rec = _records(w, scene)
    # the kernel deals (region, entry) items to 8192 waves in chunks of at most 64: more items than that and the waves come round again
    n = (8192 * 64) // entries + 300
    rng = np.random.default_rng(51)
    regs = R.regions(_cubes(rng, n, rec, 1.0))
    regs["plane_count"][::5] = 3                                          # some half-open: more records, items that reach many entries
    _invalid(regs, rng)
    _, total = _same(w, rec, regs, f"{n} regions x {entries} entries")
    assert total > n
    w.close()


def test_capacity_writes_whole_segments_and_nothing_behind_them():
    scene = _three_runs()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    regs = _regions(np.random.default_rng(52), 257, rec)
    ref_off, _, total = R.region(rec, w.nbox, regs, capacity=0)
    nz = np.nonzero(np.diff(ref_off.astype(np.int64)) > 1)[0]
    boundary = int(ref_off[nz[len(nz) // 2]])                  # the start of a segment of at least two records: a cut between two segments
    for cap in (total, total - 1, boundary, boundary + 1, 0):
        _same(w, rec, regs, f"capacity {cap} of {total}", capacity=cap)
    # capacity 0 with a non-null hits buffer: count only, the buffer untouched
    off, hits = _gpu(w, regs, 0)
    assert off.tobytes() == ref_off.tobytes() and set(hits.tobytes()) == {SENTINEL}
    w.close()


def test_two_identical_calls_give_identical_bytes():
    scene = _three_runs()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    regs = _regions(np.random.default_rng(53), 257, rec)
    total = R.region(rec, w.nbox, regs, capacity=0)[2]
    assert total > 10000
    a, b = _gpu(w, regs, total), _gpu(w, regs, total)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    w.close()


def test_the_python_wrapper():
    scene = _three_runs()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    rng = np.random.default_rng(54)
    planes = _frusta(rng, 5, rec)
    ref_off, ref_hits, total = R.region(rec, w.nbox, R.regions(planes))
    r = w.region(planes, synchronize=True)
    assert r["offsets"].cpu().numpy().astype(np.uint32).tobytes() == ref_off.tobytes() and int(r["written"]) == total
    assert r["raw"].cpu().numpy().tobytes() == ref_hits[:total].tobytes()
    assert np.array_equal(r["query"].cpu().numpy(), np.repeat(np.arange(5), np.diff(ref_off.astype(np.int64))))
    # (P, 4) is one region; plane_counts and ignore_body go into the record
    body = int(ref_hits["body"][0])
    one = R.regions(planes[0], plane_counts=4, ignore_body=body)
    ref_off, ref_hits, total = R.region(rec, w.nbox, one)
    r = w.region(planes[0], plane_counts=4, ignore_body=body, capacity=total + 7, synchronize=True)
    assert int(r["written"]) == total and r["raw"].cpu().numpy()[:total].tobytes() == ref_hits[:total].tobytes()
    assert body not in r["body"].cpu().numpy()[:total]
    with pytest.raises(ValueError):
        w.region(np.zeros((1, 9, 4)))
    w.close()


# ---- layer masks ----------------------------------------------------------------------------------------------------------------------------------
def test_the_filter_off_uniform_and_per_query_equals_the_brute_force_over_the_masked_world():
    scene = _three_runs()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    rng = np.random.default_rng(55)
    regs = _regions(rng, 257, rec)
    words = F.layers(len(rec), 56)
    assert (words == 0).any()
    whole_off, whole = _same(w, rec, regs, "before any filter call")
    w.query_set_layers(words[:w.nbox], words[w.nbox:])
    _same(w, rec, regs, "layers set, filter off")
    for mask in F.MASKS:
        w.query_filter(mask)
        off, total = _same(w, F.masked(rec, words, mask), regs, f"uniform mask {mask:#x}")
        if mask == 0:
            assert total == 0 and not off.any()                           # mask 0 lists nothing
        elif mask != NONE:
            assert total < whole and (total > 0) == (mask != 0x80000000)  # (no collider carries bit 31)
    # per-query masks: region i under masks[i]
    values = (0, 1, 6, 0xFFFFFFFF)
    masks = rng.choice(np.uint32(values), size=len(regs))
    w.query_filter(_upload(w, masks).view(w.torch.int32))
    cnt, _ = _gpu(w, regs, None)
    sizes = np.zeros(len(regs), dtype=np.int64)
    parts = {}
    for v in values:
        o, h, _ = R.region(F.masked(rec, words, v), w.nbox, regs)
        sizes[masks == v] = np.diff(o.astype(np.int64))[masks == v]
        parts[v] = (o, h)
    ref_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    ref_hits = np.concatenate([parts[int(masks[i])][1][int(parts[int(masks[i])][0][i]):int(parts[int(masks[i])][0][i + 1])] for i in range(len(regs))])
    assert cnt.tobytes() == ref_off.tobytes()
    off, hits = _gpu(w, regs, len(ref_hits) + 5)
    assert off.tobytes() == ref_off.tobytes() and hits[:len(ref_hits)].tobytes() == ref_hits.tobytes() and set(hits[len(ref_hits):].tobytes()) == {SENTINEL}
    assert any(ref_off.tobytes() != parts[v][0].tobytes() for v in values)
    # all-ones layers with a mask, and the filter off again, give the filter-off bytes
    w.query_filter(5)
    w.query_set_layers(np.full(w.nbox, NONE, dtype=np.uint32), np.full(w.nsph, NONE, dtype=np.uint32))
    assert _same(w, rec, regs, "all-ones layers, mask 5")[0].tobytes() == whole_off.tobytes()
    w.query_set_layers(words[:w.nbox], words[w.nbox:])
    w.query_filter(None)
    assert _same(w, rec, regs, "filter off again")[0].tobytes() == whole_off.tobytes()
    w.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_abi_edge_cases():
    import torch
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    L = w.L
    rec = _records(w, scene)
    regs = _regions(np.random.default_rng(57), 64, rec)
    regs["plane_count"][regs["plane_count"] == 1] = 0                     # (the keep-everything planes: the records shall fit 4096)
    qt = _upload(w, regs)
    buf = torch.zeros(4 * 72, dtype=torch.int32, device=w.dev)
    ot = buf[:65]
    ht = torch.zeros((4096, 16), dtype=torch.uint8, device=w.dev)
    qp, op, hp = C.c_void_p(qt.data_ptr()), C.c_void_p(ot.data_ptr()), C.c_void_p(ht.data_ptr())
    assert L.nh_region(w.ctx, qp, 64, op, hp, 4096, 0) == 1                    # before any build: NH_ERR_INVALID
    assert L.nh_region(None, qp, 64, op, hp, 4096, 0) == 1
    w.query_build()
    assert L.nh_region(w.ctx, qp, 64, op, hp, 4096, 1) == 1                    # flags
    assert L.nh_region(w.ctx, None, 64, op, hp, 4096, 0) == 1                  # null / unaligned regions
    assert L.nh_region(w.ctx, C.c_void_p(qt.data_ptr() + 4), 63, op, hp, 4096, 0) == 1
    assert L.nh_region(w.ctx, qp, 64, None, hp, 4096, 0) == 1                  # null / unaligned offsets
    assert L.nh_region(w.ctx, qp, 64, C.c_void_p(ot.data_ptr() + 2), hp, 4096, 0) == 1
    assert L.nh_region(w.ctx, qp, 64, op, None, 4096, 0) == 1                  # null hits with a capacity, unaligned hits
    assert L.nh_region(w.ctx, qp, 64, op, C.c_void_p(ht.data_ptr() + 8), 4095, 0) == 1
    assert L.nh_region(w.ctx, qp, 1 << 30, op, hp, 4096, 0) == 1               # count >= 2^30: refused on the host, nothing launched
    assert L.nh_region(w.ctx, qp, 0xFFFFFFFF, op, hp, 4096, 0) == 1
    assert L.nh_region(w.ctx, qp, 0, op, hp, 4096, 0) == 0                     # count 0: a no-op
    assert L.nh_region(w.ctx, None, 0, None, None, 0, 0) == 0
    w.torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0 and int(ht.sum()) == 0                    # nothing was written
    # offsets need 4-byte alignment only
    ot4 = buf[1:66]
    assert L.nh_region(w.ctx, qp, 64, C.c_void_p(ot4.data_ptr()), hp, 4096, 0) == 0
    ref_off, ref_hits, total = R.region(rec, w.nbox, regs, capacity=4096, hits=sentinel_hits(4096, E.OVERLAP_HIT))
    assert 0 < total <= 4096
    assert ot4.cpu().numpy().view(np.uint32).tobytes() == ref_off.tobytes()
    got = np.frombuffer(ht.cpu().numpy().tobytes(), dtype=E.OVERLAP_HIT)
    assert got[:total].tobytes() == ref_hits[:total].tobytes() and not got[total:].view(np.uint8).any()
    assert int(buf[66:].abs().sum()) == 0 and int(buf[0]) == 0                 # count + 1 offsets and no word beside them
    w.close()


# ---- observers -----------------------------------------------------------------------------------------------------------------------------
def _observer_batch(a, scene):
    import torch
    a.query_build()
    rec = _records(a, scene)
    regs = _regions(np.random.default_rng(58), 64, rec)
    return _upload(a, regs), torch.empty(65, dtype=torch.int32, device=a.dev), torch.empty((1 << 15, 16), dtype=torch.uint8, device=a.dev)


def _query(w, qt, ot, ht):
    w.query_build()
    w.region_records(qt, offsets=ot)
    w.region_records(qt, offsets=ot, hits=ht, capacity=ht.shape[0])


def test_regions_between_nh_step_calls_change_nothing():
    LU.queries_between_nh_step_calls_change_nothing(OBSERVED["grid_tiles"], _observer_batch, _query, "grid_tiles", still=True)


def test_regions_between_every_call_of_the_fused_step_change_nothing():
    LU.queries_between_every_call_of_the_fused_step_change_nothing(OBSERVED["pile"], _observer_batch, _query, "pile", steps=120)
