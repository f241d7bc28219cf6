"""Layer masks on the GPU (pytest -m gpu): nh_query_set_layers / nh_query_filter / nh_query_layer_info (include/nudge_hip.h, "layer masks").

The contract is exact: with the filter on, a query with mask m writes what the same call writes, with the filter off, on the world in which every
collider with (layers & m) == 0 has a NaN pose.  So the oracle is the one the other query tests use -- the host brute forces with the device's
arithmetic -- over the MASKED records (tests/filter_util.py), and every comparison is byte for byte (any-hit casts: hit or miss).
tests/test_cpu_filter.py checks, without a GPU, that a NaN position is a deleted collider in each of those oracles and that the layers and batches
used here leave no comparison empty."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_util as F                      # noqa: E402
import hostcast_util as CAST                 # noqa: E402
import hostcastk_util as HK                  # noqa: E402
import hostquery_util as Q                   # noqa: E402
import test_gpu_closest as TP                # noqa: E402
import test_gpu_distance as TD               # noqa: E402
import test_gpu_nearest as TN                # noqa: E402
import test_gpu_overlap as TO                # noqa: E402
import test_gpu_penetration as TPEN          # noqa: E402
from cast_util import all_hits, box_casts, capsule_casts, casts_through, closest as _cast, coincident, first_k, sphere_casts      # noqa: E402
from query_util import OBSERVED, SMALL, bounds as _bounds, same_stepped_world as _same_stepped_world, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
FUSED = E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP
SENTINEL = F.SENTINEL
BIT31 = 0x80000000


def _records(w, scene):
    return Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)


def _set_layers(w, words):
    w.query_set_layers(words[:w.nbox], words[w.nbox:])


def _list(fn, w, queries, total):
    """A count-only call and a list call with room for exactly `total` records (the oracle's): the offsets of both must agree, nothing may be written
    behind the total.  Returns (offsets, the first `total` records)."""
    cnt, _ = fn(w, queries, None)
    off, hits = fn(w, queries, total)
    assert cnt.tobytes() == off.tobytes(), "list-mode offsets differ from the count-only ones"
    assert set(hits[total:].tobytes()) <= {SENTINEL}, "records behind the capacity were written"
    return off, hits[:total]


def _gpu(w, b, ref, before=lambda name: None):
    """The GPU's answers of all nineteen calls to the batch, in the layout of filter_util.host (the lists with the capacity of `ref`'s), and the
    any-hit answer of every cast shape as hit-or-miss.  `before(batch name)` runs ahead of the calls on that batch."""
    out, any_hit = {}, {}
    for name in F.CASTS:
        before(name)
        out[name] = _cast(w, b[name])
        any_hit[name] = _cast(w, b[name], any_hit=True)["shape"] != NONE
        out[name + "_all"] = _list(all_hits, w, b[name], len(ref[name + "_all"][1]))
        out[name + "_k"] = first_k(w, b[name], F.CAST_K)
        assert first_k(w, b[name], F.CAST_K, with_counts=False)[1].tobytes() == out[name + "_k"][1].tobytes(), f"{name}: counts = NULL writes other records"
    before("points")
    out["points"] = TP._closest(w, b["points"])
    out["points_k"] = TN._nearest(w, b["points"], F.NEAR_K)
    before("distances")
    out["distances"] = TD._distance(w, b["distances"])
    before("overlaps")
    out["overlap_list"] = _list(TO._gpu, w, b["overlaps"], len(ref["overlap_list"][1]))
    before("capsule_overlaps")
    out["capsule_list"] = _list(TO._gpu, w, b["capsule_overlaps"], len(ref["capsule_list"][1]))
    before("penetrations")
    out["penetrations"] = _list(TPEN._gpu, w, b["penetrations"], len(ref["penetrations"][1]))
    return out, any_hit


def _differing(w, b, ref, before=lambda name: None):
    """The names of the answers the GPU gives otherwise than `ref` (any-hit casts: in hit-or-miss)."""
    got, any_hit = _gpu(w, b, ref, before)
    return F.differing(got, ref) + [f"any-hit {name}" for name in F.CASTS if not np.array_equal(any_hit[name], ref[name]["shape"] != NONE)]


# ---- 1. all nineteen calls, uniform masks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SMALL))
def test_every_call_under_uniform_masks_equals_the_brute_force_over_the_masked_world(name):
    scene = SMALL[name]()
    layer_seed, batch_seed = F.SEEDS[name]
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    words = F.layers(len(rec), layer_seed)
    assert (words == 0).any()                                            # seen by no mask, but seen with the filter off
    b = F.batch(np.random.default_rng(batch_seed), rec)
    _set_layers(w, words)
    assert w.query_layer_info() == dict(set=1, colliders=len(rec), any_layers=int(np.bitwise_or.reduce(words)))
    whole = F.host(rec, w.nbox, b)
    for mask in F.MASKS:
        w.query_filter(mask)
        ref = F.host(F.masked(rec, words, mask), w.nbox, b)
        assert _differing(w, b, ref) == [], f"{name} mask {mask:#x}"
        if mask in (1, 2, 6):
            assert sorted(F.differing(ref, whole)) == sorted(ref), f"{name} mask {mask:#x}: the masked world answers as the whole one"
    w.query_filter(None)                                                  # off: the words of 0 are seen again
    assert _differing(w, b, whole) == [], f"{name} filter off"
    w.close()


# ---- 2. per-query masks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pile", "grid_tiles"])
def test_per_query_masks_mix_within_a_wave(name):
    scene = SMALL[name]()
    layer_seed, batch_seed = F.SEEDS[name]
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    words = F.layers(len(rec), layer_seed)
    rng = np.random.default_rng(batch_seed + 50)
    b = F.batch(rng, rec)
    values = (0, 1, 6, 0xFFFFFFFF)
    masks = {k: rng.choice(np.uint32(values), size=len(b[k])) for k in b}
    assert all(len(m) % 64 for m in masks.values())                      # no batch is whole waves
    tensors = {k: _upload(w, m).view(w.torch.int32) for k, m in masks.items()}
    _set_layers(w, words)
    refs = {v: F.host(F.masked(rec, words, v), w.nbox, b) for v in values}
    ref = F.per_query(refs, masks, F.GROUPS)
    assert _differing(w, b, ref, before=lambda k: w.query_filter(tensors[k])) == []
    assert all(F.differing(ref, refs[v]) for v in values)                # no single mask gives these answers
    w.close()


# ---- 3. a tree with a top phase ---------------------------------------------------------------------------------------------------------------------
def test_a_bit_of_one_collider_reaches_the_root_of_a_tree_of_several_runs():
    scene = S.grid_tiles(2, side=64, sphere_fraction=0.5, seed=2)
    w = E.World(scene, flags=FUSED)
    w.query_build()
    st = w.query_stats()
    assert st["colliders"] == 8194 and st["runs"] >= 7 and st["top_nodes"] >= st["runs"] - 1
    rec = _records(w, scene)
    n = len(rec)
    words = F.layers(n, 31)
    _set_layers(w, words)
    assert w.query_layer_info() == dict(set=1, colliders=n, any_layers=int(np.bitwise_or.reduce(words)))
    rng = np.random.default_rng(930)
    lo, hi = _bounds(rec)
    points = TP._queries(rng.uniform(lo - 5.0, hi + 5.0, size=(256, 3)))
    w.query_filter(BIT31)
    assert (TP._closest(w, points)["shape"] == NONE).all()               # nobody has the bit yet
    for c in (0, n - 1, 4 * st["run_length"] + st["run_length"] // 2 + 3):
        one = words.copy()
        one[c] |= BIT31
        _set_layers(w, one)
        assert w.query_layer_info()["any_layers"] == int(np.bitwise_or.reduce(one)), c
        shape, index = (E.NH_SHAPE_BOX, c) if c < w.nbox else (E.NH_SHAPE_SPHERE, c - w.nbox)
        near = TP._closest(w, points)
        assert (near["shape"] == shape).all() and (near["collider"] == index).all(), c
        assert near.tobytes() == TP.H.closest(F.masked(rec, one, BIT31), w.nbox, points).tobytes(), c
        # rays at it from 30 units away, through everything in front
        rays = casts_through(rec["p"][c], 256, rng)
        rays["origin"] = rec["p"][c] - 30.0 * rays["direction"]
        rays["ignore_body"] = NONE
        hits = _cast(w, rays)
        assert (hits["shape"] == shape).all() and (hits["collider"] == index).all(), c
        assert hits.tobytes() == CAST.cast(CAST.RAY, F.masked(rec, one, BIT31), w.nbox, rays).tobytes(), c
    w.close()


# ---- 4. identities ----------------------------------------------------------------------------------------------------------------------------------
def test_identities_off_all_ones_forgotten_layers_and_mask_zero():
    scene = SMALL["pile"]()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    words = F.layers(len(rec), 41)
    b = F.batch(np.random.default_rng(940), rec)
    whole = F.host(rec, w.nbox, b)
    before, _ = _gpu(w, b, whole)                                          # before any filter call
    assert F.differing(before, whole) == []
    _set_layers(w, words)
    w.query_filter(2)
    assert F.differing(_gpu(w, b, whole)[0], whole) != []
    w.query_filter(None)                                                   # OFF after UNIFORM
    assert F.differing(_gpu(w, b, whole)[0], before) == []
    w.query_filter(5)
    w.query_set_layers(np.full(w.nbox, NONE, dtype=np.uint32), np.full(w.nsph, NONE, dtype=np.uint32))
    assert F.differing(_gpu(w, b, whole)[0], before) == []                # all-ones layers, mask 5
    _set_layers(w, words)
    assert F.differing(_gpu(w, b, whole)[0], before) != []
    w.query_set_layers(None, None)                                         # forgotten: all ones again
    assert w.query_layer_info() == dict(set=0, colliders=len(rec), any_layers=NONE)
    assert F.differing(_gpu(w, b, whole)[0], before) == []
    # one NULL array: all ones for that shape
    w.query_set_layers(None, words[w.nbox:])
    half = words.copy()
    half[:w.nbox] = NONE
    assert _differing(w, b, F.host(F.masked(rec, half, 5), w.nbox, b)) == []
    # mask 0 sees nothing, with layers or without: misses with t = max_t (max_distance), empty segments, counts 0 -- and nothing outside the records
    for set_them in (True, False):
        if set_them:
            _set_layers(w, words)
        else:
            w.query_set_layers(None, None)
        w.query_filter(0)
        nothing = F.host(F.masked(rec, words, 0), w.nbox, b)
        assert all((nothing[k]["shape"] == NONE).all() for k in F.SINGLE) and all(int(nothing[k][0][-1]) == 0 for k in F.LISTS)
        assert all((nothing[k][0] == 0).all() for k in F.ROWS)
        valid = np.isfinite(b["rays"]["origin"]).all(axis=1) & np.isfinite(b["rays"]["direction"]).all(axis=1)
        assert (nothing["rays"]["t"][valid].view(np.uint32) == b["rays"]["max_t"][valid].view(np.uint32)).all()
        assert _differing(w, b, nothing) == []
        torch = w.torch
        for call, queries, size in ((w.raycast_records, b["rays"], 32), (w.closest_records, b["points"], 48), (w.distance_records, b["distances"], 48)):
            ht = torch.full((len(queries) + 64, size), SENTINEL, dtype=torch.uint8, device=w.dev)
            call(_upload(w, queries), hits=ht)
            assert set(ht[len(queries):].cpu().numpy().tobytes()) == {SENTINEL}
    w.close()


# ---- 5. refit and rebuild -----------------------------------------------------------------------------------------------------------------------------
def test_layers_follow_the_collider_through_a_refit_and_a_rebuild_and_are_forgotten_with_the_counts():
    scene = SMALL["pile"]()
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec0 = _records(w, scene)
    words = F.layers(len(rec0), 51)
    _set_layers(w, words)
    w.query_filter(6)
    w.step(20)
    w.query_refit()
    rec = _records(w, scene)
    assert rec.tobytes() != rec0.tobytes()
    b = F.batch(np.random.default_rng(950), rec)
    assert _differing(w, b, F.host(F.masked(rec, words, 6), w.nbox, b)) == [], "after a refit"
    # a third of the bodies change sides: another Morton order, another tree; the layers are the colliders', not the leaves'
    bt = w.get_bodies()["transforms"].copy()
    lo, hi = _bounds(rec)
    moved = np.arange(1, nb, 3)
    bt["position"][moved, 0] = np.float32(lo[0] + hi[0]) - bt["position"][moved, 0]
    bt["position"][moved, 2] = np.float32(lo[2] + hi[2]) - bt["position"][moved, 2]
    w.set_bodies(transforms=bt)
    w.torch.cuda.synchronize()
    w.query_build()                                                        # no new set_layers
    assert w.query_layer_info() == dict(set=1, colliders=len(rec), any_layers=int(np.bitwise_or.reduce(words)))
    rec = _records(w, scene)
    b = F.batch(np.random.default_rng(951), rec)
    for mask in (6, 1):
        w.query_filter(mask)
        assert _differing(w, b, F.host(F.masked(rec, words, mask), w.nbox, b)) == [], f"after a rebuild, mask {mask}"
    # other counts are another world: the layers are forgotten, a non-zero mask sees everything
    w.set_counts(nb, w.nbox - 3, w.nsph - 2)
    w.query_build()
    rec = _records(w, scene)
    assert w.query_layer_info() == dict(set=0, colliders=len(rec), any_layers=NONE)
    b = F.batch(np.random.default_rng(952), rec)
    assert _differing(w, b, F.host(rec, w.nbox, b)) == [], "layers forgotten"
    w.close()


# ---- 6. ties --------------------------------------------------------------------------------------------------------------------------------------------
def test_ties_through_4096_coincident_boxes_go_to_the_lowest_index_the_mask_sees():
    scene = coincident(4096)
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = _records(w, scene)
    words = np.where(np.arange(len(rec)) % 2 == 0, 1, 2).astype(np.uint32)
    _set_layers(w, words)
    w.query_filter(2)
    masked = F.masked(rec, words, 2)
    rng = np.random.default_rng(960)
    rays = casts_through((0.25, 3.0, -0.5), 64, rng)
    batches = {"rays": rays, "spheres": sphere_casts(rays, invalid=False), "boxes": box_casts(rng, rays, invalid=False),
               "capsules": capsule_casts(rng, rays, invalid=False)}
    for name, casts in batches.items():
        best = _cast(w, casts)
        assert (best["shape"] == E.NH_SHAPE_BOX).all() and (best["collider"] == 1).all(), name
        counts, hits = first_k(w, casts, 32)
        assert (counts == 32).all() and (hits["collider"] == np.arange(1, 65, 2)).all(), name
        assert hits[:, 0].tobytes() == best.tobytes(), name
        off, _ = all_hits(w, casts, None)
        assert (np.diff(off.astype(np.int64)) == 2048).all(), name
        ref_counts, ref_hits = HK.cast_k(masked, w.nbox, casts, 32)
        assert counts.tobytes() == ref_counts.tobytes() and hits.tobytes() == ref_hits.tobytes(), name
    w.close()


# ---- 7. with ignore_body and NaN poses ------------------------------------------------------------------------------------------------------------------
def test_the_filter_composes_with_ignore_body_and_nan_poses():
    scene = SMALL["pile"]()
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    w.set_counts(nb - 10, w.nbox, w.nsph)                  # the last 10 spheres belong to bodies that no longer exist: NaN poses
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"][: nb - 10], scene, w.nbox, w.nsph)
    assert np.isnan(rec["p"][-10:]).all() and np.isfinite(rec["p"][:-10]).all()
    words = F.layers(len(rec), 71)
    words[-10:] = 0xF                                       # every mask would see them
    rng = np.random.default_rng(970)
    b = F.batch(rng, rec)
    live = np.nonzero(np.isfinite(rec["p"]).all(axis=1))[0]
    for k in b:
        b[k]["ignore_body"][::3] = rec["body"][rng.choice(live, size=len(b[k]["ignore_body"][::3]))]
    _set_layers(w, words)
    for mask in (1, 6):
        w.query_filter(mask)
        ref = F.host(F.masked(rec, words, mask), w.nbox, b)
        assert _differing(w, b, ref) == [], mask
        for k in F.CASTS + ("points", "distances"):
            hit = ref[k]["shape"] != NONE
            assert hit.mean() > 0.1 and not (ref[k]["body"][hit] == b[k]["ignore_body"][hit]).any(), k
            assert not ((ref[k]["shape"] == E.NH_SHAPE_SPHERE) & (ref[k]["collider"] >= w.nsph - 10)).any(), k
    w.close()


# ---- 8. ABI -----------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_edge_cases():
    scene = SMALL["pile"]()
    w = E.World(scene, flags=FUSED)
    torch = w.torch
    L = w.L
    n = w.nbox + w.nsph
    words = F.layers(n, 81)
    lt = _upload(w, np.concatenate([words, np.zeros(4, np.uint32)])).view(torch.int32)
    ptr = lambda t, byte=0: C.c_void_p(t.data_ptr() + byte)               # noqa: E731
    info = E.QueryLayerInfo()
    # before any build: NH_ERR_INVALID from all three
    assert L.nh_query_set_layers(w.ctx, ptr(lt), ptr(lt, 4 * w.nbox)) == 1
    assert L.nh_query_filter(w.ctx, E.NH_FILTER_UNIFORM, 1, None) == 1 and L.nh_query_filter(w.ctx, E.NH_FILTER_OFF, 0, None) == 1
    assert L.nh_query_layer_info(w.ctx, C.byref(info)) == 1
    w.query_build()
    assert L.nh_query_set_layers(None, ptr(lt), ptr(lt, 4 * w.nbox)) == 1 and L.nh_query_filter(None, 0, 0, None) == 1
    assert L.nh_query_layer_info(w.ctx, None) == 1 and L.nh_query_layer_info(None, C.byref(info)) == 1
    rec = _records(w, scene)
    b = F.batch(np.random.default_rng(980), rec)
    _set_layers(w, words)
    w.query_filter(2)
    ref = F.host(F.masked(rec, words, 2), w.nbox, b)
    assert _differing(w, b, ref) == []
    # refused calls: an unknown mode, PER_QUERY with NULL or a misaligned pointer, misaligned layer arrays
    assert L.nh_query_filter(w.ctx, 3, 1, None) == 1 and L.nh_query_filter(w.ctx, 0xFFFFFFFF, 1, ptr(lt)) == 1
    assert L.nh_query_filter(w.ctx, E.NH_FILTER_PER_QUERY, 1, None) == 1
    for byte in (1, 2, 3):
        assert L.nh_query_filter(w.ctx, E.NH_FILTER_PER_QUERY, 1, ptr(lt, byte)) == 1
        assert L.nh_query_set_layers(w.ctx, ptr(lt, byte), ptr(lt, 4 * w.nbox)) == 1
        assert L.nh_query_set_layers(w.ctx, ptr(lt), ptr(lt, 4 * w.nbox + byte)) == 1
        assert L.nh_query_set_layers(w.ctx, None, ptr(lt, byte)) == 1
    # ... change no state: the next queries still use the previous layers and filter
    assert w.query_layer_info() == dict(set=1, colliders=n, any_layers=int(np.bitwise_or.reduce(words)))
    assert _differing(w, b, ref) == []
    # count = 0 under every mode: NH_OK, nothing written
    masks = _upload(w, np.full(1024, 1, np.uint32)).view(torch.int32)
    ht = torch.full((64, 48), SENTINEL, dtype=torch.uint8, device=w.dev)
    ot = torch.full((64,), -1, dtype=torch.int32, device=w.dev)
    for mode, mask, mp in ((E.NH_FILTER_OFF, 0, None), (E.NH_FILTER_UNIFORM, 2, None), (E.NH_FILTER_UNIFORM, 0, None), (E.NH_FILTER_PER_QUERY, 0, ptr(masks))):
        assert L.nh_query_filter(w.ctx, mode, mask, mp) == 0
        for fn in (L.nh_raycast, L.nh_spherecast, L.nh_boxcast, L.nh_capsulecast, L.nh_closest, L.nh_distance):
            assert fn(w.ctx, ptr(ht), 0, ptr(ht), 0) == 0 and fn(w.ctx, None, 0, None, 0) == 0
        for fn in (L.nh_raycast_k, L.nh_spherecast_k, L.nh_boxcast_k, L.nh_capsulecast_k, L.nh_closest_k):
            assert fn(w.ctx, ptr(ht), 0, 4, ptr(ot), ptr(ht), 0) == 0
        for fn in (L.nh_overlap, L.nh_penetration, L.nh_raycast_all, L.nh_spherecast_all, L.nh_boxcast_all, L.nh_capsulecast_all):
            assert fn(w.ctx, ptr(ht), 0, ptr(ot), ptr(ht), 64, 0) == 0
    torch.cuda.synchronize()
    assert set(ht.cpu().numpy().tobytes()) == {SENTINEL} and (ot.cpu().numpy() == -1).all()
    # the Python wrapper: numpy or torch layers, an int or a tensor as the filter
    w.query_set_layers(torch.from_numpy(words[:w.nbox].astype(np.int64)), lt[w.nbox:n])
    w.query_filter(masks[:len(b["rays"])])
    assert _cast(w, b["rays"]).tobytes() == F.host(F.masked(rec, words, 1), w.nbox, b)["rays"].tobytes()
    with pytest.raises(ValueError):
        w.query_set_layers(words[:5], None)
    w.close()


# ---- 9. observers -----------------------------------------------------------------------------------------------------------------------------------------
class _Observer:
    """Layers, filters and filtered calls of several kinds on buffers allocated once."""

    def __init__(self, w, scene):
        torch = w.torch
        rec = Q.records(scene["body_transforms"], scene)
        rng = np.random.default_rng(990)
        b = F.batch(rng, rec, n=128)
        words = F.layers(len(rec), 91)
        self.w = w
        bits = lambda words: torch.from_numpy(words.view(np.int32).copy()).to(w.dev)          # noqa: E731
        self.box_layers, self.sphere_layers = bits(words[:w.nbox]), bits(words[w.nbox:])
        self.rays, self.points, self.overlaps = _upload(w, b["rays"]), _upload(w, b["points"]), _upload(w, b["overlaps"])
        self.masks = bits(rng.choice(np.uint32([0, 1, 2, 6]), size=len(b["rays"])))
        self.hits = torch.empty((len(b["rays"]) * 4, 48), dtype=torch.uint8, device=w.dev)
        self.offsets = torch.empty(len(b["overlaps"]) + 1, dtype=torch.int32, device=w.dev)
        self.turn = 0

    def __call__(self):
        w, turn = self.w, self.turn
        self.turn += 1
        if turn % 4 == 0:
            w.query_build()
        else:
            w.query_refit()
        if turn % 3 == 0:
            w.query_set_layers(self.box_layers, self.sphere_layers)
        elif turn % 3 == 1:
            w.query_set_layers(None, self.sphere_layers if w.nsph else None)
        w.query_filter((2, self.masks, None, 0, 6)[turn % 5])
        w.raycast_records(self.rays, hits=self.hits)
        w.raycast_k_records(self.rays, 4, hits=self.hits)
        w.closest_records(self.points, hits=self.hits)
        w.overlap_records(self.overlaps, offsets=self.offsets)
        if turn % 7 == 0:
            w.query_layer_info()


@pytest.mark.parametrize("name", sorted(OBSERVED))
def test_layers_filters_and_filtered_calls_between_calls_change_nothing(name):
    scene = OBSERVED[name]()
    # between nh_step calls
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    observe = _Observer(a, scene)
    done = 0
    for k in [1, 2, 3, 5, 7, 4, 8] * 5:
        k = min(k, 150 - done)
        if k <= 0:
            break
        observe()
        a.step(k)
        b.step(k)
        done += k
    observe()
    _same_stepped_world(a, b, f"{name} nh_step")
    a.close(); b.close()
    # between every pair of entry points of the fused step
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    observe = _Observer(a, scene)
    for s in range(100):
        for call in ("collide", "gravity", "read_cache", "setup", "apply", "update", "write_cache", "advance"):
            observe()
            getattr(a, call)()
            getattr(b, call)()
        a.step_done(); b.step_done()
    observe()
    _same_stepped_world(a, b, f"{name} call by call")
    a.close(); b.close()
