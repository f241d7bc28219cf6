"""Layer masks on the host (no GPU): nh_query_set_layers / nh_query_filter / nh_query_layer_info of include/nudge_hip.h, "layer masks".

The GPU test compares every filtered call, byte for byte, with the host brute forces over the MASKED world -- the records with a NaN position wherever
(layers & mask) == 0.  What that comparison rests on is checked here without the feature: that a NaN position really is "removed" in every oracle it
leans on (the answers over the masked records equal the answers over a world from which those colliders were DELETED, indices mapped back), and that
under the GPU test's own layers and batches the comparison cannot be vacuous.  And the declarations and exports."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import filter_util as F                      # noqa: E402
import hostquery_util as Q                   # noqa: E402
from query_util import SMALL                 # noqa: E402
from nudge_amd import engine as E           # noqa: E402

NONE = 0xFFFFFFFF
NAMES = ("nh_query_set_layers", "nh_query_filter", "nh_query_layer_info")


# ---- declarations and exports -----------------------------------------------------------------------------------------------------------------
def test_the_three_entry_points_are_declared_exported_and_built():
    header = open(os.path.join(ROOT, "include", "nudge_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S)).replace(" ,", ",").replace(" )", ")")
    assert "int nh_query_set_layers(nh_context* ctx, const uint32_t* box_layers, const uint32_t* sphere_layers);" in flat
    assert "int nh_query_filter(nh_context* ctx, uint32_t mode, uint32_t mask, const uint32_t* masks);" in flat
    assert "int nh_query_layer_info(nh_context* ctx, nh_QueryLayerInfo* out);" in flat
    assert "enum { NH_FILTER_OFF = 0u, NH_FILTER_UNIFORM = 1u, NH_FILTER_PER_QUERY = 2u };" in flat
    assert "typedef struct nh_QueryLayerInfo { uint32_t set; uint32_t colliders; uint32_t any_layers; uint32_t reserved; } nh_QueryLayerInfo;" in flat
    assert set(NAMES) <= set(E.EXPORTS)
    assert (E.NH_FILTER_OFF, E.NH_FILTER_UNIFORM, E.NH_FILTER_PER_QUERY) == (0, 1, 2)
    # note 9's list of observers names them, and no "Not built" line says any more that filters by tag are missing
    note9 = next(line for line in header.splitlines() if "The scene queries (nh_query_build" in line)
    assert all(name in note9 for name in NAMES)
    assert not any("filters by tag" in line for line in header.splitlines() if "Not built" in line)
    so = os.path.join(ROOT, "nudge_amd", "libnudge_hip.so")
    if not os.path.exists(so):
        pytest.fail("nudge_amd/libnudge_hip.so is not built")
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    for name in NAMES:
        assert f" T {name}\n" in syms, name
    for method in ("query_set_layers", "query_filter", "query_layer_info"):
        assert callable(getattr(E.World, method)), method


# ---- the oracle's premise: a NaN position is a collider that is not there ---------------------------------------------------------------------------
def _world(name):
    scene = SMALL[name]()
    return Q.records(scene["body_transforms"], scene), len(scene["box_tags"])


def _mapped_back(ans, boxes, spheres):
    """The records of an answer over the compacted world with the collider indices of the whole one."""
    def fix(h):
        h = h.copy()
        if "collider" in (h.dtype.names or ()):
            box, sph = h["shape"] == E.NH_SHAPE_BOX, h["shape"] == E.NH_SHAPE_SPHERE
            c = h["collider"].copy()
            c[box] = boxes[h["collider"][box]]
            c[sph] = spheres[h["collider"][sph]]
            h["collider"] = c
        return h
    return {k: tuple(fix(x) for x in v) if isinstance(v, tuple) else fix(v) for k, v in ans.items()}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_a_nan_position_is_a_deleted_collider_in_every_oracle(name):
    rec, nbox = _world(name)
    rng = np.random.default_rng(880 + sorted(SMALL).index(name))
    b = F.batch(rng, rec)
    gone = rng.random(len(rec)) < 0.5
    nan = rec.copy()
    nan["p"][gone] = np.nan
    keep = np.nonzero(~gone)[0]
    boxes, spheres = keep[keep < nbox], keep[keep >= nbox] - nbox
    over_nan = F.host(nan, nbox, b)
    over_kept = _mapped_back(F.host(rec[keep], len(boxes), b), boxes, spheres)
    assert F.differing(over_nan, over_kept) == []
    # ... and the batch can tell: the whole world answers otherwise, in every one of the nineteen
    assert sorted(F.differing(F.host(rec, nbox, b), over_nan)) == sorted(over_nan)


# ---- the GPU comparison is not one of empty answers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SMALL))
def test_the_gpu_tests_layers_and_batches_hit_and_differ_under_every_single_bit_mask(name):
    rec, nbox = _world(name)
    layer_seed, batch_seed = F.SEEDS[name]
    words = F.layers(len(rec), layer_seed)
    assert (words == 0).any() and all((words & bit).any() for bit in (1, 2, 4, 8))
    b = F.batch(np.random.default_rng(batch_seed), rec)
    base = F.host(rec, nbox, b)
    for mask in (1, 2, 4, 8):
        hit, diff, totals = F.shares(F.host(F.masked(rec, words, mask), nbox, b), base)
        print(f"\n[{name} mask {mask}] least hit share {hit:.3f}, least differing share {diff:.3f}, overlap totals (masked, whole) {totals}", end="")
        assert hit >= 0.10 and diff >= 0.10, (name, mask, hit, diff)
        assert all(0 < masked < whole for masked, whole in totals), (name, mask, totals)


def test_the_per_query_assembly_is_the_single_mask_answer_where_every_query_has_that_mask():
    rec, nbox = _world("pile")
    words = F.layers(len(rec), F.SEEDS["pile"][0])
    b = F.batch(np.random.default_rng(5), rec, n=20)
    refs = {m: F.host(F.masked(rec, words, m), nbox, b) for m in (1, 6)}
    for m in (1, 6):
        masks = {k: np.full(len(b[k]), m, dtype=np.uint32) for k in set(F.GROUPS.values())}
        assert F.differing(F.per_query(refs, masks, F.GROUPS), refs[m]) == []
