"""What the layer-mask tests share (tests/test_cpu_filter.py, tests/test_gpu_filter.py; include/nudge_hip.h, "layer masks"): the layer assignment, the
masked world of the contract -- the records with a NaN position wherever (layers & mask) == 0 -- one batch of every query type, and the brute-force
answers of all nineteen calls to it, from the oracles the other query tests use.  Nothing here knows about the filter: the oracles only ever see a
world in which the rejected colliders cannot be hit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostcastk_util as HK                  # noqa: E402
import hostdistance_util as D                # noqa: E402
import hostnearest_util as N                 # noqa: E402
import hostpen_util as HPEN                  # noqa: E402
import test_gpu_closest as TP                # noqa: E402
import test_gpu_distance as TD               # noqa: E402
import test_gpu_overlap as TO                # noqa: E402
import test_gpu_penetration as TPEN          # noqa: E402
import test_gpu_refit as TR                  # noqa: E402
from cast_util import boxes, capsules, spheres      # noqa: E402
from query_util import bounds, rays as _rays, unit_quats    # noqa: E402

NONE = 0xFFFFFFFF
SENTINEL = 0xA5
MASKS = (0, 1, 2, 6, 0x80000000, 0xFFFFFFFF)
CAST_K = 3                                   # the k of the first-k casts
NEAR_K = 4                                   # the k of nh_closest_k
N_PER_KIND = 100                             # batch()'s n: 300 casts of each shape, 300 points, 300 overlap queries, 100 capsule overlaps
CASTS = ("rays", "spheres", "boxes", "capsules")
# seeds of the layer assignment and of the batch, per small scene: chosen so that test_cpu_filter's non-emptiness conditions hold
SEEDS = {"pile": (11, 900), "compound": (11, 901), "stacks": (11, 902), "grid_tiles": (11, 903), "ball_pit": (11, 904)}


def layers(n, seed):
    """One word per collider: each of bits 0 .. 3 set with probability 1/2 (a sixteenth of the words are 0: seen by no mask)."""
    rng = np.random.default_rng(seed)
    return ((rng.random((n, 4)) < 0.5) * np.uint32([1, 2, 4, 8])).sum(axis=1).astype(np.uint32)


def masked(rec, words, mask):
    """The masked world: `rec` with a NaN position wherever the query's mask sees nothing of the collider's word."""
    out = rec.copy()
    out["p"][(words & np.uint32(mask)) == 0] = np.nan
    return out


def batch(rng, rec, n=N_PER_KIND):
    """One batch of every query type around the colliders of `rec`, from the generators of the other query tests (test_gpu_refit's composition), the
    distance tests' shapes and the penetration tests' mixed queries."""
    lo, hi = bounds(rec)
    rays = np.concatenate([_rays(rng, n, lo, hi, kind) for kind in ("random", "axis", "down")])
    rays["max_t"] = rng.choice([np.inf, 5.0, 50.0], size=len(rays))
    # every other ray is turned towards the centre of a collider that is not the ground's: where one slab catches most random rays, half the world
    # going away would change few answers while it is seen and leave few hits while it is not
    live = np.nonzero(np.isfinite(rec["p"]).all(axis=1) & (rec["body"] != 0))[0]
    aimed = np.arange(0, len(rays), 2)
    d = rec["p"][rng.choice(live, size=len(aimed))].astype(np.float64) - rays["origin"][aimed]
    rays["direction"][aimed] = d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9) * rng.uniform(0.25, 4.0, size=(len(aimed), 1))
    rays["max_t"][aimed] = np.inf
    m = len(rays)
    points = np.concatenate([TP._points(rng, n, rec, lo, hi, kind) for kind in ("inside", "uniform", "above")])
    b = dict(
        rays=rays,
        spheres=spheres(rays, rng.choice(np.float32((0.05, 0.5, 2.0)), size=m)),
        boxes=boxes(rays, rng.choice(np.float32((0.05, 0.5, 2.0)), size=m), unit_quats(rng, m)),
        capsules=capsules(rays, rng.choice(np.float32([0.05, 0.5, 1.0]), size=m), rng.choice(np.float32([0.0, 0.5, 2.0]), size=m), unit_quats(rng, m)),
        points=TP._queries(points, max_distance=rng.choice(np.float32([np.inf, 0.5, 2.0]), size=len(points))),
        overlaps=np.concatenate([TO._queries(rng, n, rec, kind) for kind in ("sphere", "box", "mixed")]),
        capsule_overlaps=TO._capsule_queries(rng, n, rec))
    b["distances"] = np.concatenate([q for shape in TD.SHAPES for q in TD._batches(rng, shape, rec, n=24).values()])
    b["penetrations"] = TPEN._queries(rng, 3 * n, rec, "mixed")
    return b


def host(rec, nbox, b):
    """The brute-force answers of all nineteen calls to the batch `b` over `rec`.  Per-query answers are arrays (or (counts, rows)), list answers
    (offsets, records) with every segment complete."""
    out = TR._host(rec, nbox, b)
    out.pop("overlap_counts"); out.pop("capsule_counts")           # (the offsets of the lists: every segment is complete)
    for name in CASTS:
        seg = HK.segments(rec, nbox, b[name])
        out[name + "_all"] = seg
        out[name + "_k"] = HK.cast_k(rec, nbox, b[name], CAST_K, seg)
    out["points_k"] = N.closest_k(rec, nbox, b["points"], NEAR_K)
    out["distances"] = D.distance(rec, nbox, b["distances"])
    off, hits, total = HPEN.penetration(rec, nbox, b["penetrations"])
    out["penetrations"] = (off, hits[:total])
    out["overlap_list"] = (out["overlap_list"][0], out["overlap_list"][1][:int(out["overlap_list"][0][-1])])
    out["capsule_list"] = (out["capsule_list"][0], out["capsule_list"][1][:int(out["capsule_list"][0][-1])])
    return out


LISTS = ("overlap_list", "capsule_list", "penetrations") + tuple(c + "_all" for c in CASTS)
ROWS = tuple(c + "_k" for c in CASTS) + ("points_k",)
SINGLE = CASTS + ("points", "distances")


def differing(got, ref):
    """The names of the answers that differ in any byte."""
    out = []
    for k, r in ref.items():
        g = got[k]
        same = all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(g, r)) if isinstance(r, tuple) else g.tobytes() == r.tobytes()
        if not same:
            out.append(k)
    return out


def per_query(refs, masks, groups):
    """The answers to a batch whose query i carries masks[name][i]: query i's answer taken from refs[m], the answers of the whole batch under mask m,
    for m = its own mask.  `groups`: {answer name: batch name}."""
    out = {}
    any_ref = next(iter(refs.values()))
    for name in any_ref:
        m = masks[groups[name]]
        if name in SINGLE:
            out[name] = any_ref[name].copy()
            for v, r in refs.items():
                out[name][m == v] = r[name][m == v]
        elif name in ROWS:
            counts, rows = any_ref[name][0].copy(), any_ref[name][1].copy()
            for v, r in refs.items():
                counts[m == v] = r[name][0][m == v]
                rows[m == v] = r[name][1][m == v]
            out[name] = (counts, rows)
        else:
            size = np.zeros(len(m), dtype=np.int64)
            for v, r in refs.items():
                size[m == v] = np.diff(r[name][0].astype(np.int64))[m == v]
            off = np.concatenate([[0], np.cumsum(size)]).astype(np.uint32)
            parts = [refs[int(m[i])][name][1][int(refs[int(m[i])][name][0][i]):int(refs[int(m[i])][name][0][i + 1])] for i in range(len(m))]
            hits = np.concatenate(parts) if parts else any_ref[name][1][:0]
            out[name] = (off, hits)
    return out


GROUPS = dict(rays="rays", spheres="spheres", boxes="boxes", capsules="capsules", points="points", points_k="points", distances="distances",
              overlap_list="overlaps", capsule_list="capsule_overlaps", penetrations="penetrations",
              **{c + "_all": c for c in CASTS}, **{c + "_k": c for c in CASTS})


def shares(ref, base):
    """Of the answers `ref` beside the unfiltered answers `base`: (least share of hits, least share of records that differ) over the closest-hit casts and
    the point queries, and the overlap totals of both."""
    hit = min(float((ref[k]["shape"] != NONE).mean()) for k in CASTS + ("points",))
    diff = min(float((ref[k].view(np.uint8).reshape(len(ref[k]), -1) != base[k].view(np.uint8).reshape(len(base[k]), -1)).any(axis=1).mean())
               for k in CASTS + ("points",))
    totals = [(int(ref[k][0][-1]), int(base[k][0][-1])) for k in ("overlap_list", "capsule_list")]
    return hit, diff, totals
