"""nh_region rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "nh_region"), and beside them in the same
process the only tool there was for a large question, nh_overlap with a large box.  Per case the count-only call and the count + exactly sized list
call, ms per call as the best of --reps blocks of --inner calls after a warm-up, by device events around the block (the nh_overlap twins one call a
block); then one more call of each with nh_enable_timing for the per-label
breakdown (q_region_count, q_region_list, the scan, the sort, q_overlap_gather).

    (a) one six-plane region that is the world's AABB                     beside nh_overlap with one box query equal to that AABB (one lane walks it all)
    (b) one perspective frustum that sees about a tenth of the colliders  (its far plane found by bisection on the count)
    (c) 64 such frusta, eyes on a ring around the world
    (d) 4,096 cubes of one tile's size around random bodies               beside nh_overlap with the same cubes as box queries (a lane per cube)

The two nh_overlap calls are existing calls: they say which call is for which size of question.  Totals of a region and its nh_overlap twin are
compared; they may differ by the few colliders near edges and corners that the plane-by-plane test keeps and the box test does not.

    python tools/region_rates.py [--steps 70] [--reps 5] [--inner 20] [--out profiles/region_rates.log]
    (on a GPU box; prints the table, one JSON line at the end, and writes both to --out)
"""
import json

import numpy as np

import rates
from rates import box_planes
from nudge_amd import engine as E           # noqa: E402


def camera(eye, target, fov_deg, aspect, near, far):
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, (0.0, 1.0, 0.0))
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    view = np.eye(4)
    view[0, :3], view[1, :3], view[2, :3] = right, up, -fwd
    view[:3, 3] = -view[:3, :3] @ eye
    f = 1.0 / np.tan(np.radians(fov_deg) / 2)
    proj = np.array([[f / aspect, 0, 0, 0], [0, f, 0, 0], [0, 0, (far + near) / (near - far), 2 * far * near / (near - far)], [0, 0, -1, 0]])
    return E.frustum_planes(proj @ view)


def main():
    ap = rates.parser("region_rates")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="nh_region calls per timed block (the nh_overlap twins are timed one call at a time)")
    ap.add_argument("--walk-reps", type=int, default=1, help="calls of the one-lane nh_overlap twin of (a): each takes seconds")
    ap.add_argument("--cubes", type=int, default=4096)
    a = ap.parse_args()
    import hostregion_util as R
    land = rates.landed(a)
    w, rec = land.world, land.records
    st = w.query_stats()
    log = rates.Log()
    C = len(rec)
    lo, hi = rates.reach_bounds(rec)
    dyn = rec["p"][rec["body"] != 0].astype(np.float64)
    dlo, dhi = dyn.min(axis=0), dyn.max(axis=0)
    tile_size = rates.tile_size(land.scene, w.get_bodies()["transforms"]["position"])

    def count_of(planes):
        off, _ = w.region_records(rates.upload(w, R.regions(planes)))
        return rates.total_of(off)

    # (b): from outside a corner of the world, looking at its middle; the far plane by bisection on the count
    mid = 0.5 * (dlo + dhi)
    eye = np.array([dlo[0] - 20.0, dhi[1] + 40.0, dlo[2] - 20.0])
    near, f_lo, f_hi = 1.0, 2.0, 2.0 * float(np.linalg.norm(hi - lo))
    for _ in range(24):
        far = 0.5 * (f_lo + f_hi)
        if count_of(camera(eye, mid, 50.0, 1.6, near, far)) < C // 10:
            f_lo = far
        else:
            f_hi = far
    far = f_hi
    rng = np.random.default_rng(1)
    ring = []
    radius = 0.5 * float(np.linalg.norm((dhi - dlo)[[0, 2]])) + 20.0
    for k in range(64):
        ang = 2 * np.pi * k / 64
        e = mid + np.array([radius * np.cos(ang), dhi[1] - mid[1] + 40.0, radius * np.sin(ang)])
        ring.append(camera(e, mid + rng.normal(scale=5.0, size=3), 50.0, 1.6, near, far))
    centres = dyn[rng.integers(0, len(dyn), size=a.cubes)]
    half = 0.5 * tile_size
    cases = {
        "a": R.regions(box_planes(lo, hi)),
        "b": R.regions(camera(eye, mid, 50.0, 1.6, near, far)),
        "c": R.regions(np.stack(ring)),
        "d": R.regions(box_planes(centres - half, centres + half)),
    }
    twins = {"a": rates.overlap_queries([0.5 * (lo + hi)], [0.5 * (hi - lo)], E.NH_SHAPE_BOX),
             "d": rates.overlap_queries(centres, np.full((a.cubes, 3), half), E.NH_SHAPE_BOX)}

    def measure(records, q, reps, inner, breakdown=True):
        return rates.count_then_list(w, records, rates.upload(w, q), len(q), 16, reps, inner, breakdown)[0]

    log.say(f"landed {land.name} world: {C:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; {st['runs']} runs, {st['top_nodes'] + 1} entry nodes; "
            f"GPU {rates.gpu_name(w)}")
    log.say(f"ms per call: the best of {a.reps} blocks of {a.inner} calls after a warm-up, device events around the block; one box, one run.  "
            f"tile size {tile_size:.1f}, frustum far plane {far:.1f}")
    log.say(f"  {'case':58s} {'regions':>8s} {'records':>11s} {'count ms':>10s} {'count+list ms':>14s}")
    names = {"a": "(a) nh_region, the world's AABB", "b": "(b) nh_region, a frustum that sees a tenth", "c": "(c) nh_region, 64 such frusta",
             "d": f"(d) nh_region, {a.cubes:,} cubes of a tile's size"}
    out = {}
    for key, regs in cases.items():
        r = measure(w.region_records, regs, a.reps, a.inner)
        out[key] = dict(regions=len(regs), **r)
        log.say(f"  {names[key]:58s} {len(regs):8,d} {r['records']:11,d} {r['count_ms']:10.3f} {r['list_ms']:14.3f}   (medians {r['count_median_ms']:.3f}, {r['list_median_ms']:.3f})")
        log.say(f"      labels of count + list, ms: {r['labels']}")
        if key in twins:
            reps = a.walk_reps if key == "a" else a.reps
            o = measure(w.overlap_records, twins[key], reps, 1, breakdown=key != "a")
            out[key + "_overlap"] = dict(queries=len(twins[key]), **o)
            log.say(f"  {'    nh_overlap, the same as box queries (%d x 1 call)' % reps:58s} {len(twins[key]):8,d} {o['records']:11,d} {o['count_ms']:10.3f} {o['list_ms']:14.3f}"
                    f"   (medians {o['count_median_ms']:.3f}, {o['list_median_ms']:.3f})")
            fewer = "" if o["records"] == r["records"] else f"   (the box test lists {r['records'] - o['records']:,} fewer: edges and corners)"
            log.say(f"      nh_overlap / nh_region: count {o['count_ms'] / r['count_ms']:.1f} x, count + list {o['list_ms'] / r['list_ms']:.1f} x{fewer}")
    assert out["a"]["records"] == C, "the world's AABB does not hold every collider"
    # 3 regions of (c) and 8 of (d), byte for byte against the brute force over all colliders
    import torch
    pick = np.concatenate([cases["c"][:3], cases["d"][:8]])
    ref_off, ref_hits, total = R.region(rec, w.nbox, pick)
    ot, ht = w.region_records(rates.upload(w, pick), hits=torch.empty((total, 16), dtype=torch.uint8, device=w.dev), capacity=total)
    assert ot.cpu().numpy().view(np.uint32).tobytes() == ref_off.tobytes() and ht.cpu().numpy().tobytes() == ref_hits[:total].tobytes(), "the GPU differs from the brute force"
    log.say(f"  {len(pick)} regions ({total:,} records) equal the brute force byte for byte")
    log.say()
    log.say(json.dumps(dict(colliders=C, steps=a.steps, entries=st["top_nodes"] + 1, **out)))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
