"""What the layer masks cost and buy on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "layer masks"): 1,048,576
incoherent queries of nh_raycast, nh_spherecast (r 0.75), nh_overlap (count only, spheres of radius 1) and nh_closest, each timed four ways in the
same process on the same records --
    off        NH_FILTER_OFF
    mask 3     NH_FILTER_UNIFORM, sees every collider: the price of the filtered walk
    mask 1     NH_FILTER_UNIFORM, sees the static world only: what pruning by node words buys
    per query  NH_FILTER_PER_QUERY, masks alternating 1 / 2: neighbouring lanes of a wave see different worlds
with the dynamic boxes in layer 2 and body 0's colliders in layer 1 -- device events, interleaved, the median [min .. max] of --repeats blocks of
--reps calls after two warm-ups.  Also nh_query_set_layers, and nh_query_build with and without layers.  256 rays and points per way are compared byte
for byte with the brute force over the masked world.
With NUDGE_HIP_LIBRARY naming another build of the library (the parent commit's), a second world on THAT library is stepped and built in the same
process, and the four calls with the filter off are timed on both, alternating: this library beside the other, and the other beside itself (two
timings of it per block: the spread repeated runs of one library show).

    [NUDGE_HIP_LIBRARY=.../libparent.so] python tools/filter_rates.py [--steps 70] [--reps 10] [--repeats 5] [--out profiles/filter_rates.log]
    (on a GPU box; prints the table, one JSON line at the end, and writes both to --out)
"""
import json
import os
import sys

import numpy as np

import rates
OTHER = rates.other_library()
from nudge_amd import engine as E           # noqa: E402

NONE = rates.NONE
WAYS = ("off", "mask 3", "mask 1", "per query")


def main():
    ap = rates.parser("filter_rates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--no-check", action="store_true", help="skip the brute-force spot check")
    a = ap.parse_args()
    import torch
    land = rates.landed(a)
    other = rates.landed(a, OTHER, like=land).world if OTHER else None
    w, C, n, scene, lo, hi = land.world, land.colliders, a.queries, land.scene, land.lo, land.hi
    up, log = rates.upload, rates.Log()

    def interleaved(fns):
        return rates.spreads(rates.interleaved(w, fns, a.reps, a.repeats))

    # the incoherent rays of tools/query_rates.py (the same seed); the other calls take their origins
    rng = np.random.default_rng(1)
    rays, _ = rates.ray_sets(rng, n, lo, hi)
    balls = rates.cast_records(rays, E.SPHERE_CAST, radius=0.75)
    near = rng.uniform(lo, hi + np.array([0, 6, 0]), size=(n, 3))          # where the bodies lie
    overlaps = rates.overlap_queries(near, (1.0, 0.0, 0.0), E.NH_SHAPE_SPHERE)
    points = rates.point_queries(rays["origin"], np.inf)

    words = np.where(np.concatenate([scene["box_transforms"]["body"], scene["sphere_transforms"]["body"]]) == 0, 1, 2).astype(np.uint32)
    box_layers, sphere_layers = up(w, words[:w.nbox]).view(torch.int32), (up(w, words[w.nbox:]).view(torch.int32) if w.nsph else None)
    alternating = up(w, np.where(np.arange(n) % 2 == 0, 1, 2).astype(np.uint32)).view(torch.int32)
    filters = {"off": None, "mask 3": 3, "mask 1": 1, "per query": alternating}

    def calls(world):
        rt, bt, ot_, pt = up(world, rays), up(world, balls), up(world, overlaps), up(world, points)
        hits = torch.empty((n, 48), dtype=torch.uint8, device=world.dev)
        offsets = torch.empty(n + 1, dtype=torch.int32, device=world.dev)
        return {"nh_raycast": lambda: world.raycast_records(rt, hits=hits), "nh_spherecast r=.75": lambda: world.spherecast_records(bt, hits=hits),
                "nh_overlap count, r=1": lambda: world.overlap_records(ot_, offsets=offsets), "nh_closest": lambda: world.closest_records(pt, hits=hits)}

    mine = calls(w)
    w.query_set_layers(box_layers, sphere_layers)
    info = w.query_layer_info()
    assert info["set"] == 1 and info["any_layers"] == 3, info

    def filtered(call, way):
        def fn():
            w.query_filter(filters[way])
            call()
        return fn

    rows = {}
    for name, call in mine.items():
        t = interleaved({way: filtered(call, way) for way in WAYS})
        rows[name] = dict(ways=t, over_off={way: t[way]["ms"] / t["off"]["ms"] for way in WAYS})
        print(f"timed: {name}", file=sys.stderr, flush=True)
    w.query_filter(None)

    # the layer pass, and the build with and without it
    w.query_set_layers(None, None)
    t_plain = interleaved({"build": w.query_build})["build"]
    w.query_set_layers(box_layers, sphere_layers)
    t_layers = interleaved({"set_layers": lambda: w.query_set_layers(box_layers, sphere_layers), "build": w.query_build, "refit": w.query_refit})
    w.query_set_layers(None, None)
    t_refit = interleaved({"refit": w.query_refit})["refit"]
    passes = dict(set_layers=t_layers["set_layers"], build_with_layers=t_layers["build"], build_without=t_plain, refit_with_layers=t_layers["refit"], refit_without=t_refit)

    checked = 0
    if not a.no_check:
        import filter_util as F
        import hostcast_util as CAST
        import hostpoint_util as HP
        rec = land.records
        pick = np.sort(np.random.default_rng(3).choice(n // 2, size=128, replace=False)) * 2
        pick = np.sort(np.concatenate([pick, pick + 1]))
        w.query_set_layers(box_layers, sphere_layers)
        for way, flt in filters.items():
            w.query_filter(flt)
            got_r = rates.download(w.raycast_records(up(w, rays)), E.RAY_HIT)[pick]
            got_p = rates.download(w.closest_records(up(w, points)), E.POINT_HIT)[pick]
            # the mask of every picked query (off: none -- the whole world)
            mvals = np.zeros(len(pick), np.uint32) if flt is None else np.full(len(pick), flt, np.uint32) if isinstance(flt, int) else np.where(pick % 2 == 0, 1, 2).astype(np.uint32)
            for m in np.unique(mvals):
                sel = mvals == m
                world_m = rec if flt is None else F.masked(rec, words, m)
                assert got_r[sel].tobytes() == CAST.cast(CAST.RAY, world_m, w.nbox, rays[pick][sel]).tobytes(), f"{way}: rays differ from the brute force"
                assert got_p[sel].tobytes() == HP.closest(world_m, w.nbox, points[pick][sel]).tobytes(), f"{way}: closest points differ from the brute force"
                checked += 2 * int(sel.sum())
        w.query_filter(None)

    ab = None
    if other is not None:
        theirs = calls(other)
        ab = {}
        for name in mine:
            t = interleaved({"other (a)": theirs[name], "this": mine[name], "other (b)": theirs[name]})
            ab[name] = dict(t, this_over_other=t["this"]["ms"] / (0.5 * (t["other (a)"]["ms"] + t["other (b)"]["ms"])), other_over_itself=t["other (b)"]["ms"] / t["other (a)"]["ms"])

    fmt = rates.fmt
    log.say(f"landed {land.name} world: {C:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; GPU {rates.gpu_name(w)}")
    log.say(f"{n:,} incoherent queries per call; dynamic boxes in layer 2, body 0's colliders in layer 1; median of {a.repeats} blocks of {a.reps} calls, "
            f"interleaved (min .. max of the blocks); one box, one run; {checked} records equal the brute force over the masked world byte for byte")
    log.say()
    log.say(f"{'call':<24}" + "".join(f"{way + ' ms':>28}" for way in WAYS) + "".join(f"{way + ' / off':>16}" for way in WAYS[1:]))
    for name, v in rows.items():
        log.say(f"{name:<24}" + "".join(f"{fmt(v['ways'][way]):>28}" for way in WAYS) + "".join(f"{v['over_off'][way]:16.3f}" for way in WAYS[1:]))
    log.say()
    log.say("the layer pass, and the tree with and without layers (ms):")
    for key, v in passes.items():
        log.say(f"  {key:<22}{fmt(v):>28}")
    log.say()
    if ab is None:
        log.say("filter off, this library beside another build: no NUDGE_HIP_LIBRARY given, not measured")
    else:
        log.say(f"filter off, this library beside {os.path.basename(OTHER)} in the same process (ms):")
        log.say(f"{'call':<24}{'other (a)':>28}{'this':>28}{'other (b)':>28}{'this / other':>14}{'other b / a':>14}")
        for name, v in ab.items():
            log.say(f"{name:<24}{fmt(v['other (a)']):>28}{fmt(v['this']):>28}{fmt(v['other (b)']):>28}{v['this_over_other']:14.3f}{v['other_over_itself']:14.3f}")
    log.say()
    log.say(json.dumps(dict(colliders=C, steps=a.steps, queries=n, calls=rows, passes=passes, off_beside_other=ab, checked=checked)))
    log.write(a.out)
    w.close()
    if other is not None:
        other.close()


if __name__ == "__main__":
    main()
