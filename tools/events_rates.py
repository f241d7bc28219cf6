"""nh_overlap_bodies / nh_overlap_events rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "trigger
events"), each beside the list call that produced its input.  Per case two lists -- the volumes at A, and moved by one body's size -- then, ms per
call as the best of --reps blocks of --inner calls after a warm-up, by device events around the block: the list call (count + exactly sized list) of
the second list, nh_overlap_bodies on it, nh_overlap_events by collider on the two lists, and nh_overlap_events by body on their nh_overlap_bodies
outputs; each also as a ratio to the list call.  Then one more call of each with nh_enable_timing for the per-label breakdown.

    (1) 1 M sphere queries of one box's size around random bodies (nh_overlap)
    (2) 4,096 cubes of one tile's size around random bodies (nh_region; case (d) of profiles/region_rates.log)
    (3) one region that is the world's AABB (nh_region; case (a) there)

    python tools/events_rates.py [--steps 70] [--reps 5] [--inner 10] [--out profiles/events_rates.log]
    (on a GPU box; prints the table, one JSON line at the end, and writes both to --out)
"""
import json

import numpy as np

import rates
from rates import box_planes
from nudge_amd import engine as E           # noqa: E402

NONE = rates.NONE


def main():
    ap = rates.parser("events_rates")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--cubes", type=int, default=4096)
    a = ap.parse_args()
    import torch
    import hostevents_util as HE
    import hostregion_util as R
    land = rates.landed(a)
    w, rec = land.world, land.records
    up, log = rates.upload, rates.Log()
    C = len(rec)
    lo, hi = rates.reach_bounds(rec)
    dyn = rec["p"][rec["body"] != 0].astype(np.float64)
    body_size = 2.0 * float(np.median(rec["h"][rec["body"] != 0]))
    tile_size = rates.tile_size(land.scene, w.get_bodies()["transforms"]["position"])
    rng = np.random.default_rng(1)
    shift = np.array([body_size, 0.0, 0.0])

    spheres = rates.overlap_queries(dyn[rng.integers(0, len(dyn), size=a.queries)] + rng.normal(scale=0.5 * body_size, size=(a.queries, 3)), 0.0, E.NH_SHAPE_SPHERE)
    spheres["size"][:, 0] = rng.uniform(0.5, 1.0, size=a.queries) * body_size
    moved = spheres.copy()
    moved["center"] = spheres["center"] + shift.astype(np.float32)
    centres = dyn[rng.integers(0, len(dyn), size=a.cubes)]          # tools/region_rates.py's cubes (d) and world region (a)
    half = 0.5 * tile_size
    cases = [
        (f"(1) nh_overlap, {a.queries:,} spheres of a box's size", w.overlap_records, spheres, moved),
        (f"(2) nh_region, {a.cubes:,} cubes of a tile's size", w.region_records, R.regions(box_planes(centres - half, centres + half)),
         R.regions(box_planes(centres - half + shift, centres + half + shift))),
        ("(3) nh_region, the world's AABB", w.region_records, R.regions(box_planes(lo, hi)), R.regions(box_planes(lo + shift, hi + shift))),
    ]

    def listed(records, q):
        qt = up(w, q)
        ot, _ = records(qt)
        total = rates.total_of(ot)
        ht = torch.empty((max(total, 1), 16), dtype=torch.uint8, device=w.dev)
        records(qt, offsets=ot, hits=ht, capacity=total)
        return qt, (ot, ht, total)

    def output(n, cap):
        return torch.empty(n + 1, dtype=torch.int32, device=w.dev), torch.empty((max(cap, 1), 16), dtype=torch.uint8, device=w.dev), cap

    log.say(f"landed {land.name} world: {C:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; GPU {rates.gpu_name(w)}")
    log.say(f"ms per call: the best of {a.reps} blocks of {a.inner} calls after a warm-up, device events around the block; one box, one run.  "
            f"body size {body_size:.2f} (the shift between the two lists), tile size {tile_size:.1f}")
    log.say(f"  {'case':58s} {'volumes':>9s} {'records':>11s} {'ms':>9s} {'median':>9s} {'/ list call':>12s}")
    out = {}
    for name, records, qa, qb in cases:
        n = len(qa)
        _, prev = listed(records, qa)
        qt, cur = listed(records, qb)
        ot, ht, total = cur
        inner = max(1, a.inner // 4) if total > (1 << 24) else a.inner
        bp, bc = output(n, prev[2]), output(n, total)
        w.overlap_bodies_records(n, prev, *bp)
        w.overlap_bodies_records(n, cur, *bc)
        entered, left = output(n, total), output(n, prev[2])
        rows = [
            ("the list call (count + exactly sized list)", lambda: (records(qt, offsets=ot), records(qt, offsets=ot, hits=ht, capacity=total))),
            ("nh_overlap_bodies", lambda: w.overlap_bodies_records(n, cur, *bc)),
            ("nh_overlap_events, by collider", lambda: w.overlap_events_records(n, prev, cur, entered=entered, left=left)),
            ("nh_overlap_events, by body", lambda: w.overlap_events_records(n, bp, bc, entered=entered, left=left, by_body=True)),
        ]
        res = {}
        base = None
        log.say(f"  {name:58s} {n:9,d} {total:11,d}")
        for label, fn in rows:
            best, median = rates.best_median(rates.blocks(w, fn, a.reps, inner))
            labels = rates.labels(w, fn)
            base = best if base is None else base
            res[label] = dict(ms=best, median_ms=median, ratio=best / base, labels=labels)
            log.say(f"      {label:54s} {'':9s} {'':11s} {best:9.3f} {median:9.3f} {best / base:12.3f}")
            log.say(f"          labels, ms: {labels}")
        torch.cuda.current_stream(w.dev).synchronize()
        counts = {k: rates.total_of(v[0]) for k, v in (("bodies", bc), ("entered_by_body", entered), ("left_by_body", left))}
        w.overlap_events_records(n, prev, cur, entered=entered, left=left)
        counts.update(entered=rates.total_of(entered[0]), left=rates.total_of(left[0]), prev_records=prev[2])
        log.say(f"      records: prev {prev[2]:,}, cur {total:,}; bodies of cur {counts['bodies']:,}; entered {counts['entered']:,}, left {counts['left']:,}; "
                f"by body entered {counts['entered_by_body']:,}, left {counts['left_by_body']:,}")
        if total <= (1 << 21):          # against the host oracle, byte for byte
            lp = (prev[0].cpu().numpy().view(np.uint32), rates.download(prev[1], E.OVERLAP_HIT)[:prev[2]], prev[2])
            lc = (ot.cpu().numpy().view(np.uint32), rates.download(ht, E.OVERLAP_HIT)[:total], total)
            (eo, eh), (lo_, lh) = HE.events(lp, lc)
            ok = (entered[0].cpu().numpy().view(np.uint32).tobytes() == eo.tobytes() and left[0].cpu().numpy().view(np.uint32).tobytes() == lo_.tobytes()
                  and entered[1].cpu().numpy().tobytes()[:16 * len(eh)] == eh.tobytes() and left[1].cpu().numpy().tobytes()[:16 * len(lh)] == lh.tobytes())
            assert ok, "the GPU's events differ from the host oracle's"
            log.say("      events by collider equal the host oracle byte for byte")
        out[name] = dict(volumes=n, records=total, counts=counts, **res)
        del prev, cur, bp, bc, entered, left, ot, ht
        torch.cuda.empty_cache()
    log.say()
    log.say(json.dumps(dict(colliders=C, steps=a.steps, **out)))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
