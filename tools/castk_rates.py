"""First-k cast rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, nh_raycast_k / nh_spherecast_k /
nh_boxcast_k / nh_capsulecast_k): 1,048,576 incoherent casts of each shape at k = 1, 4, 8, 16, 32, and BESIDE them in the same process, on the same
records, the closest-hit call and the all-hits call (count only; count + list = the count-only call and the list call added, which is what a caller
runs who counts, reads the total and lists) -- device events, interleaved, the median [min .. max] of --repeats blocks of --reps calls after two
warm-ups.  Rays also as tools/query_rates.py's coherent downward grid.  258 casts per (shape, k) are compared byte for byte with the brute force over
all colliders (tests/hostcastk_util.py).  The two ratios the documents quote: the k call over the closest-hit call (what the list costs, k = 1
especially) and the k call over count + list (what the limit saves).

    python tools/castk_rates.py [--steps 70] [--reps 10] [--repeats 5] [--out profiles/castk_rates.log]
    (on a GPU box; prints the table, one JSON line at the end, and writes both to --out)
"""
import json
import sys

import numpy as np

import rates
from nudge_amd import engine as E           # noqa: E402

NONE = rates.NONE
KS = (1, 4, 8, 16, 32)


def main():
    ap = rates.parser("castk_rates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--casts", type=int, default=1 << 20)
    ap.add_argument("--only", default="", help="time only the workloads whose name contains this")
    ap.add_argument("--no-check", action="store_true", help="skip the brute-force spot check")
    a = ap.parse_args()
    import torch
    land = rates.landed(a)
    w, C, n = land.world, land.colliders, a.casts
    log = rates.Log()
    incoherent, coherent = rates.ray_sets(np.random.default_rng(1), n, land.lo, land.hi)          # tools/query_rates.py's
    rot = rates.random_rotations(n)
    sets = {"rays, incoherent": incoherent, "rays, coherent grid": coherent, "balls r=.75, incoherent": rates.cast_records(incoherent, E.SPHERE_CAST, radius=0.75),
            "boxes h=.75 random rot, incoherent": rates.cast_records(incoherent, E.BOX_CAST, rotation=rot, size=0.75),
            "capsules r=.5 hh=.5 random rot, incoherent": rates.cast_records(incoherent, E.CAPSULE_CAST, rotation=rot, radius=0.5, half_height=0.5)}
    if a.only:
        sets = {k: v for k, v in sets.items() if a.only in k}
    calls = {E.RAY: (w.raycast_k_records, w.raycast_all_records, w.raycast_records), E.SPHERE_CAST: (w.spherecast_k_records, w.spherecast_all_records, w.spherecast_records),
             E.BOX_CAST: (w.boxcast_k_records, w.boxcast_all_records, w.boxcast_records), E.CAPSULE_CAST: (w.capsulecast_k_records, w.capsulecast_all_records, w.capsulecast_records)}
    rec = None
    if not a.no_check:
        import hostcastk_util as HK
        rec = land.records

    rows = {}
    for name, recs in sets.items():
        k_records, all_records, closest_records = calls[recs.dtype]
        ct = rates.upload(w, recs)
        ot = torch.empty(n + 1, dtype=torch.int32, device=w.dev)
        bt = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
        nt = torch.empty(n, dtype=torch.int32, device=w.dev)
        kt = torch.empty((n * max(KS), 32), dtype=torch.uint8, device=w.dev)
        all_records(ct, offsets=ot)
        off = ot.to(torch.int64) & NONE
        total = int(off[-1].item())
        if total == NONE:
            log.say(f"{name}: the total overflows 2^32 - 1; not timed")
            continue
        size = off[1:] - off[:-1]
        ht = torch.empty((max(total, 1), 32), dtype=torch.uint8, device=w.dev)
        fns = dict(closest=lambda: closest_records(ct, hits=bt), count=lambda: all_records(ct, offsets=ot),
                   list=lambda: all_records(ct, offsets=ot, hits=ht, capacity=total))
        for k in KS:
            fns[k] = (lambda k: lambda: k_records(ct, k, counts=nt, hits=kt))(k)
        t = rates.spreads(rates.interleaved(w, fns, a.reps, a.repeats))
        print(f"timed: {name}", file=sys.stderr, flush=True)
        checked = 0
        if rec is not None:
            pick = rates.spot(n)
            seg = HK.segments(rec, w.nbox, recs[pick])
            pt = torch.from_numpy(pick).to(w.dev)
            for k in KS:
                k_records(ct, k, counts=nt, hits=kt)
                got_n = nt[pt].cpu().numpy().view(np.uint32)
                got_h = kt[:n * k].reshape(n, k * 32)[pt].cpu().numpy().tobytes()
                ref_n, ref_h = HK.cast_k(rec, w.nbox, recs[pick], k, seg)
                assert np.array_equal(got_n, ref_n) and got_h == ref_h.tobytes(), f"{name}, k {k}: the GPU differs from the brute force"
                checked += len(pick)
        both = t["count"]["ms"] + t["list"]["ms"]
        rows[name] = dict(casts=n, records=total, per_cast=total / n, longest=int(size.max().item()), share_more_than={k: float((size > k).float().mean().item()) for k in KS},
                          closest=t["closest"], count_only=t["count"], list_call=t["list"], count_plus_list_ms=both, k_calls={k: t[k] for k in KS},
                          k_over_closest={k: t[k]["ms"] / t["closest"]["ms"] for k in KS}, k_over_count_plus_list={k: t[k]["ms"] / both for k in KS},
                          checked_against_brute_force=checked)

    fmt = rates.fmt
    log.say(f"landed {land.name} world: {C:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; GPU {rates.gpu_name(w)}")
    log.say(f"{n:,} casts per workload; median of {a.repeats} blocks of {a.reps} calls, interleaved (min .. max of the blocks); one box, one run")
    for name, v in rows.items():
        log.say()
        log.say(f"{name}: {v['records']:,} records in all ({v['per_cast']:.2f} per cast, the longest {v['longest']}); {v['checked_against_brute_force']} rows equal the brute force byte for byte")
        log.say(f"  closest hit {fmt(v['closest'])} ms; all hits: count only {fmt(v['count_only'])} ms, list call {fmt(v['list_call'])} ms, count + list {v['count_plus_list_ms']:.3f} ms")
        log.say(f"  {'k':>4}{'first k ms':>28}{'/ closest hit':>15}{'/ (count + list)':>18}{'casts with more than k':>24}")
        for k in KS:
            log.say(f"  {k:>4}{fmt(v['k_calls'][k]):>28}{v['k_over_closest'][k]:15.2f}{v['k_over_count_plus_list'][k]:18.3f}{v['share_more_than'][k]:24.3f}")
    log.say()
    log.say(json.dumps(dict(colliders=C, steps=a.steps, workloads=rows)))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
