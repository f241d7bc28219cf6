"""All-hits cast rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, nh_raycast_all / nh_spherecast_all /
nh_boxcast_all / nh_capsulecast_all):
each workload timed with device events -- the count-only call, the count + list pair, and BESIDE them in the same process the closest-hit call
(nh_raycast / nh_spherecast / nh_boxcast / nh_capsulecast) on the same records and nh_overlap in list mode with the 1 M sphere queries of tools/overlap_rates.py (interleaved
repeats; the median and the spread of --repeats blocks of --reps calls) -- and broken down per kernel with the library's own event timing
(nh_kernel_times).  Workloads: tools/query_rates.py's 1,048,576 incoherent rays and its coherent downward grid, and the same as sphere casts of
radius 0.75, as box casts of half extent 0.75 (identity and random rotations) and as capsule casts of radius 0.5 and half height 0.5 (upright and
random rotations) -- the workloads of tools/boxcast_rates.py and tools/capsulecast_rates.py.  The ratios the documents quote: the all-hits count walk over the closest-hit cast (what the missing best-hit pruning costs), and
the list call over nh_overlap's list call per record written.

    python tools/castall_rates.py [--steps 70] [--reps 10] [--repeats 5] [--out profiles/castall_rates.log]
    (on a GPU box; prints the table, one JSON line at the end, and writes both to --out)
"""
import json

import numpy as np

import rates
from nudge_amd import engine as E           # noqa: E402

NONE = rates.NONE


def main():
    ap = rates.parser("castall_rates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--only", default="", help="time only the workloads whose name contains this")
    a = ap.parse_args()
    import torch
    land = rates.landed(a)
    w, C, n = land.world, land.colliders, a.rays
    log = rates.Log()
    rng = np.random.default_rng(1)
    incoherent, coherent = rates.ray_sets(rng, n, land.lo, land.hi)          # tools/query_rates.py's

    def shaped(rays, dtype, turned):
        size = dict(size=0.75) if dtype == E.BOX_CAST else dict(radius=0.5, half_height=0.5)
        return rates.cast_records(rays, dtype, rotation=rates.random_rotations(len(rays)) if turned else None, **size)

    sets = {"rays, incoherent": incoherent, "rays, coherent grid": coherent,
            "balls r=.75, incoherent": rates.cast_records(incoherent, E.SPHERE_CAST, radius=0.75),
            "balls r=.75, coherent grid": rates.cast_records(coherent, E.SPHERE_CAST, radius=0.75)}
    for label, dtype in (("boxes h=.75", E.BOX_CAST), ("capsules r=.5 hh=.5", E.CAPSULE_CAST)):
        for turn, turned in (("identity", False), ("random rot", True)):
            sets[f"{label} {turn}, incoherent"] = shaped(incoherent, dtype, turned)
            sets[f"{label} {turn}, coherent grid"] = shaped(coherent, dtype, turned)
    if a.only:
        sets = {k: v for k, v in sets.items() if a.only in k}
    calls = {E.RAY: (w.raycast_all_records, w.raycast_records), E.SPHERE_CAST: (w.spherecast_all_records, w.spherecast_records),
             E.BOX_CAST: (w.boxcast_all_records, w.boxcast_records), E.CAPSULE_CAST: (w.capsulecast_all_records, w.capsulecast_records)}

    # nh_overlap's usual 1 M sphere queries (tools/overlap_rates.py's first set), list mode
    qt = rates.upload(w, rates.spheres_on_bodies(rng, n, land.positions))
    qo = torch.empty(n + 1, dtype=torch.int32, device=w.dev)
    w.overlap_records(qt, offsets=qo)
    qtotal = rates.total_of(qo)
    qh = torch.empty((max(qtotal, 1), 16), dtype=torch.uint8, device=w.dev)
    overlap = lambda: w.overlap_records(qt, offsets=qo, hits=qh, capacity=qtotal)              # noqa: E731
    overlap(); overlap()

    rows = {}
    for name, recs in sets.items():
        all_records, closest_records = calls[recs.dtype]
        ct = rates.upload(w, recs)
        ot = torch.empty(n + 1, dtype=torch.int32, device=w.dev)
        bt = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
        all_records(ct, offsets=ot)
        off = ot.to(torch.int64) & NONE
        total = int(off[-1].item())
        if total == NONE:
            log.say(f"{name}: the total overflows 2^32 - 1; not timed")
            continue
        longest = int((off[1:] - off[:-1]).max().item())
        ht = torch.empty((max(total, 1), 32), dtype=torch.uint8, device=w.dev)
        count = lambda: all_records(ct, offsets=ot)                                              # noqa: E731
        lst = lambda: all_records(ct, offsets=ot, hits=ht, capacity=total)                       # noqa: E731
        best = lambda: closest_records(ct, hits=bt)                                              # noqa: E731
        for fn in (count, lst, best, overlap):                                                   # warm-up in this order: the scratch grows here, not in a timed call
            fn(); fn()
        t = rates.spreads(rates.interleaved(w, dict(best=best, count=count, list=lst, overlap=overlap), a.reps, a.repeats, warm=0))
        kl = {k: v[0] / a.reps for k, v in rates.kernel_times(w, lst, a.reps).items()}
        kb = {k: v[0] / a.reps for k, v in rates.kernel_times(w, best, a.reps).items()}
        walk = [v for k, v in kl.items() if k.endswith("_all_count")][0]
        closest_kernel = [v for k, v in kb.items() if k in ("q_raycast", "q_spherecast", "q_boxcast", "q_capsulecast")][0]
        c, ls, b, o = t["count"], t["list"], t["best"], t["overlap"]
        rows[name] = dict(casts=n, records=total, per_cast=total / n, longest=longest, closest=b, count_only=c, list_call=ls, count_plus_list_ms=c["ms"] + ls["ms"],
                          overlap_list=o, overlap_records=qtotal,
                          count_walk_over_closest_kernel=walk / closest_kernel, count_only_over_closest_call=c["ms"] / b["ms"],
                          list_per_record_over_overlap_per_record=(ls["ms"] / max(total, 1)) / (o["ms"] / max(qtotal, 1)),
                          kernels_list_call=kl, kernels_closest=kb)

    fmt = rates.fmt
    log.say(f"landed {land.name} world: {C:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; GPU {rates.gpu_name(w)}")
    log.say(f"median of {a.repeats} blocks of {a.reps} calls, interleaved (min .. max of the blocks); one box, one run")
    log.say(f"nh_overlap, list mode, {n:,} sphere queries r=1: {qtotal:,} records")
    log.say(f"{'workload':<48}{'records':>11}{'/cast':>7}{'longest':>8}{'closest hit ms':>24}{'all: count only ms':>24}{'all: list call ms':>24}{'nh_overlap list ms':>24}")
    for k, v in rows.items():
        log.say(f"{k:<48}{v['records']:11d}{v['per_cast']:7.2f}{v['longest']:8d}{fmt(v['closest']):>24}{fmt(v['count_only']):>24}{fmt(v['list_call']):>24}{fmt(v['overlap_list']):>24}")
    log.say()
    log.say("(the list call runs the count walk, the scan, the list walk, the ordering and the gather: count, read the total, list = the two columns added)")
    log.say(f"{'workload':<48}{'count + list ms':>16}{'count walk / closest kernel':>29}{'count only / closest call':>27}{'list / overlap list, per record':>33}")
    for k, v in rows.items():
        log.say(f"{k:<48}{v['count_plus_list_ms']:16.3f}{v['count_walk_over_closest_kernel']:29.2f}{v['count_only_over_closest_call']:27.2f}{v['list_per_record_over_overlap_per_record']:33.2f}")
    for k, v in rows.items():
        log.say(f"\n{k}: the list call per kernel, ms per call (nh_kernel_times); closest hit: " + ", ".join(f"{kn} {t:.4f}" for kn, t in v["kernels_closest"].items()))
        for kn, t in sorted(v["kernels_list_call"].items(), key=lambda kv: -kv[1]):
            log.say(f"  {kn:<28}{t:9.4f}")
    log.say(json.dumps(dict(colliders=C, steps=a.steps, workloads=rows)))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
