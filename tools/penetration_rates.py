"""Penetration-query rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, nh_penetration): each workload
timed with device events, nh_penetration and nh_overlap in list mode beside each other in the same process (interleaved repeats; the median and the
spread of --repeats blocks of --reps calls), and broken down per kernel with the library's own event timing (nh_kernel_times).  Workloads: the
1 M spheres of tools/overlap_rates.py (about one box's size, centred on random bodies), 1 M oriented boxes and 1 M capsules of comparable size.

    python tools/penetration_rates.py [--steps 70] [--reps 10] [--repeats 5]        (on a GPU box; prints the table, one JSON line at the end)
"""
import json

import numpy as np

import rates
from nudge_amd import engine as E           # noqa: E402


def main():
    ap = rates.parser("penetration_rates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--queries", type=int, default=1 << 20, help="queries per workload")
    a = ap.parse_args()
    import torch
    land = rates.landed(a)
    w, C, pos, n = land.world, land.colliders, land.positions, a.queries

    def centres():
        return pos[rng.integers(0, len(pos), size=n)] + rng.normal(scale=0.25, size=(n, 3))

    rng = np.random.default_rng(1)
    sets = {"1 M spheres r=1": rates.spheres_on_bodies(rng, n, pos)}                            # (tools/overlap_rates.py's first set, the same seed)
    rot = rates.unit_rows(rng.normal(size=(n, 4)))
    sets["1 M oriented boxes"] = rates.overlap_queries(centres(), rng.uniform(0.5, 1.0, size=(n, 3)), E.NH_SHAPE_BOX, rotation=rot)
    sets["1 M capsules r=.5 hh=.5"] = rates.overlap_queries(centres(), (0.5, 0.5, 0.0), E.NH_SHAPE_CAPSULE, rotation=rot)

    rows = {}
    for name, q in sets.items():
        qt = rates.upload(w, q)
        ot = torch.empty(len(q) + 1, dtype=torch.int32, device=w.dev)
        w.overlap_records(qt, offsets=ot)
        total = rates.total_of(ot)
        ht = torch.empty((max(total, 1), 16), dtype=torch.uint8, device=w.dev)
        pt = torch.empty((max(total, 1), 32), dtype=torch.uint8, device=w.dev)
        pen = lambda: w.penetration_records(qt, offsets=ot, hits=pt, capacity=total)              # noqa: E731
        t = rates.interleaved(w, dict(overlap=lambda: w.overlap_records(qt, offsets=ot, hits=ht, capacity=total), pen=pen), a.reps, a.repeats)
        to, tp = t["overlap"], t["pen"]
        kp = {k: v[0] / a.reps for k, v in rates.kernel_times(w, pen, a.reps).items()}
        depth = pt.view(torch.float32).reshape(-1, 8)[:total, 3]
        rows[name] = dict(queries=len(q), records=total, overlap_list_ms=float(np.median(to)), overlap_list_ms_min=min(to), overlap_list_ms_max=max(to),
                          penetration_ms=float(np.median(tp)), penetration_ms_min=min(tp), penetration_ms_max=max(tp),
                          ratio=float(np.median(tp) / np.median(to)), mean_depth=float(depth.mean().item()) if total else 0.0, kernels_penetration=kp)

    log = rates.Log()
    log.say(f"landed {land.name} world: {C:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; GPU {rates.gpu_name(w)}")
    log.say(f"median of {a.repeats} blocks of {a.reps} calls, interleaved (min .. max of the blocks)")
    log.say(f"{'workload':<26}{'queries':>9}{'records':>10}{'nh_overlap list ms':>30}{'nh_penetration ms':>30}{'ratio':>7}")
    for k, v in rows.items():
        o = f"{v['overlap_list_ms']:.3f} ({v['overlap_list_ms_min']:.3f} .. {v['overlap_list_ms_max']:.3f})"
        p = f"{v['penetration_ms']:.3f} ({v['penetration_ms_min']:.3f} .. {v['penetration_ms_max']:.3f})"
        log.say(f"{k:<26}{v['queries']:9d}{v['records']:10d}{o:>30}{p:>30}{v['ratio']:7.2f}")
    for k, v in rows.items():
        log.say(f"\n{k}: nh_penetration per kernel, ms per call (nh_kernel_times)")
        for kn, t in sorted(v["kernels_penetration"].items(), key=lambda kv: -kv[1]):
            log.say(f"  {kn:<26}{t:9.4f}")
    log.say(json.dumps(dict(colliders=C, steps=a.steps, workloads=rows)))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
