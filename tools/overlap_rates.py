"""Overlap-query rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, nh_overlap): each workload timed
with device events (mean of --reps calls) and broken down per kernel with the library's own event timing (nh_kernel_times), in count-only and in
list mode.  Workloads: 1 M spheres of about one box's size centred on random bodies, 64 K oriented boxes, and a few boxes that each cover a whole
tile (thousands of records per segment: the sort's case).

    python tools/overlap_rates.py [--steps 70] [--reps 10]        (on a GPU box; prints the table, one JSON line at the end)
"""
import json

import numpy as np

import rates
from nudge_amd import engine as E           # noqa: E402


def main():
    ap = rates.parser("overlap_rates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--queries", type=int, default=1 << 20, help="spheres of the first workload")
    a = ap.parse_args()
    import torch
    land = rates.landed(a)
    w, C, scene, pos = land.world, land.colliders, land.scene, land.positions

    def per_call(fn):
        return {k: v[0] / a.reps for k, v in rates.kernel_times(w, fn, a.reps).items()}

    rng = np.random.default_rng(1)
    sets = {"1 M spheres r=1": rates.spheres_on_bodies(rng, a.queries, pos)}
    n = 1 << 16
    centres = pos[rng.integers(0, len(pos), size=n)] + rng.normal(scale=0.25, size=(n, 3))
    rot = rates.unit_rows(rng.normal(size=(n, 4)))
    sets["64 K oriented boxes"] = rates.overlap_queries(centres, rng.uniform(0.5, 1.5, size=(n, 3)), E.NH_SHAPE_BOX, rotation=rot)
    tiles = rng.choice(land.slabs, size=min(8, land.slabs), replace=False)
    sets["8 whole tiles"] = rates.overlap_queries(scene["box_transforms"]["position"][tiles] + np.array([0.0, 20.0, 0.0], np.float32),
                                                  scene["box_data"]["size"][tiles] * np.array([1.0, 0.0, 1.0], np.float32) + np.array([0.0, 25.0, 0.0], np.float32),
                                                  E.NH_SHAPE_BOX, ignore_body=0)        # the ground slab itself left out

    rows = {}
    for name, q in sets.items():
        qt = rates.upload(w, q)
        ot = torch.empty(len(q) + 1, dtype=torch.int32, device=w.dev)
        w.overlap_records(qt, offsets=ot)
        total = rates.total_of(ot)
        ht = torch.empty((max(total, 1), 16), dtype=torch.uint8, device=w.dev)
        count = lambda: w.overlap_records(qt, offsets=ot)                                    # noqa: E731
        lst = lambda: w.overlap_records(qt, offsets=ot, hits=ht, capacity=total)             # noqa: E731
        count_ms = rates.block(w, count, a.reps)
        list_ms = rates.block(w, lst, a.reps)
        kc, kl = per_call(count), per_call(lst)
        counts = np.diff(ot.cpu().numpy().view(np.uint32).astype(np.int64))
        rows[name] = dict(queries=len(q), records=total, max_segment=int(counts.max()), count_ms=count_ms, list_ms=list_ms,
                          queries_per_s_count=len(q) / (count_ms * 1e-3), queries_per_s_list=len(q) / (list_ms * 1e-3),
                          records_per_s_list=total / (list_ms * 1e-3), kernels_count=kc, kernels_list=kl)

    log = rates.Log()
    log.say(f"landed {land.name} world: {C:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; GPU {rates.gpu_name(w)}")
    log.say(f"{'workload':<22}{'queries':>9}{'records':>11}{'max seg':>9}{'count ms':>10}{'list ms':>9}{'M q/s count':>13}{'M q/s list':>12}{'M rec/s':>9}")
    for k, v in rows.items():
        log.say(f"{k:<22}{v['queries']:9d}{v['records']:11d}{v['max_segment']:9d}{v['count_ms']:10.3f}{v['list_ms']:9.3f}"
                f"{v['queries_per_s_count'] / 1e6:13.1f}{v['queries_per_s_list'] / 1e6:12.1f}{v['records_per_s_list'] / 1e6:9.1f}")
    for k, v in rows.items():
        log.say(f"\n{k}: per kernel, ms per call (nh_kernel_times)")
        log.say(f"  {'kernel':<18}{'count-only':>11}{'list':>9}")
        names = sorted(set(v["kernels_count"]) | set(v["kernels_list"]), key=lambda n_: -v["kernels_list"].get(n_, 0.0))
        for kn in names:
            log.say(f"  {kn:<18}{v['kernels_count'].get(kn, 0.0):11.4f}{v['kernels_list'].get(kn, 0.0):9.4f}")
        sort = sum(t for kn, t in v["kernels_list"].items() if kn.startswith("radix"))
        walk = v["kernels_list"].get("q_overlap_count", 0.0) + v["kernels_list"].get("q_overlap_list", 0.0)
        log.say(f"  the two tree walks {walk:.4f} ms, the sort (radix_*) {sort:.4f} ms of {sum(v['kernels_list'].values()):.4f} ms of kernels")
    log.say(json.dumps(dict(colliders=C, steps=a.steps, workloads=rows)))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
