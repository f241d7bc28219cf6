"""Overlap-query rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, nh_overlap): each workload timed
with device events (mean of --reps calls) and broken down per kernel with the library's own event timing (nh_kernel_times), in count-only and in
list mode.  Workloads: 1 M spheres of about one box's size centred on random bodies, 64 K oriented boxes, and a few boxes that each cover a whole
tile (thousands of records per segment: the sort's case).

    python tools/overlap_rates.py [--steps 70] [--reps 10]        (on a GPU box; prints the table, one JSON line at the end)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

NONE = 0xFFFFFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=70)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
    C = len(scene["box_tags"]) + len(scene["sphere_tags"])
    w = E.World(scene, flags=E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP, max_contacts=6 * nb)
    w.step(a.steps)
    w.synchronize()
    w.query_build()
    stream = torch.cuda.current_stream(w.dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, reps):
        fn()
        stream.synchronize()
        ev0.record(stream)
        for _ in range(reps):
            fn()
        ev1.record(stream)
        ev1.synchronize()
        return ev0.elapsed_time(ev1) / reps

    def kernels(fn, reps):
        w.enable_timing(True)
        w.kernel_times(reset=True)
        for _ in range(reps):
            fn()
        stream.synchronize()
        kt = w.kernel_times(reset=True)
        w.enable_timing(False)
        return {k: v[0] / reps for k, v in kt.items()}

    rng = np.random.default_rng(1)
    pos = w.get_bodies()["transforms"]["position"][1:].astype(np.float64)
    sets = {}
    n = 1 << 20
    q = np.zeros(n, dtype=E.OVERLAP_QUERY)
    q["shape"], q["rotation"], q["ignore_body"] = E.NH_SHAPE_SPHERE, (0, 0, 0, 1), NONE
    q["center"] = pos[rng.integers(0, len(pos), size=n)] + rng.normal(scale=0.25, size=(n, 3))
    q["size"][:, 0] = 1.0
    sets["1 M spheres r=1"] = q
    n = 1 << 16
    q = np.zeros(n, dtype=E.OVERLAP_QUERY)
    q["shape"], q["ignore_body"] = E.NH_SHAPE_BOX, NONE
    q["center"] = pos[rng.integers(0, len(pos), size=n)] + rng.normal(scale=0.25, size=(n, 3))
    r = rng.normal(size=(n, 4))
    q["rotation"] = r / np.linalg.norm(r, axis=1, keepdims=True)
    q["size"] = rng.uniform(0.5, 1.5, size=(n, 3))
    sets["64 K oriented boxes"] = q
    tiles = rng.choice(124, size=8, replace=False)
    q = np.zeros(len(tiles), dtype=E.OVERLAP_QUERY)
    q["shape"], q["rotation"], q["ignore_body"] = E.NH_SHAPE_BOX, (0, 0, 0, 1), 0        # the ground slab itself left out
    q["center"] = scene["box_transforms"]["position"][tiles] + np.array([0.0, 20.0, 0.0], np.float32)
    q["size"] = scene["box_data"]["size"][tiles] * np.array([1.0, 0.0, 1.0], np.float32) + np.array([0.0, 25.0, 0.0], np.float32)
    sets["8 whole tiles"] = q

    rows = {}
    for name, q in sets.items():
        qt = torch.from_numpy(q.view(np.uint8).copy()).to(w.dev)
        ot = torch.empty(len(q) + 1, dtype=torch.int32, device=w.dev)
        w.overlap_records(qt, offsets=ot)
        total = int(ot[-1].item()) & NONE
        ht = torch.empty((max(total, 1), 16), dtype=torch.uint8, device=w.dev)
        count_ms = timed(lambda: w.overlap_records(qt, offsets=ot), a.reps)
        list_ms = timed(lambda: w.overlap_records(qt, offsets=ot, hits=ht, capacity=total), a.reps)
        kc = kernels(lambda: w.overlap_records(qt, offsets=ot), a.reps)
        kl = kernels(lambda: w.overlap_records(qt, offsets=ot, hits=ht, capacity=total), a.reps)
        counts = np.diff(ot.cpu().numpy().view(np.uint32).astype(np.int64))
        rows[name] = dict(queries=len(q), records=total, max_segment=int(counts.max()), count_ms=count_ms, list_ms=list_ms,
                          queries_per_s_count=len(q) / (count_ms * 1e-3), queries_per_s_list=len(q) / (list_ms * 1e-3),
                          records_per_s_list=total / (list_ms * 1e-3), kernels_count=kc, kernels_list=kl)

    print(f"landed config-2 world: {C:,} colliders, {nb:,} bodies, after {a.steps} steps; GPU {torch.cuda.get_device_name(w.dev)}")
    print(f"{'workload':<22}{'queries':>9}{'records':>11}{'max seg':>9}{'count ms':>10}{'list ms':>9}{'M q/s count':>13}{'M q/s list':>12}{'M rec/s':>9}")
    for k, v in rows.items():
        print(f"{k:<22}{v['queries']:9d}{v['records']:11d}{v['max_segment']:9d}{v['count_ms']:10.3f}{v['list_ms']:9.3f}"
              f"{v['queries_per_s_count'] / 1e6:13.1f}{v['queries_per_s_list'] / 1e6:12.1f}{v['records_per_s_list'] / 1e6:9.1f}")
    for k, v in rows.items():
        print(f"\n{k}: per kernel, ms per call (nh_kernel_times)")
        print(f"  {'kernel':<18}{'count-only':>11}{'list':>9}")
        names = sorted(set(v["kernels_count"]) | set(v["kernels_list"]), key=lambda n_: -v["kernels_list"].get(n_, 0.0))
        for kn in names:
            print(f"  {kn:<18}{v['kernels_count'].get(kn, 0.0):11.4f}{v['kernels_list'].get(kn, 0.0):9.4f}")
        sort = sum(t for kn, t in v["kernels_list"].items() if kn.startswith("radix"))
        walk = v["kernels_list"].get("q_overlap_count", 0.0) + v["kernels_list"].get("q_overlap_list", 0.0)
        print(f"  the two tree walks {walk:.4f} ms, the sort (radix_*) {sort:.4f} ms of {sum(v['kernels_list'].values()):.4f} ms of kernels")
    print(json.dumps(dict(colliders=C, steps=a.steps, workloads=rows)))
    w.close()


if __name__ == "__main__":
    main()
