"""Penetration-query rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, nh_penetration): each workload
timed with device events, nh_penetration and nh_overlap in list mode beside each other in the same process (interleaved repeats; the median and the
spread of --repeats blocks of --reps calls), and broken down per kernel with the library's own event timing (nh_kernel_times).  Workloads: the
1 M spheres of tools/overlap_rates.py (about one box's size, centred on random bodies), 1 M oriented boxes and 1 M capsules of comparable size.

    python tools/penetration_rates.py [--steps 70] [--reps 10] [--repeats 5]        (on a GPU box; prints the table, one JSON line at the end)
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
    ap.add_argument("--repeats", type=int, default=5)
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
    n = 1 << 20
    sets = {}
    q = np.zeros(n, dtype=E.OVERLAP_QUERY)
    q["shape"], q["rotation"], q["ignore_body"] = E.NH_SHAPE_SPHERE, (0, 0, 0, 1), NONE
    q["center"] = pos[rng.integers(0, len(pos), size=n)] + rng.normal(scale=0.25, size=(n, 3))
    q["size"][:, 0] = 1.0
    sets["1 M spheres r=1"] = q                                        # (tools/overlap_rates.py's first set, the same seed)
    r = rng.normal(size=(n, 4))
    rot = r / np.linalg.norm(r, axis=1, keepdims=True)
    q = np.zeros(n, dtype=E.OVERLAP_QUERY)
    q["shape"], q["rotation"], q["ignore_body"] = E.NH_SHAPE_BOX, rot, NONE
    q["center"] = pos[rng.integers(0, len(pos), size=n)] + rng.normal(scale=0.25, size=(n, 3))
    q["size"] = rng.uniform(0.5, 1.0, size=(n, 3))
    sets["1 M oriented boxes"] = q
    q = np.zeros(n, dtype=E.OVERLAP_QUERY)
    q["shape"], q["rotation"], q["ignore_body"] = E.NH_SHAPE_CAPSULE, rot, NONE
    q["center"] = pos[rng.integers(0, len(pos), size=n)] + rng.normal(scale=0.25, size=(n, 3))
    q["size"][:, 0], q["size"][:, 1] = 0.5, 0.5
    sets["1 M capsules r=.5 hh=.5"] = q

    rows = {}
    for name, q in sets.items():
        qt = torch.from_numpy(q.view(np.uint8).copy()).to(w.dev)
        ot = torch.empty(len(q) + 1, dtype=torch.int32, device=w.dev)
        w.overlap_records(qt, offsets=ot)
        total = int(ot[-1].item()) & NONE
        ht = torch.empty((max(total, 1), 16), dtype=torch.uint8, device=w.dev)
        pt = torch.empty((max(total, 1), 32), dtype=torch.uint8, device=w.dev)
        overlap = lambda: w.overlap_records(qt, offsets=ot, hits=ht, capacity=total)              # noqa: E731
        pen = lambda: w.penetration_records(qt, offsets=ot, hits=pt, capacity=total)              # noqa: E731
        for fn in (overlap, pen):                                                                    # warm-up: the scratch grows here, not in a timed call
            fn(); fn()
        stream.synchronize()
        to, tp = [], []
        for _ in range(a.repeats):
            to.append(timed(overlap, a.reps))
            tp.append(timed(pen, a.reps))
        kp = kernels(pen, a.reps)
        depth = pt.view(torch.float32).reshape(-1, 8)[:total, 3]
        rows[name] = dict(queries=len(q), records=total, overlap_list_ms=float(np.median(to)), overlap_list_ms_min=min(to), overlap_list_ms_max=max(to),
                          penetration_ms=float(np.median(tp)), penetration_ms_min=min(tp), penetration_ms_max=max(tp),
                          ratio=float(np.median(tp) / np.median(to)), mean_depth=float(depth.mean().item()) if total else 0.0, kernels_penetration=kp)

    print(f"landed config-2 world: {C:,} colliders, {nb:,} bodies, after {a.steps} steps; GPU {torch.cuda.get_device_name(w.dev)}")
    print(f"median of {a.repeats} blocks of {a.reps} calls, interleaved (min .. max of the blocks)")
    print(f"{'workload':<26}{'queries':>9}{'records':>10}{'nh_overlap list ms':>30}{'nh_penetration ms':>30}{'ratio':>7}")
    for k, v in rows.items():
        o = f"{v['overlap_list_ms']:.3f} ({v['overlap_list_ms_min']:.3f} .. {v['overlap_list_ms_max']:.3f})"
        p = f"{v['penetration_ms']:.3f} ({v['penetration_ms_min']:.3f} .. {v['penetration_ms_max']:.3f})"
        print(f"{k:<26}{v['queries']:9d}{v['records']:10d}{o:>30}{p:>30}{v['ratio']:7.2f}")
    for k, v in rows.items():
        print(f"\n{k}: nh_penetration per kernel, ms per call (nh_kernel_times)")
        for kn, t in sorted(v["kernels_penetration"].items(), key=lambda kv: -kv[1]):
            print(f"  {kn:<26}{t:9.4f}")
    print(json.dumps(dict(colliders=C, steps=a.steps, workloads=rows)))
    w.close()


if __name__ == "__main__":
    main()
