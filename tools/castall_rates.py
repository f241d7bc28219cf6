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
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--only", default="", help="time only the workloads whose name contains this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "castall_rates.log"))
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
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

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

    def med(v):
        return dict(ms=float(np.median(v)), min=min(v), max=max(v))

    # the ray sets of tools/query_rates.py (the same seed)
    rng = np.random.default_rng(1)
    n = a.rays
    slab_p, slab_h = scene["box_transforms"]["position"][:124].astype(np.float64), scene["box_data"]["size"][:124].astype(np.float64)
    lo, hi = (slab_p - slab_h).min(axis=0), (slab_p + slab_h).max(axis=0)
    r = np.zeros(n, dtype=E.RAY)
    r["max_t"] = np.inf
    r["ignore_body"] = NONE
    r["origin"] = rng.uniform(lo, hi + np.array([0, 60, 0]), size=(n, 3))
    d = rng.normal(size=(n, 3))
    r["direction"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    incoherent = r.copy()
    side = 1024
    gx, gz = np.meshgrid(np.linspace(lo[0], hi[0], side), np.linspace(lo[2], hi[2], n // side))
    r["origin"][:, 0] = gx.reshape(-1)
    r["origin"][:, 1] = 30.0
    r["origin"][:, 2] = gz.reshape(-1)
    r["direction"] = (0.0, -1.0, 0.0)
    coherent = r.copy()

    def casts(rays, radius):
        c = np.zeros(len(rays), dtype=E.SPHERE_CAST)
        for k in ("origin", "max_t", "direction", "ignore_body"):
            c[k] = rays[k]
        c["radius"] = radius
        return c

    def shaped(rays, dtype, turned):
        c = np.zeros(len(rays), dtype=dtype)
        for k in ("origin", "max_t", "direction", "ignore_body"):
            c[k] = rays[k]
        c["rotation"] = (0.0, 0.0, 0.0, 1.0)
        if turned:
            qr = np.random.default_rng(2).normal(size=(len(rays), 4))
            c["rotation"] = qr / np.linalg.norm(qr, axis=1, keepdims=True)
        if dtype == E.BOX_CAST:
            c["size"] = 0.75
        else:
            c["radius"], c["half_height"] = 0.5, 0.5
        return c

    sets = {"rays, incoherent": incoherent, "rays, coherent grid": coherent,
            "balls r=.75, incoherent": casts(incoherent, 0.75), "balls r=.75, coherent grid": casts(coherent, 0.75)}
    for label, dtype in (("boxes h=.75", E.BOX_CAST), ("capsules r=.5 hh=.5", E.CAPSULE_CAST)):
        for turn, turned in (("identity", False), ("random rot", True)):
            sets[f"{label} {turn}, incoherent"] = shaped(incoherent, dtype, turned)
            sets[f"{label} {turn}, coherent grid"] = shaped(coherent, dtype, turned)
    if a.only:
        sets = {k: v for k, v in sets.items() if a.only in k}
    calls = {E.RAY: (w.raycast_all_records, w.raycast_records), E.SPHERE_CAST: (w.spherecast_all_records, w.spherecast_records),
             E.BOX_CAST: (w.boxcast_all_records, w.boxcast_records), E.CAPSULE_CAST: (w.capsulecast_all_records, w.capsulecast_records)}

    # nh_overlap's usual 1 M sphere queries (tools/overlap_rates.py's first set), list mode
    pos = w.get_bodies()["transforms"]["position"][1:].astype(np.float64)
    q = np.zeros(n, dtype=E.OVERLAP_QUERY)
    q["shape"], q["rotation"], q["ignore_body"] = E.NH_SHAPE_SPHERE, (0, 0, 0, 1), NONE
    q["center"] = pos[rng.integers(0, len(pos), size=n)] + rng.normal(scale=0.25, size=(n, 3))
    q["size"][:, 0] = 1.0
    qt = torch.from_numpy(q.view(np.uint8).copy()).to(w.dev)
    qo = torch.empty(n + 1, dtype=torch.int32, device=w.dev)
    w.overlap_records(qt, offsets=qo)
    qtotal = int(qo[-1].item()) & NONE
    qh = torch.empty((max(qtotal, 1), 16), dtype=torch.uint8, device=w.dev)
    overlap = lambda: w.overlap_records(qt, offsets=qo, hits=qh, capacity=qtotal)              # noqa: E731
    overlap(); overlap()

    rows = {}
    for name, recs in sets.items():
        all_records, closest_records = calls[recs.dtype]
        ct = torch.from_numpy(recs.view(np.uint8).copy()).to(w.dev)
        ot = torch.empty(n + 1, dtype=torch.int32, device=w.dev)
        bt = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
        all_records(ct, offsets=ot)
        off = ot.to(torch.int64) & NONE
        total = int(off[-1].item())
        if total == NONE:
            say(f"{name}: the total overflows 2^32 - 1; not timed")
            continue
        longest = int((off[1:] - off[:-1]).max().item())
        ht = torch.empty((max(total, 1), 32), dtype=torch.uint8, device=w.dev)
        count = lambda: all_records(ct, offsets=ot)                                              # noqa: E731
        lst = lambda: all_records(ct, offsets=ot, hits=ht, capacity=total)                       # noqa: E731
        best = lambda: closest_records(ct, hits=bt)                                              # noqa: E731
        for fn in (count, lst, best, overlap):                                                   # warm-up: the scratch grows here, not in a timed call
            fn(); fn()
        stream.synchronize()
        tc, tl, tb, to = [], [], [], []
        for _ in range(a.repeats):
            tb.append(timed(best, a.reps))
            tc.append(timed(count, a.reps))
            tl.append(timed(lst, a.reps))
            to.append(timed(overlap, a.reps))
        kl = kernels(lst, a.reps)
        kb = kernels(best, a.reps)
        walk = [v for k, v in kl.items() if k.endswith("_all_count")][0]
        closest_kernel = [v for k, v in kb.items() if k in ("q_raycast", "q_spherecast", "q_boxcast", "q_capsulecast")][0]
        c, ls, b, o = med(tc), med(tl), med(tb), med(to)
        rows[name] = dict(casts=n, records=total, per_cast=total / n, longest=longest, closest=b, count_only=c, list_call=ls, count_plus_list_ms=c["ms"] + ls["ms"],
                          overlap_list=o, overlap_records=qtotal,
                          count_walk_over_closest_kernel=walk / closest_kernel, count_only_over_closest_call=c["ms"] / b["ms"],
                          list_per_record_over_overlap_per_record=(ls["ms"] / max(total, 1)) / (o["ms"] / max(qtotal, 1)),
                          kernels_list_call=kl, kernels_closest=kb)

    say(f"landed config-2 world: {C:,} colliders, {nb:,} bodies, after {a.steps} steps; GPU {torch.cuda.get_device_name(w.dev)}")
    say(f"median of {a.repeats} blocks of {a.reps} calls, interleaved (min .. max of the blocks); one box, one run")
    say(f"nh_overlap, list mode, {n:,} sphere queries r=1: {qtotal:,} records")
    say(f"{'workload':<48}{'records':>11}{'/cast':>7}{'longest':>8}{'closest hit ms':>24}{'all: count only ms':>24}{'all: list call ms':>24}{'nh_overlap list ms':>24}")
    fmt = lambda v: f"{v['ms']:.3f} ({v['min']:.3f} .. {v['max']:.3f})"                       # noqa: E731
    for k, v in rows.items():
        say(f"{k:<48}{v['records']:11d}{v['per_cast']:7.2f}{v['longest']:8d}{fmt(v['closest']):>24}{fmt(v['count_only']):>24}{fmt(v['list_call']):>24}{fmt(v['overlap_list']):>24}")
    say()
    say("(the list call runs the count walk, the scan, the list walk, the ordering and the gather: count, read the total, list = the two columns added)")
    say(f"{'workload':<48}{'count + list ms':>16}{'count walk / closest kernel':>29}{'count only / closest call':>27}{'list / overlap list, per record':>33}")
    for k, v in rows.items():
        say(f"{k:<48}{v['count_plus_list_ms']:16.3f}{v['count_walk_over_closest_kernel']:29.2f}{v['count_only_over_closest_call']:27.2f}{v['list_per_record_over_overlap_per_record']:33.2f}")
    for k, v in rows.items():
        say(f"\n{k}: the list call per kernel, ms per call (nh_kernel_times); closest hit: " + ", ".join(f"{kn} {t:.4f}" for kn, t in v["kernels_closest"].items()))
        for kn, t in sorted(v["kernels_list_call"].items(), key=lambda kv: -kv[1]):
            say(f"  {kn:<28}{t:9.4f}")
    say(json.dumps(dict(colliders=C, steps=a.steps, workloads=rows)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    w.close()


if __name__ == "__main__":
    main()
