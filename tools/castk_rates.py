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
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

NONE = 0xFFFFFFFF
KS = (1, 4, 8, 16, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=70)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--casts", type=int, default=1 << 20)
    ap.add_argument("--only", default="", help="time only the workloads whose name contains this")
    ap.add_argument("--no-check", action="store_true", help="skip the brute-force spot check")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "castk_rates.log"))
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

    def med(v):
        return dict(ms=float(np.median(v)), min=min(v), max=max(v))

    # the ray sets of tools/query_rates.py (the same seed)
    rng = np.random.default_rng(1)
    n = a.casts
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

    def shaped(rays, dtype):
        c = np.zeros(len(rays), dtype=dtype)
        for k in ("origin", "max_t", "direction", "ignore_body"):
            c[k] = rays[k]
        if dtype == E.SPHERE_CAST:
            c["radius"] = 0.75
            return c
        qr = np.random.default_rng(2).normal(size=(len(rays), 4))
        c["rotation"] = qr / np.linalg.norm(qr, axis=1, keepdims=True)
        if dtype == E.BOX_CAST:
            c["size"] = 0.75
        else:
            c["radius"], c["half_height"] = 0.5, 0.5
        return c

    sets = {"rays, incoherent": incoherent, "rays, coherent grid": coherent, "balls r=.75, incoherent": shaped(incoherent, E.SPHERE_CAST),
            "boxes h=.75 random rot, incoherent": shaped(incoherent, E.BOX_CAST), "capsules r=.5 hh=.5 random rot, incoherent": shaped(incoherent, E.CAPSULE_CAST)}
    if a.only:
        sets = {k: v for k, v in sets.items() if a.only in k}
    calls = {E.RAY: (w.raycast_k_records, w.raycast_all_records, w.raycast_records), E.SPHERE_CAST: (w.spherecast_k_records, w.spherecast_all_records, w.spherecast_records),
             E.BOX_CAST: (w.boxcast_k_records, w.boxcast_all_records, w.boxcast_records), E.CAPSULE_CAST: (w.capsulecast_k_records, w.capsulecast_all_records, w.capsulecast_records)}
    rec = None
    if not a.no_check:
        import hostcastk_util as HK
        import hostquery_util as Q
        rec = Q.records(w.get_bodies()["transforms"], scene)

    rows = {}
    for name, recs in sets.items():
        k_records, all_records, closest_records = calls[recs.dtype]
        ct = torch.from_numpy(recs.view(np.uint8).copy()).to(w.dev)
        ot = torch.empty(n + 1, dtype=torch.int32, device=w.dev)
        bt = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
        nt = torch.empty(n, dtype=torch.int32, device=w.dev)
        kt = torch.empty((n * max(KS), 32), dtype=torch.uint8, device=w.dev)
        all_records(ct, offsets=ot)
        off = ot.to(torch.int64) & NONE
        total = int(off[-1].item())
        if total == NONE:
            say(f"{name}: the total overflows 2^32 - 1; not timed")
            continue
        size = off[1:] - off[:-1]
        ht = torch.empty((max(total, 1), 32), dtype=torch.uint8, device=w.dev)
        fns = dict(closest=lambda: closest_records(ct, hits=bt), count=lambda: all_records(ct, offsets=ot),
                   list=lambda: all_records(ct, offsets=ot, hits=ht, capacity=total))
        for k in KS:
            fns[k] = (lambda k: lambda: k_records(ct, k, counts=nt, hits=kt))(k)
        for fn in fns.values():                                                                  # warm-up: the scratch grows here, not in a timed call
            fn(); fn()
        stream.synchronize()
        times = {key: [] for key in fns}
        for _ in range(a.repeats):
            for key, fn in fns.items():
                times[key].append(timed(fn, a.reps))
        t = {key: med(v) for key, v in times.items()}
        print(f"timed: {name}", file=sys.stderr, flush=True)
        checked = 0
        if rec is not None:
            pick = np.sort(np.random.default_rng(3).choice(n, size=258, replace=False))
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

    say(f"landed config-2 world: {C:,} colliders, {nb:,} bodies, after {a.steps} steps; GPU {torch.cuda.get_device_name(w.dev)}")
    say(f"{n:,} casts per workload; median of {a.repeats} blocks of {a.reps} calls, interleaved (min .. max of the blocks); one box, one run")
    fmt = lambda v: f"{v['ms']:.3f} ({v['min']:.3f} .. {v['max']:.3f})"                       # noqa: E731
    for name, v in rows.items():
        say()
        say(f"{name}: {v['records']:,} records in all ({v['per_cast']:.2f} per cast, the longest {v['longest']}); {v['checked_against_brute_force']} rows equal the brute force byte for byte")
        say(f"  closest hit {fmt(v['closest'])} ms; all hits: count only {fmt(v['count_only'])} ms, list call {fmt(v['list_call'])} ms, count + list {v['count_plus_list_ms']:.3f} ms")
        say(f"  {'k':>4}{'first k ms':>28}{'/ closest hit':>15}{'/ (count + list)':>18}{'casts with more than k':>24}")
        for k in KS:
            say(f"  {k:>4}{fmt(v['k_calls'][k]):>28}{v['k_over_closest'][k]:15.2f}{v['k_over_count_plus_list'][k]:18.3f}{v['share_more_than'][k]:24.3f}")
    say()
    say(json.dumps(dict(colliders=C, steps=a.steps, workloads=rows)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    w.close()


if __name__ == "__main__":
    main()
