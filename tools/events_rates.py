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


def box_planes(lo, hi):
    """The six planes of the axis-aligned boxes [lo, hi] ((n, 3) each), as (n, 6, 4)."""
    lo, hi = np.atleast_2d(lo), np.atleast_2d(hi)
    out = np.zeros((len(lo), 6, 4), dtype=np.float32)
    for k in range(3):
        out[:, 2 * k, k], out[:, 2 * k, 3] = 1.0, -lo[:, k]
        out[:, 2 * k + 1, k], out[:, 2 * k + 1, 3] = -1.0, hi[:, k]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=70)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--cubes", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_rates.log"))
    a = ap.parse_args()
    import torch
    import hostevents_util as HE
    import hostregion_util as R
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
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

    def up(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).to(w.dev)

    rec = R.records(w.get_bodies()["transforms"], scene)
    C = len(rec)
    reach = np.linalg.norm(rec["h"].astype(np.float64), axis=1, keepdims=True)
    lo, hi = (rec["p"] - reach).min(axis=0) - 1.0, (rec["p"] + reach).max(axis=0) + 1.0
    dyn = rec["p"][rec["body"] != 0].astype(np.float64)
    body_size = 2.0 * float(np.median(rec["h"][rec["body"] != 0]))
    tile = np.nonzero(np.asarray(scene["tile_of_body"]) == 0)[0]
    tp = w.get_bodies()["transforms"]["position"][tile].astype(np.float64)
    tile_size = float((tp.max(axis=0) - tp.min(axis=0))[[0, 2]].max())
    rng = np.random.default_rng(1)
    shift = np.array([body_size, 0.0, 0.0])

    spheres = np.zeros(a.queries, dtype=E.OVERLAP_QUERY)
    spheres["shape"], spheres["rotation"], spheres["ignore_body"] = E.NH_SHAPE_SPHERE, (0, 0, 0, 1), NONE
    spheres["center"] = dyn[rng.integers(0, len(dyn), size=a.queries)] + rng.normal(scale=0.5 * body_size, size=(a.queries, 3))
    spheres["size"][:, 0] = rng.uniform(0.5, 1.0, size=a.queries) * body_size
    moved = spheres.copy()
    moved["center"] = spheres["center"] + shift.astype(np.float32)
    centres = dyn[rng.integers(0, len(dyn), size=a.cubes)]
    half = 0.5 * tile_size
    cases = [
        (f"(1) nh_overlap, {a.queries:,} spheres of a box's size", w.overlap_records, spheres, moved),
        (f"(2) nh_region, {a.cubes:,} cubes of a tile's size", w.region_records, R.regions(box_planes(centres - half, centres + half)),
         R.regions(box_planes(centres - half + shift, centres + half + shift))),
        ("(3) nh_region, the world's AABB", w.region_records, R.regions(box_planes(lo, hi)), R.regions(box_planes(lo + shift, hi + shift))),
    ]

    def listed(records, q):
        qt = up(q)
        ot, _ = records(qt)
        total = int(ot[-1].item()) & NONE
        ht = torch.empty((max(total, 1), 16), dtype=torch.uint8, device=w.dev)
        records(qt, offsets=ot, hits=ht, capacity=total)
        return qt, (ot, ht, total)

    def output(n, cap):
        return torch.empty(n + 1, dtype=torch.int32, device=w.dev), torch.empty((max(cap, 1), 16), dtype=torch.uint8, device=w.dev), cap

    def timed(fn, inner):
        fn()
        stream.synchronize()
        ts = []
        for _ in range(a.reps):
            ev0.record(stream)
            for _ in range(inner):
                fn()
            ev1.record(stream)
            ev1.synchronize()
            ts.append(ev0.elapsed_time(ev1) / inner)
        w.enable_timing(True)
        w.kernel_times()
        fn()
        labels = {k: round(v[0], 4) for k, v in sorted(w.kernel_times().items()) if v[1]}
        w.enable_timing(False)
        return min(ts), float(np.median(ts)), labels

    say(f"landed config-2 world: {C:,} colliders, {nb:,} bodies, after {a.steps} steps; GPU {torch.cuda.get_device_name(w.dev)}")
    say(f"ms per call: the best of {a.reps} blocks of {a.inner} calls after a warm-up, device events around the block; one box, one run.  "
        f"body size {body_size:.2f} (the shift between the two lists), tile size {tile_size:.1f}")
    say(f"  {'case':58s} {'volumes':>9s} {'records':>11s} {'ms':>9s} {'median':>9s} {'/ list call':>12s}")
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
        say(f"  {name:58s} {n:9,d} {total:11,d}")
        for label, fn in rows:
            best, median, labels = timed(fn, inner)
            base = best if base is None else base
            res[label] = dict(ms=best, median_ms=median, ratio=best / base, labels=labels)
            say(f"      {label:54s} {'':9s} {'':11s} {best:9.3f} {median:9.3f} {best / base:12.3f}")
            say(f"          labels, ms: {labels}")
        stream.synchronize()
        counts = {k: int(v[0][-1].item()) & NONE for k, v in (("bodies", bc), ("entered_by_body", entered), ("left_by_body", left))}
        w.overlap_events_records(n, prev, cur, entered=entered, left=left)
        counts.update(entered=int(entered[0][-1].item()) & NONE, left=int(left[0][-1].item()) & NONE, prev_records=prev[2])
        say(f"      records: prev {prev[2]:,}, cur {total:,}; bodies of cur {counts['bodies']:,}; entered {counts['entered']:,}, left {counts['left']:,}; "
            f"by body entered {counts['entered_by_body']:,}, left {counts['left_by_body']:,}")
        if total <= (1 << 21):          # against the host oracle, byte for byte
            lp = (prev[0].cpu().numpy().view(np.uint32), np.frombuffer(prev[1].cpu().numpy().tobytes(), dtype=E.OVERLAP_HIT)[:prev[2]], prev[2])
            lc = (ot.cpu().numpy().view(np.uint32), np.frombuffer(ht.cpu().numpy().tobytes(), dtype=E.OVERLAP_HIT)[:total], total)
            (eo, eh), (lo_, lh) = HE.events(lp, lc)
            ok = (entered[0].cpu().numpy().view(np.uint32).tobytes() == eo.tobytes() and left[0].cpu().numpy().view(np.uint32).tobytes() == lo_.tobytes()
                  and entered[1].cpu().numpy().tobytes()[:16 * len(eh)] == eh.tobytes() and left[1].cpu().numpy().tobytes()[:16 * len(lh)] == lh.tobytes())
            assert ok, "the GPU's events differ from the host oracle's"
            say("      events by collider equal the host oracle byte for byte")
        out[name] = dict(volumes=n, records=total, counts=counts, **res)
        del prev, cur, bp, bc, entered, left, ot, ht
        torch.cuda.empty_cache()
    say()
    say(json.dumps(dict(colliders=C, steps=a.steps, **out)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    w.close()


if __name__ == "__main__":
    main()
