"""Distance query rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "scene queries"): 1 M queries per shape
(sphere, box, capsule; sizes up to half a body's) and workload -- tools/closest_rates.py's three: centres near random bodies with max_distance 2,
uniform over the scene's bounds with +inf, 20 m above the pile with +inf -- through nh_distance, beside nh_closest on the centres and beside
nh_overlap's count walk of the same shapes in the same run.  Per shape and set a few queries (SPOT) are compared byte for byte with the brute force
over all colliders (tests/hostdistance_util.py).  Timed with device events.

    python tools/distance_rates.py [--steps 70] [--reps 5]        (on a GPU box; prints the table, writes profiles/distance_rates.log)
"""
import argparse
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = ("sphere", "box", "capsule")
SPOT = {"sphere": 86, "box": 8, "capsule": 32}          # queries per set against the brute force: a box query costs the host ~150 segment tests per box


def measure(steps, reps, n):
    import torch
    from nudge_amd import engine as E
    from nudge_amd import scenes as S
    import hostdistance_util as D
    import hostquery_util as Q
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP, max_contacts=6 * nb)
    w.step(steps)
    w.query_build()
    w.synchronize()
    stream = torch.cuda.current_stream(w.dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        fn()
        stream.synchronize()
        ev0.record(stream)
        for _ in range(reps):
            fn()
        ev1.record(stream)
        ev1.synchronize()
        return ev0.elapsed_time(ev1) / reps

    def upload(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).to(w.dev)

    bt = w.get_bodies()["transforms"]
    rec = Q.records(bt, scene)
    live = bt["position"].astype(np.float64)[1:]
    slab_p, slab_h = scene["box_transforms"]["position"][:124].astype(np.float64), scene["box_data"]["size"][:124].astype(np.float64)
    lo, hi = (slab_p - slab_h).min(axis=0), np.maximum((slab_p + slab_h).max(axis=0), live.max(axis=0))
    half = float(np.median(rec["h"][124:].max(axis=1)))          # half a body's size
    rng = np.random.default_rng(5)
    above = rng.uniform(lo, hi, size=(n, 3))
    above[:, 1] = live[:, 1].max() + 20.0
    sets = [("near bodies, max 2", live[rng.integers(0, len(live), size=n)] + rng.normal(scale=0.5, size=(n, 3)), 2.0),
            ("uniform in bounds, inf", rng.uniform(lo, hi, size=(n, 3)), np.inf), ("20 m above the pile, inf", above, np.inf)]
    rot = rng.normal(size=(n, 4))
    rot = (rot / np.linalg.norm(rot, axis=1, keepdims=True)).astype(np.float32)
    sizes = dict(sphere=dict(radii=rng.uniform(0.1, 1.0, n) * half), box=dict(half_extents=rng.uniform(0.1, 1.0, (n, 3)) * half, rotations=rot),
                 capsule=dict(radii=rng.uniform(0.1, 0.6, n) * half, half_heights=rng.uniform(0.1, 1.0, n) * half, rotations=rot))
    hits = torch.empty((n, 48), dtype=torch.uint8, device=w.dev)
    offsets = torch.empty(n + 1, dtype=torch.int32, device=w.dev)
    rows, checked = [], 0
    for name, centres, md in sets:
        pq = np.zeros(n, dtype=E.POINT_QUERY)
        pq["point"], pq["max_distance"], pq["ignore_body"] = centres, md, 0xFFFFFFFF
        pt = upload(pq)
        row = dict(set=name, closest_ms=timed(lambda: w.closest_records(pt, hits=hits)), shapes={})
        for shape in SHAPES:
            q = D.queries(centres, max_distance=md, **sizes[shape])
            qt = upload(q)
            ot = upload(np.ascontiguousarray(q.view(np.uint8).reshape(n, 64)[:, :48]))          # (the first 48 bytes are the nh_OverlapQuery)
            ms = timed(lambda: w.distance_records(qt, hits=hits))
            got = np.frombuffer(hits.cpu().numpy().tobytes(), dtype=E.POINT_HIT)
            count_ms = timed(lambda: w.overlap_records(ot, offsets=offsets))
            found = got["shape"] != 0xFFFFFFFF
            apart = (got["normal"] != 0).any(axis=1)
            row["shapes"][shape] = dict(ms=ms, per_s=n / (ms * 1e-3), overlap_count_ms=count_ms, found=float(found.mean()), overlapping=float((found & ~apart).mean()),
                                        touching_per_query=(int(offsets[n].item()) & 0xFFFFFFFF) / n)
            pick = np.linspace(0, n - 1, SPOT[shape]).astype(np.int64)
            assert D.distance(rec, w.nbox, q[pick]).tobytes() == got[pick].tobytes(), f"{name} / {shape}: the GPU differs from the brute force"
            checked += len(pick)
        rows.append(row)
    out = dict(library=os.path.relpath(E._LIB_PATH, ROOT), gpu=torch.cuda.get_device_name(w.dev), colliders=len(rec), bodies=nb, half_body=half, rows=rows,
               checked=checked)
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=70)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_rates.log"))
    a = ap.parse_args()
    m = measure(a.steps, a.reps, a.queries)
    n = a.queries
    out = io.StringIO()
    print(f"landed config-2 world: {m['colliders']:,} colliders, {m['bodies']:,} bodies, after {a.steps} steps; GPU {m['gpu']}; {n:,} queries per shape and set; "
          f"query sizes up to {m['half_body']:.3f} (half a body)", file=out)
    print(f"{'set':<28}{'shape':<9}{'nh_distance ms':>15}{'M q/s':>9}{'nh_closest ms':>15}{'/nh_closest':>13}{'overlap count ms':>18}{'/overlap':>10}"
          f"{'found':>8}{'overlapping':>13}{'touching/query':>16}", file=out)
    for r in m["rows"]:
        for shape in SHAPES:
            s = r["shapes"][shape]
            print(f"{r['set']:<28}{shape:<9}{s['ms']:15.3f}{s['per_s'] / 1e6:9.2f}{r['closest_ms']:15.3f}{s['ms'] / r['closest_ms']:12.1f}x{s['overlap_count_ms']:18.3f}"
                  f"{s['ms'] / s['overlap_count_ms']:9.1f}x{100 * s['found']:7.1f}%{100 * s['overlapping']:12.1f}%{s['touching_per_query']:16.2f}", file=out)
    print(f"({m['checked']} queries equal the brute force over all colliders byte for byte)", file=out)
    print(json.dumps(dict(queries=n, measured=m)), file=out)
    text = out.getvalue()
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
