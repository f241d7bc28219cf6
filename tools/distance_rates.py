"""Distance query rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "scene queries"): 1 M queries per shape
(sphere, box, capsule; sizes up to half a body's) and workload -- tools/closest_rates.py's three: centres near random bodies with max_distance 2,
uniform over the scene's bounds with +inf, 20 m above the pile with +inf -- through nh_distance, beside nh_closest on the centres and beside
nh_overlap's count walk of the same shapes in the same run.  Per shape and set a few queries (SPOT) are compared byte for byte with the brute force
over all colliders (tests/hostdistance_util.py).  Timed with device events.

    python tools/distance_rates.py [--steps 70] [--reps 5]        (on a GPU box; prints the table, writes profiles/distance_rates.log)
"""
import json
import os

import numpy as np

import rates

SHAPES = ("sphere", "box", "capsule")
SPOT = {"sphere": 86, "box": 8, "capsule": 32}          # queries per set against the brute force: a box query costs the host ~150 segment tests per box


def measure(a):
    import torch
    from nudge_amd import engine as E
    import hostdistance_util as D
    land = rates.landed(a)
    w, rec, live, n, reps = land.world, land.records, land.positions, a.queries, a.reps
    lo, hi = land.pile_bounds()
    half = float(np.median(rec["h"][land.slabs:].max(axis=1)))          # half a body's size
    rng = np.random.default_rng(5)
    sets = rates.point_sets(rng, n, live, lo, hi, above_first=True)
    rot = rates.unit_rows(rng.normal(size=(n, 4))).astype(np.float32)
    sizes = dict(sphere=dict(radii=rng.uniform(0.1, 1.0, n) * half), box=dict(half_extents=rng.uniform(0.1, 1.0, (n, 3)) * half, rotations=rot),
                 capsule=dict(radii=rng.uniform(0.1, 0.6, n) * half, half_heights=rng.uniform(0.1, 1.0, n) * half, rotations=rot))
    hits = torch.empty((n, 48), dtype=torch.uint8, device=w.dev)
    offsets = torch.empty(n + 1, dtype=torch.int32, device=w.dev)
    rows, checked = [], 0
    for name, centres, md in sets:
        pt = rates.upload(w, rates.point_queries(centres, md))
        row = dict(set=name, closest_ms=rates.block(w, lambda: w.closest_records(pt, hits=hits), reps), shapes={})
        for shape in SHAPES:
            q = D.queries(centres, max_distance=md, **sizes[shape])
            qt = rates.upload(w, q)
            ot = rates.upload(w, np.ascontiguousarray(q.view(np.uint8).reshape(n, 64)[:, :48]))          # (the first 48 bytes are the nh_OverlapQuery)
            ms = rates.block(w, lambda: w.distance_records(qt, hits=hits), reps)
            got = rates.download(hits, E.POINT_HIT)
            count_ms = rates.block(w, lambda: w.overlap_records(ot, offsets=offsets), reps)
            found = got["shape"] != rates.NONE
            apart = (got["normal"] != 0).any(axis=1)
            row["shapes"][shape] = dict(ms=ms, per_s=n / (ms * 1e-3), overlap_count_ms=count_ms, found=float(found.mean()), overlapping=float((found & ~apart).mean()),
                                        touching_per_query=rates.total_of(offsets) / n)
            pick = np.linspace(0, n - 1, SPOT[shape]).astype(np.int64)
            assert D.distance(rec, w.nbox, q[pick]).tobytes() == got[pick].tobytes(), f"{name} / {shape}: the GPU differs from the brute force"
            checked += len(pick)
        rows.append(row)
    out = dict(library=os.path.relpath(E._LIB_PATH, rates.ROOT), gpu=rates.gpu_name(w), colliders=len(rec), bodies=land.bodies, half_body=half, rows=rows,
               checked=checked)
    w.close()
    return out


def main():
    ap = rates.parser("distance_rates")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", type=int, default=1 << 20)
    a = ap.parse_args()
    m = measure(a)
    n = a.queries
    log = rates.Log()
    log.say(f"landed {rates.world_name(a.tiles, a.world_side)} world: {m['colliders']:,} colliders, {m['bodies']:,} bodies, after {a.steps} steps; GPU {m['gpu']}; {n:,} queries per shape and set; "
            f"query sizes up to {m['half_body']:.3f} (half a body)")
    log.say(f"{'set':<28}{'shape':<9}{'nh_distance ms':>15}{'M q/s':>9}{'nh_closest ms':>15}{'/nh_closest':>13}{'overlap count ms':>18}{'/overlap':>10}"
            f"{'found':>8}{'overlapping':>13}{'touching/query':>16}")
    for r in m["rows"]:
        for shape in SHAPES:
            s = r["shapes"][shape]
            log.say(f"{r['set']:<28}{shape:<9}{s['ms']:15.3f}{s['per_s'] / 1e6:9.2f}{r['closest_ms']:15.3f}{s['ms'] / r['closest_ms']:12.1f}x{s['overlap_count_ms']:18.3f}"
                    f"{s['ms'] / s['overlap_count_ms']:9.1f}x{100 * s['found']:7.1f}%{100 * s['overlapping']:12.1f}%{s['touching_per_query']:16.2f}")
    log.say(f"({m['checked']} queries equal the brute force over all colliders byte for byte)")
    log.say(json.dumps(dict(queries=n, measured=m)))
    log.write(a.out)


if __name__ == "__main__":
    main()
