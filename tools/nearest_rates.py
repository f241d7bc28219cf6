"""k-nearest query rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "scene queries"): 1 M queries per
workload -- tools/closest_rates.py's three: points near random bodies with max_distance 2, uniform points over the scene's bounds with +inf, points
20 m above the pile with +inf -- through nh_closest_k at k = 1, 4, 8, 16, 32 with the seed (the library) and without it (a build of the same sources
with -DNH_Q_CLOSEST_K_NO_SEED by tools/build_variant.sh, run in a child process of its own), beside nh_closest on the same records in the same run, and
beside the detour the call replaces: nh_overlap counting and then listing a sphere query around the same points whose radius returns about k colliders
(the median k-th distance of the near-bodies set).  258 queries per k, 86 from each of the three sets, are compared byte for byte with the brute force over
all colliders (tests/hostnearest_util.py).  Timed with device events.

    tools/build_variant.sh noseedk -DNH_Q_CLOSEST_K_NO_SEED       (here: hipcc cross-compiles)
    python tools/nearest_rates.py [--steps 70] [--reps 10]        (on a GPU box; prints the table, writes profiles/nearest_rates.log)
"""
import json
import os
import subprocess
import sys

import numpy as np

import rates

NOSEED = os.path.join(rates.ROOT, "nudge_amd", "_ab", "libnoseedk.so")
KS = (1, 4, 8, 16, 32)


def measure(a, full):
    """The figures of the library this process loaded (engine reads NUDGE_HIP_LIBRARY): one dict.  `full`: nh_closest, the overlap detour and the
    brute-force spot check as well (the seeded run); otherwise nh_closest_k's times and digests alone."""
    import torch
    from nudge_amd import engine as E
    land = rates.landed(a)
    w, n, reps = land.world, a.queries, a.reps
    lo, hi = land.pile_bounds()
    sets = [(name, rates.point_queries(points, md)) for name, points, md in rates.point_sets(np.random.default_rng(5), n, land.positions, lo, hi)]
    near = sets[0][1]
    h1 = torch.empty((n, 48), dtype=torch.uint8, device=w.dev)
    hk = torch.empty((n * max(KS), 48), dtype=torch.uint8, device=w.dev)
    ck = torch.empty(n, dtype=torch.int32, device=w.dev)
    pick = np.linspace(0, n - 1, 86).astype(np.int64)
    rows, kth, checks = [], {}, {}
    for name, arr in sets:
        t = rates.upload(w, arr)
        row = dict(set=name, k={})
        if full:
            row["closest_ms"] = rates.block(w, lambda: w.closest_records(t, hits=h1), reps)
            single = h1.cpu().numpy().tobytes()
        for k in KS:
            ms = rates.block(w, lambda: w.closest_k_records(t, k, counts=ck, hits=hk), reps)
            counts = ck.cpu().numpy().view(np.uint32)
            hits = rates.download(hk[: n * k], E.POINT_HIT).reshape(n, k)
            row["k"][k] = dict(ms=ms, per_s=n / (ms * 1e-3), full=float((counts == k).mean()), mean=float(counts.mean()),
                               digest=int(np.frombuffer(hits.tobytes(), dtype=np.uint64).sum(dtype=np.uint64)) ^ int(counts.sum(dtype=np.uint64)))
            if full:
                if k == 1:
                    assert hits.tobytes() == single, f"{name}: k = 1 is not nh_closest"
                if arr is near:
                    kth[k] = float(np.median(hits[counts == k, k - 1]["distance"])) if (counts == k).any() else 2.0
                checks.setdefault(k, []).append((arr[pick], counts[pick].copy(), hits[pick].copy()))
        rows.append(row)
    out = dict(library=os.path.relpath(E._LIB_PATH, rates.ROOT), gpu=rates.gpu_name(w), colliders=land.colliders, bodies=land.bodies, rows=rows)
    if full:
        # the detour: count the colliders touching a ball of the k-th distance around each near-bodies point, read the total, list them
        detour = {}
        ot = torch.empty(n + 1, dtype=torch.int32, device=w.dev)
        for k in KS:
            sp = rates.overlap_queries(near["point"], (max(kth[k], 0.0), 0.0, 0.0), E.NH_SHAPE_SPHERE, rotation=0.0)
            st = rates.upload(w, sp)
            count_ms = rates.block(w, lambda: w.overlap_records(st, offsets=ot), reps)
            total = rates.total_of(ot)
            d = dict(radius=sp["size"][0, 0].item(), count_ms=count_ms, per_query=total / n)
            if 0 < total <= (1 << 26):
                ht = torch.empty((total, 16), dtype=torch.uint8, device=w.dev)
                # (warm = 2: the first grows the sort scratch once, outside the timing)
                d["list_ms"] = rates.block(w, lambda: w.overlap_records(st, offsets=ot, hits=ht, capacity=total), reps, warm=2)
                del ht
            detour[k] = d
        out["detour"] = detour
        # the spot check: 3 x 86 queries per k against the brute force over every collider
        import hostnearest_util as N
        rec = land.records
        checked = 0
        for k, parts in checks.items():
            for qs, counts, hits in parts:
                rc, rh = N.closest_k(rec, w.nbox, qs, k)
                assert np.array_equal(rc, counts) and rh.tobytes() == hits.tobytes(), f"k {k}: the GPU differs from the brute force"
                checked += len(qs)
        out["checked"] = checked
    w.close()
    return out


def main():
    ap = rates.parser("nearest_rates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--child", action="store_true", help="measure the library this process loads and print one JSON line")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a, False)))
        return
    if not os.path.exists(NOSEED):
        sys.exit(f"{NOSEED} is missing: tools/build_variant.sh noseedk -DNH_Q_CLOSEST_K_NO_SEED")
    seeded = measure(a, True)
    env = dict(os.environ, NUDGE_HIP_LIBRARY=NOSEED)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--queries", str(a.queries)] + rates.world_flags(a),
                           env=env, capture_output=True, text=True, timeout=600)
    if child.returncode != 0:
        sys.exit(f"the unseeded run failed ({child.returncode}):\n{child.stderr[-2000:]}")
    plain = json.loads(child.stdout.strip().split("\n")[-1])
    n = a.queries
    log = rates.Log()
    log.say(f"landed {rates.world_name(a.tiles, a.world_side)} world: {seeded['colliders']:,} colliders, {seeded['bodies']:,} bodies, after {a.steps} steps; GPU {seeded['gpu']}; "
            f"{n:,} queries per set")
    for s, u in zip(seeded["rows"], plain["rows"]):
        log.say(f"{s['set']}: nh_closest {s['closest_ms']:.3f} ms ({n / s['closest_ms'] / 1e3:.1f} M q/s)")
        log.say(f"{'  k':<6}{'seeded ms':>11}{'M q/s':>9}{'/nh_closest':>13}{'unseeded ms':>13}{'seed gain':>11}{'full lists':>12}{'mean held':>11}")
        for k in KS:
            sk, uk = s["k"][k], u["k"][str(k)]              # (the child's keys came through JSON)
            assert sk["digest"] == uk["digest"], f"{s['set']}, k {k}: the seed changed the answer"
            log.say(f"{k:>3}   {sk['ms']:11.3f}{sk['per_s'] / 1e6:9.1f}{sk['ms'] / s['closest_ms']:12.2f}x{uk['ms']:13.3f}{uk['ms'] / sk['ms']:10.2f}x"
                    f"{100 * sk['full']:11.1f}%{sk['mean']:11.2f}")
    log.say("the detour (near-bodies points): nh_overlap with a ball of the median k-th distance, count call + list call, beside nh_closest_k on that set")
    log.say(f"{'  k':<6}{'radius':>9}{'listed/query':>14}{'count ms':>10}{'list ms':>10}{'both ms':>10}{'nh_closest_k ms':>17}{'detour/call':>13}")
    for k in KS:
        d = seeded["detour"][k]
        sk = seeded["rows"][0]["k"][k]
        if "list_ms" in d:
            both = d["count_ms"] + d["list_ms"]
            log.say(f"{k:>3}   {d['radius']:9.3f}{d['per_query']:14.2f}{d['count_ms']:10.3f}{d['list_ms']:10.3f}{both:10.3f}{sk['ms']:17.3f}{both / sk['ms']:12.2f}x")
        else:
            log.say(f"{k:>3}   {d['radius']:9.3f}{d['per_query']:14.2f}{d['count_ms']:10.3f}{'-':>10}{'-':>10}{sk['ms']:17.3f}{'-':>13}")
    log.say("(the detour still owes the distances and the order: its records are unordered collider identities)")
    log.say(f"(k = 1 equals nh_closest's bytes in every set; the seeded and unseeded records are identical: equal digests; {seeded['checked']} queries equal the "
            f"brute force over all colliders byte for byte)")
    log.say(json.dumps(dict(queries=n, seeded=seeded, unseeded=plain)))
    log.write(a.out)


if __name__ == "__main__":
    main()
