"""Closest-point query rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "scene queries"): 1 M queries
per workload -- points near random bodies with max_distance 2, uniform points over the scene's bounds with +inf, points 20 m above the pile with
+inf -- through nh_closest with the seed (the library) and without it (a build of the same sources with -DNH_Q_CLOSEST_NO_SEED by
tools/build_variant.sh, run in a child process of its own), beside the sphere-overlap count walk (1 M spheres of radius 1, count only) measured in
the same run.  Timed with device events; the kernel's own time of one call comes from nh_kernel_times.

    tools/build_variant.sh noseed -DNH_Q_CLOSEST_NO_SEED          (here: hipcc cross-compiles)
    python tools/closest_rates.py [--steps 70] [--reps 10]        (on a GPU box; prints the table, writes profiles/closest_rates.log)
"""
import json
import os
import subprocess
import sys

import numpy as np

import rates

NOSEED = os.path.join(rates.ROOT, "nudge_amd", "_ab", "libnoseed.so")


def measure(a):
    """The figures of the library this process loaded (engine reads NUDGE_HIP_LIBRARY): one dict."""
    import torch
    from nudge_amd import engine as E
    land = rates.landed(a)
    w, n, reps = land.world, a.queries, a.reps
    lo, hi = land.pile_bounds()
    sets = rates.point_sets(np.random.default_rng(5), n, land.positions, lo, hi)
    h = torch.empty((n, 48), dtype=torch.uint8, device=w.dev)
    rows = []
    for name, points, md in sets:
        t = rates.upload(w, rates.point_queries(points, md))
        call = lambda: w.closest_records(t, hits=h)          # noqa: E731
        ms = rates.block(w, call, reps)
        kms = rates.kernel_times(w, call).get("q_closest", (float("nan"), 0))[0]
        hits = rates.download(h, E.POINT_HIT)
        found = hits["shape"] != rates.NONE
        rows.append(dict(set=name, ms=ms, kernel_ms=kms, per_s=n / (ms * 1e-3), found=float(found.mean()),
                         inside=float((hits["distance"][found] < 0).mean()) if found.any() else 0.0,
                         digest=int(np.frombuffer(hits.tobytes(), dtype=np.uint64).sum(dtype=np.uint64))))
    # the sphere-overlap count walk on the same box, in the same run: the uniform set's points
    st = rates.upload(w, rates.overlap_queries(sets[1][1], (1.0, 0.0, 0.0), E.NH_SHAPE_SPHERE, rotation=0.0))
    ot = torch.empty(n + 1, dtype=torch.int32, device=w.dev)
    overlap_ms = rates.block(w, lambda: w.overlap_records(st, offsets=ot), reps)
    out = dict(library=os.path.relpath(E._LIB_PATH, rates.ROOT), gpu=rates.gpu_name(w), colliders=land.colliders, bodies=land.bodies, rows=rows,
               overlap_count_ms=overlap_ms)
    w.close()
    return out


def main():
    ap = rates.parser("closest_rates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--child", action="store_true", help="measure the library this process loads and print one JSON line")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a)))
        return
    seeded = measure(a)
    if not os.path.exists(NOSEED):
        sys.exit(f"{NOSEED} is missing: tools/build_variant.sh noseed -DNH_Q_CLOSEST_NO_SEED")
    env = dict(os.environ, NUDGE_HIP_LIBRARY=NOSEED)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--queries", str(a.queries)] + rates.world_flags(a),
                           env=env, capture_output=True, text=True, timeout=600)
    if child.returncode != 0:
        sys.exit(f"the unseeded run failed ({child.returncode}):\n{child.stderr[-2000:]}")
    plain = json.loads(child.stdout.strip().split("\n")[-1])
    n = a.queries
    log = rates.Log()
    log.say(f"landed {rates.world_name(a.tiles, a.world_side)} world: {seeded['colliders']:,} colliders, {seeded['bodies']:,} bodies, after {a.steps} steps; GPU {seeded['gpu']}; {n:,} queries per set")
    log.say(f"{'set':<28}{'seeded ms':>11}{'kernel ms':>11}{'M q/s':>9}{'unseeded ms':>13}{'kernel ms':>11}{'M q/s':>9}{'seed gain':>11}{'found':>8}{'inside':>8}"
            f"{'/overlap':>10}")
    for s, u in zip(seeded["rows"], plain["rows"]):
        assert s["digest"] == u["digest"], f"{s['set']}: the seed changed the answer"
        log.say(f"{s['set']:<28}{s['ms']:11.3f}{s['kernel_ms']:11.3f}{s['per_s'] / 1e6:9.1f}{u['ms']:13.3f}{u['kernel_ms']:11.3f}{u['per_s'] / 1e6:9.1f}"
                f"{u['ms'] / s['ms']:10.2f}x{100 * s['found']:7.1f}%{100 * s['inside']:7.1f}%{s['ms'] / seeded['overlap_count_ms']:10.2f}")
    log.say(f"sphere overlap r 1.0, count only, same centres as the uniform set: {seeded['overlap_count_ms']:.3f} ms (unseeded library's run: "
            f"{plain['overlap_count_ms']:.3f} ms)")
    log.say("(the seeded and unseeded hit records are identical in every set: equal digests)")
    log.say(json.dumps(dict(queries=n, seeded=seeded, unseeded=plain)))
    log.write(a.out)


if __name__ == "__main__":
    main()
