"""Closest-point query rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "scene queries"): 1 M queries
per workload -- points near random bodies with max_distance 2, uniform points over the scene's bounds with +inf, points 20 m above the pile with
+inf -- through nh_closest with the seed (the library) and without it (a build of the same sources with -DNH_Q_CLOSEST_NO_SEED by
tools/build_variant.sh, run in a child process of its own), beside the sphere-overlap count walk (1 M spheres of radius 1, count only) measured in
the same run.  Timed with device events; the kernel's own time of one call comes from nh_kernel_times.

    tools/build_variant.sh noseed -DNH_Q_CLOSEST_NO_SEED          (here: hipcc cross-compiles)
    python tools/closest_rates.py [--steps 70] [--reps 10]        (on a GPU box; prints the table, writes profiles/closest_rates.log)
"""
import argparse
import io
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NOSEED = os.path.join(ROOT, "nudge_amd", "_ab", "libnoseed.so")


def measure(steps, reps, n):
    """The figures of the library this process loaded (engine reads NUDGE_HIP_LIBRARY): one dict."""
    import torch
    from nudge_amd import engine as E
    from nudge_amd import scenes as S
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

    def kernel_ms(fn, name):
        w.enable_timing(True)
        w.kernel_times(reset=True)
        fn()
        w.synchronize()
        kt = w.kernel_times(reset=True)
        w.enable_timing(False)
        return kt.get(name, (float("nan"), 0))[0]

    def upload(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).to(w.dev)

    bt = w.get_bodies()["transforms"]["position"].astype(np.float64)
    live = bt[1:]
    slab_p, slab_h = scene["box_transforms"]["position"][:124].astype(np.float64), scene["box_data"]["size"][:124].astype(np.float64)
    lo, hi = (slab_p - slab_h).min(axis=0), np.maximum((slab_p + slab_h).max(axis=0), live.max(axis=0))
    rng = np.random.default_rng(5)
    sets = []
    q = np.zeros(n, dtype=E.POINT_QUERY)
    q["ignore_body"] = 0xFFFFFFFF
    near = q.copy()
    near["point"] = live[rng.integers(0, len(live), size=n)] + rng.normal(scale=0.5, size=(n, 3))
    near["max_distance"] = 2.0
    sets.append(("near bodies, max 2", near))
    uni = q.copy()
    uni["point"] = rng.uniform(lo, hi, size=(n, 3))
    uni["max_distance"] = np.inf
    sets.append(("uniform in bounds, inf", uni))
    above = q.copy()
    above["point"] = rng.uniform(lo, hi, size=(n, 3))
    above["point"][:, 1] = live[:, 1].max() + 20.0
    above["max_distance"] = np.inf
    sets.append(("20 m above the pile, inf", above))
    h = torch.empty((n, 48), dtype=torch.uint8, device=w.dev)
    rows = []
    for name, arr in sets:
        t = upload(arr)
        ms = timed(lambda: w.closest_records(t, hits=h))
        kms = kernel_ms(lambda: w.closest_records(t, hits=h), "q_closest")
        hits = np.frombuffer(h.cpu().numpy().tobytes(), dtype=E.POINT_HIT)
        found = hits["shape"] != 0xFFFFFFFF
        rows.append(dict(set=name, ms=ms, kernel_ms=kms, per_s=n / (ms * 1e-3), found=float(found.mean()),
                         inside=float((hits["distance"][found] < 0).mean()) if found.any() else 0.0,
                         digest=int(np.frombuffer(hits.tobytes(), dtype=np.uint64).sum(dtype=np.uint64))))
    # the sphere-overlap count walk on the same box, in the same run
    sp = np.zeros(n, dtype=E.OVERLAP_QUERY)
    sp["center"] = uni["point"]
    sp["shape"] = E.NH_SHAPE_SPHERE
    sp["size"][:, 0] = 1.0
    sp["ignore_body"] = 0xFFFFFFFF
    st = upload(sp)
    ot = torch.empty(n + 1, dtype=torch.int32, device=w.dev)
    overlap_ms = timed(lambda: w.overlap_records(st, offsets=ot))
    out = dict(library=os.path.relpath(E._LIB_PATH, ROOT), gpu=torch.cuda.get_device_name(w.dev), colliders=len(scene["box_tags"]) + len(scene["sphere_tags"]), bodies=nb,
               rows=rows, overlap_count_ms=overlap_ms)
    w.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=70)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--child", action="store_true", help="measure the library this process loads and print one JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "closest_rates.log"))
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.steps, a.reps, a.queries)))
        return
    seeded = measure(a.steps, a.reps, a.queries)
    if not os.path.exists(NOSEED):
        sys.exit(f"{NOSEED} is missing: tools/build_variant.sh noseed -DNH_Q_CLOSEST_NO_SEED")
    env = dict(os.environ, NUDGE_HIP_LIBRARY=NOSEED)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--reps", str(a.reps), "--queries", str(a.queries)],
                           env=env, capture_output=True, text=True, timeout=600)
    if child.returncode != 0:
        sys.exit(f"the unseeded run failed ({child.returncode}):\n{child.stderr[-2000:]}")
    plain = json.loads(child.stdout.strip().split("\n")[-1])
    n = a.queries
    out = io.StringIO()
    print(f"landed config-2 world: {seeded['colliders']:,} colliders, {seeded['bodies']:,} bodies, after {a.steps} steps; GPU {seeded['gpu']}; {n:,} queries per set",
          file=out)
    print(f"{'set':<28}{'seeded ms':>11}{'kernel ms':>11}{'M q/s':>9}{'unseeded ms':>13}{'kernel ms':>11}{'M q/s':>9}{'seed gain':>11}{'found':>8}{'inside':>8}"
          f"{'/overlap':>10}", file=out)
    for s, u in zip(seeded["rows"], plain["rows"]):
        assert s["digest"] == u["digest"], f"{s['set']}: the seed changed the answer"
        print(f"{s['set']:<28}{s['ms']:11.3f}{s['kernel_ms']:11.3f}{s['per_s'] / 1e6:9.1f}{u['ms']:13.3f}{u['kernel_ms']:11.3f}{u['per_s'] / 1e6:9.1f}"
              f"{u['ms'] / s['ms']:10.2f}x{100 * s['found']:7.1f}%{100 * s['inside']:7.1f}%{s['ms'] / seeded['overlap_count_ms']:10.2f}", file=out)
    print(f"sphere overlap r 1.0, count only, same centres as the uniform set: {seeded['overlap_count_ms']:.3f} ms (unseeded library's run: "
          f"{plain['overlap_count_ms']:.3f} ms)", file=out)
    print("(the seeded and unseeded hit records are identical in every set: equal digests)", file=out)
    print(json.dumps(dict(queries=n, seeded=seeded, unseeded=plain)), file=out)
    text = out.getvalue()
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
