"""Scene-query rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "scene queries"): the build with each
k_q_* kernel and the sort shown apart (nh_kernel_times), and rays per second of 1 M closest-hit rays for three ray sets (incoherent, coherent
downward grid, any-hit), timed with device events; per kernel the bytes moved over its time as a share of 8 TB/s (byte model below).

    python tools/query_rates.py [--steps 70] [--reps 10]        (on a GPU box; prints the table, one JSON line at the end)
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

HBM = 8.0e12

# bytes each kernel moves at C colliders (n rays), read + write, counting every record once (caches not modelled)
#   q_xform: collider transform 32 + body transform 32 + shape 16 + tag 4 in; record 48 out
#   q_keys: record position 16 in; key 8 + index 4 out
#   radix_*: 6 passes of (key 8 + value 4) read twice (histogram, scatter) and written once
#   q_tree: ~2 log2(C) key reads of 8 B per internal node (binary searches hit cache lines shared by neighbours: counted as 4 keys) + 5 words out
#   q_links: last 4 + table 4 in, the link 4 out per internal node
#   q_boxes_runs: per leaf index 4 + what q_xform reads 84 + parent word 4 + escape 4 in, record 48 + leaf node 32 out; per internal node parent word 4 in, box 24 out
#   (q_boxes_top: a few thousand nodes, latency bound: no share printed; tools/refit_rates.py)
#   q_raycast: ray 32 + hit 32 per ray (node and record reads come from the caches: the share printed is of the compulsory traffic only)
def byte_model(C, n_rays):
    return {
        "q_xform": C * (32 + 32 + 16 + 4 + 48),
        "q_keys": C * (16 + 8 + 4),
        "radix_hist": 6 * C * 8, "radix_scan": 6 * 256 * 512 * 4 * 2, "radix_scatter": 6 * C * (8 + 4) * 2,
        "q_tree": (C - 1) * (4 * 8 + 28),
        "q_links": (C - 1) * 12,
        "q_boxes_runs": C * (4 + 84 + 4 + 4 + 48 + 32) + (C - 1) * (4 + 24),
        "q_raycast": n_rays * 64,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=70)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rays", type=int, default=1 << 20)
    a = ap.parse_args()
    import torch
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
    C = len(scene["box_tags"]) + len(scene["sphere_tags"])
    w = E.World(scene, flags=E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP, max_contacts=6 * nb)
    w.step(a.steps)
    w.synchronize()
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

    # the step, for scale: the landed world's still step and a full step (option no_still on a second world would double the memory: a kernel-time
    # sum of the steps is what DESIGN quotes; here the event time of 10 nh_step sub-steps)
    step_ms = timed(lambda: w.step(1), 20)
    build_ms = timed(w.query_build, a.reps)
    w.enable_timing(True)
    w.kernel_times(reset=True)
    for _ in range(a.reps):
        w.query_build()
    w.synchronize()
    kt = w.kernel_times(reset=True)
    w.enable_timing(False)

    rng = np.random.default_rng(1)
    n = a.rays
    slab_p, slab_h = scene["box_transforms"]["position"][:124].astype(np.float64), scene["box_data"]["size"][:124].astype(np.float64)
    lo, hi = (slab_p - slab_h).min(axis=0), (slab_p + slab_h).max(axis=0)
    sets = {}
    r = np.zeros(n, dtype=E.RAY)
    r["max_t"] = np.inf; r["ignore_body"] = 0xFFFFFFFF
    r["origin"] = rng.uniform(lo, hi + np.array([0, 60, 0]), size=(n, 3))
    d = rng.normal(size=(n, 3)); r["direction"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    sets["incoherent"] = r.copy()
    side = 1024
    gx, gz = np.meshgrid(np.linspace(lo[0], hi[0], side), np.linspace(lo[2], hi[2], n // side))
    r["origin"][:, 0] = gx.reshape(-1); r["origin"][:, 1] = 30.0; r["origin"][:, 2] = gz.reshape(-1)
    r["direction"] = (0.0, -1.0, 0.0)
    sets["coherent"] = r.copy()
    rows = {}
    for name, rays in sets.items():
        t = torch.from_numpy(rays.view(np.uint8).copy()).to(w.dev)
        h = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
        for any_hit in (False, True):
            if name == "coherent" and any_hit:
                continue
            ms = timed(lambda: w.raycast_records(t, any_hit=any_hit, hits=h), a.reps)
            hits = np.frombuffer(h.cpu().numpy().tobytes(), dtype=E.RAY_HIT)
            key = name + (" any-hit" if any_hit else "")
            rows[key] = dict(ms=ms, rays_per_s=n / (ms * 1e-3), hit_share=float((hits["shape"] != 0xFFFFFFFF).mean()))

    model = byte_model(C, n)
    print(f"landed config-2 world: {C:,} colliders, {nb:,} bodies, after {a.steps} steps; GPU {torch.cuda.get_device_name(w.dev)}")
    print(f"step (nh_step, 1 sub-step, event time): {step_ms:.3f} ms")
    print(f"nh_query_build (event time, mean of {a.reps}): {build_ms:.3f} ms = {build_ms / step_ms:.2f} steps")
    print(f"{'kernel':<16}{'ms/build':>10}{'launches':>10}{'MB':>10}{'% of 8 TB/s':>13}")
    sort_ms = 0.0
    for k, (ms, launches) in sorted(kt.items(), key=lambda kv: -kv[1][0]):
        per = ms / a.reps
        if k.startswith("radix"):
            sort_ms += per
        b = model.get(k)
        share = f"{100.0 * b / (per * 1e-3) / HBM:12.1f}" if b and per > 0 else f"{'':>12}"
        print(f"{k:<16}{per:10.4f}{launches // a.reps:10d}{(b or 0) / 1e6:10.1f} {share}")
    print(f"  sort (radix_*) {sort_ms:.4f} ms of the build")
    print(f"{'ray set':<22}{'ms':>9}{'M rays/s':>11}{'hits':>7}{'% of 8 TB/s (64 B/ray)':>25}")
    for k, v in rows.items():
        print(f"{k:<22}{v['ms']:9.3f}{v['rays_per_s'] / 1e6:11.1f}{100 * v['hit_share']:6.1f}%{100.0 * model['q_raycast'] / (v['ms'] * 1e-3) / HBM:24.2f}")
    print(json.dumps(dict(colliders=C, step_ms=step_ms, build_ms=build_ms, kernels={k: v[0] / a.reps for k, v in kt.items()}, sort_ms=sort_ms,
                          rays=n, casts=rows)))
    w.close()


if __name__ == "__main__":
    main()
