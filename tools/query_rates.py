"""Scene-query rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "scene queries"): the build with each
k_q_* kernel and the sort shown apart (nh_kernel_times), and rays per second of 1 M closest-hit rays for three ray sets (incoherent, coherent
downward grid, any-hit), timed with device events; per kernel the bytes moved over its time as a share of 8 TB/s (byte model below).

    python tools/query_rates.py [--steps 70] [--reps 10]        (on a GPU box; prints the table, one JSON line at the end)
"""
import json

import numpy as np

import rates
from nudge_amd import engine as E           # noqa: E402

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
    ap = rates.parser("query_rates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rays", type=int, default=1 << 20)
    a = ap.parse_args()
    import torch
    land = rates.landed(a, build=False)
    w, C, n = land.world, land.colliders, a.rays
    # the step, for scale: the landed world's still step and a full step (option no_still on a second world would double the memory: a kernel-time
    # sum of the steps is what DESIGN quotes; here the event time of 10 nh_step sub-steps)
    step_ms = rates.block(w, lambda: w.step(1), 20)
    build_ms = rates.block(w, w.query_build, a.reps)
    kt = rates.kernel_times(w, w.query_build, a.reps)

    sets = dict(zip(("incoherent", "coherent"), rates.ray_sets(np.random.default_rng(1), n, land.lo, land.hi)))
    rows = {}
    for name, rays in sets.items():
        t = rates.upload(w, rays)
        h = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
        for any_hit in (False, True):
            if name == "coherent" and any_hit:
                continue
            ms = rates.block(w, lambda: w.raycast_records(t, any_hit=any_hit, hits=h), a.reps)
            hits = rates.download(h, E.RAY_HIT)
            key = name + (" any-hit" if any_hit else "")
            rows[key] = dict(ms=ms, rays_per_s=n / (ms * 1e-3), hit_share=float((hits["shape"] != rates.NONE).mean()))

    model = byte_model(C, n)
    log = rates.Log()
    log.say(f"landed {land.name} world: {C:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; GPU {rates.gpu_name(w)}")
    log.say(f"step (nh_step, 1 sub-step, event time): {step_ms:.3f} ms")
    log.say(f"nh_query_build (event time, mean of {a.reps}): {build_ms:.3f} ms = {build_ms / step_ms:.2f} steps")
    log.say(f"{'kernel':<16}{'ms/build':>10}{'launches':>10}{'MB':>10}{'% of 8 TB/s':>13}")
    sort_ms = 0.0
    for k, (ms, launches) in sorted(kt.items(), key=lambda kv: -kv[1][0]):
        per = ms / a.reps
        if k.startswith("radix"):
            sort_ms += per
        b = model.get(k)
        share = f"{100.0 * b / (per * 1e-3) / HBM:12.1f}" if b and per > 0 else f"{'':>12}"
        log.say(f"{k:<16}{per:10.4f}{launches // a.reps:10d}{(b or 0) / 1e6:10.1f} {share}")
    log.say(f"  sort (radix_*) {sort_ms:.4f} ms of the build")
    log.say(f"{'ray set':<22}{'ms':>9}{'M rays/s':>11}{'hits':>7}{'% of 8 TB/s (64 B/ray)':>25}")
    for k, v in rows.items():
        log.say(f"{k:<22}{v['ms']:9.3f}{v['rays_per_s'] / 1e6:11.1f}{100 * v['hit_share']:6.1f}%{100.0 * model['q_raycast'] / (v['ms'] * 1e-3) / HBM:24.2f}")
    log.say(json.dumps(dict(colliders=C, step_ms=step_ms, build_ms=build_ms, kernels={k: v[0] / a.reps for k, v in kt.items()}, sort_ms=sort_ms,
                            rays=n, casts=rows)))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
