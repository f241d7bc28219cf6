"""Sphere-cast rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "scene queries"): 1 M casts per set --
incoherent closest hit at two radii (about half a body's size and about two bodies' size), any hit, a coherent downward grid -- and the same ray sets
through nh_raycast in the same run, so the cost of the radius is a ratio measured on one box.  Timed with device events.

    python tools/spherecast_rates.py [--steps 70] [--reps 10]        (on a GPU box; prints the table, one JSON line at the end)
"""
import json

import numpy as np

import rates
from nudge_amd import engine as E           # noqa: E402

SETS = (("incoherent", False), ("incoherent any-hit", True), ("coherent", False))


def main():
    ap = rates.parser("spherecast_rates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--casts", type=int, default=1 << 20)
    a = ap.parse_args()
    import torch
    land = rates.landed(a)
    w, C, n = land.world, land.colliders, a.casts
    body_half = float(np.median(land.scene["box_data"]["size"][land.slabs:]))
    incoherent, coherent = rates.ray_sets(np.random.default_rng(1), n, land.lo, land.hi)          # tools/query_rates.py's
    rays_of = {"incoherent": incoherent, "incoherent any-hit": incoherent, "coherent": coherent}
    small, large = 0.5 * 2 * body_half, 2.0 * 2 * body_half          # about half a body's size, about two bodies' size
    h = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)

    def share():
        return float((rates.download(h, E.RAY_HIT)["shape"] != rates.NONE).mean())

    ray_rows = {}
    for name, any_hit in SETS:
        t = rates.upload(w, rays_of[name])
        ms = rates.block(w, lambda: w.raycast_records(t, any_hit=any_hit, hits=h), a.reps)
        ray_rows[name] = dict(ms=ms, per_s=n / (ms * 1e-3), hit_share=share())
    rows = []
    for name, any_hit in SETS:
        for radius in (small, large):
            t = rates.upload(w, rates.cast_records(rays_of[name], E.SPHERE_CAST, radius=radius))
            ms = rates.block(w, lambda: w.spherecast_records(t, any_hit=any_hit, hits=h), a.reps)
            rows.append(dict(set=name, radius=radius, ms=ms, per_s=n / (ms * 1e-3), hit_share=share(), ray_ms=ray_rows[name]["ms"], cost=ms / ray_rows[name]["ms"]))
    # radius 0 is a ray: the same walk, for the cost of the entry point itself
    t = rates.upload(w, rates.cast_records(incoherent, E.SPHERE_CAST))
    r0_ms = rates.block(w, lambda: w.spherecast_records(t, hits=h), a.reps)

    log = rates.Log()
    log.say(f"landed {land.name} world: {C:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; GPU {rates.gpu_name(w)}; "
            f"median body half extent {body_half:.3f}")
    log.say(f"{'set':<20}{'radius':>8}{'ms':>9}{'M casts/s':>11}{'hits':>8}{'ray ms':>9}{'M rays/s':>10}{'ray hits':>10}{'cast / ray':>12}")
    for row in rows:
        rr = ray_rows[row["set"]]
        log.say(f"{row['set']:<20}{row['radius']:8.3f}{row['ms']:9.3f}{row['per_s'] / 1e6:11.1f}{100 * row['hit_share']:7.1f}%{rr['ms']:9.3f}"
                f"{rr['per_s'] / 1e6:10.1f}{100 * rr['hit_share']:9.1f}%{row['cost']:12.2f}")
    log.say(f"incoherent, radius 0 through nh_spherecast: {r0_ms:.3f} ms (nh_raycast {ray_rows['incoherent']['ms']:.3f} ms)")
    log.say(json.dumps(dict(colliders=C, casts=n, body_half=body_half, rays=ray_rows, sweeps=rows, radius0_ms=r0_ms)))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
