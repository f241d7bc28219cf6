"""Box-cast rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "scene queries"): 1 M casts per set --
incoherent closest hit at two half extents (0.75, one body; 3.0) each with the identity and with random rotations, any hit, a coherent downward
grid -- and the same sets through nh_raycast and through nh_spherecast at radius 0.75 in the same run, so the cost of the box is a ratio measured on
one box.  Timed with device events; the per-kernel times of one cast of each set come from nh_kernel_times.

    python tools/boxcast_rates.py [--steps 70] [--reps 10]        (on a GPU box; prints the table, writes profiles/boxcast_rates.log)
"""
import json

import numpy as np

import rates
from nudge_amd import engine as E           # noqa: E402

SETS = (("incoherent", False), ("incoherent any-hit", True), ("coherent", False))


def main():
    ap = rates.parser("boxcast_rates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--casts", type=int, default=1 << 20)
    a = ap.parse_args()
    import torch
    land = rates.landed(a)
    w, C, n = land.world, land.colliders, a.casts
    incoherent, coherent = rates.ray_sets(np.random.default_rng(1), n, land.lo, land.hi)          # tools/query_rates.py's and spherecast_rates.py's
    rays_of = {"incoherent": incoherent, "incoherent any-hit": incoherent, "coherent": coherent}
    random_rot = rates.random_rotations(n)
    h = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)

    def share():
        return float((rates.download(h, E.RAY_HIT)["shape"] != rates.NONE).mean())

    base = {}
    for name, any_hit in SETS:
        t = rates.upload(w, rays_of[name])
        ray_ms = rates.block(w, lambda: w.raycast_records(t, any_hit=any_hit, hits=h), a.reps)
        ray_share = share()
        t = rates.upload(w, rates.cast_records(rays_of[name], E.SPHERE_CAST, radius=0.75))
        sph_ms = rates.block(w, lambda: w.spherecast_records(t, any_hit=any_hit, hits=h), a.reps)
        base[name] = dict(ray_ms=ray_ms, ray_hits=ray_share, sphere_ms=sph_ms, sphere_hits=share())
    rows = []
    for name, any_hit in SETS:
        for size in (0.75, 3.0):
            for rot_name, rot in (("identity", None), ("random", random_rot)):
                t = rates.upload(w, rates.cast_records(rays_of[name], E.BOX_CAST, rotation=rot, size=size))
                cast = lambda: w.boxcast_records(t, any_hit=any_hit, hits=h)          # noqa: E731
                ms = rates.block(w, cast, a.reps)
                hs = share()
                kms = rates.kernel_times(w, cast, only="q_boxcast").get("q_boxcast", (float("nan"), 0))[0]
                b = base[name]
                rows.append(dict(set=name, size=size, rotation=rot_name, ms=ms, kernel_ms=kms, per_s=n / (ms * 1e-3), hit_share=hs,
                                 ray_ms=b["ray_ms"], sphere_ms=b["sphere_ms"], vs_ray=ms / b["ray_ms"], vs_sphere=ms / b["sphere_ms"]))
    # size 0 is a ray: the same walk, for the cost of the entry point itself
    t = rates.upload(w, rates.cast_records(incoherent, E.BOX_CAST))
    s0_ms = rates.block(w, lambda: w.boxcast_records(t, hits=h), a.reps)

    log = rates.Log()
    log.say(f"landed {land.name} world: {C:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; GPU {rates.gpu_name(w)}; {n:,} casts per set")
    log.say(f"{'set':<20}{'size':>6}{'rotation':>10}{'ms':>9}{'kernel ms':>11}{'M casts/s':>11}{'hits':>8}{'ray ms':>9}{'sphere ms':>11}{'box/ray':>9}{'box/sphere':>12}")
    for row in rows:
        log.say(f"{row['set']:<20}{row['size']:6.2f}{row['rotation']:>10}{row['ms']:9.3f}{row['kernel_ms']:11.3f}{row['per_s'] / 1e6:11.1f}{100 * row['hit_share']:7.1f}%"
                f"{row['ray_ms']:9.3f}{row['sphere_ms']:11.3f}{row['vs_ray']:9.2f}{row['vs_sphere']:12.2f}")
    for name, b in base.items():
        log.say(f"{name}: rays {b['ray_ms']:.3f} ms ({100 * b['ray_hits']:.1f}% hit), sphere casts r 0.75 {b['sphere_ms']:.3f} ms ({100 * b['sphere_hits']:.1f}% hit)")
    log.say(f"incoherent, size 0 through nh_boxcast: {s0_ms:.3f} ms (nh_raycast {base['incoherent']['ray_ms']:.3f} ms)")
    log.say(json.dumps(dict(colliders=C, casts=n, base=base, boxes=rows, size0_ms=s0_ms)))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
