"""Capsule-cast and capsule-overlap rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "scene queries"):
1 M casts per set -- incoherent closest hit at (r, hh) = (0.5, 0.5) and (1.0, 2.0), each with the identity (upright) and with random rotations, any
hit, a coherent downward grid -- beside the same sets through nh_raycast, nh_spherecast at radius 0.75 and nh_boxcast at half extent 0.75 in the same
run, so the cost of the capsule is a ratio measured on one box; then 1 M capsule overlap queries, count only and list.  Timed with device events;
the per-kernel times of one call come from nh_kernel_times.

    python tools/capsulecast_rates.py [--steps 70] [--reps 10]        (on a GPU box; prints the table, writes profiles/capsulecast_rates.log)
"""
import json

import numpy as np

import rates
from nudge_amd import engine as E           # noqa: E402

SETS = (("incoherent", False), ("incoherent any-hit", True), ("coherent", False))


def main():
    ap = rates.parser("capsulecast_rates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--casts", type=int, default=1 << 20)
    a = ap.parse_args()
    import torch
    land = rates.landed(a)
    w, C, n, scene, lo, hi = land.world, land.colliders, a.casts, land.scene, land.lo, land.hi
    incoherent, coherent = rates.ray_sets(np.random.default_rng(1), n, lo, hi)          # tools/query_rates.py's, spherecast_rates.py's and boxcast_rates.py's
    rays_of = {"incoherent": incoherent, "incoherent any-hit": incoherent, "coherent": coherent}
    random_rot = rates.random_rotations(n)
    h = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)

    def share():
        return float((rates.download(h, E.RAY_HIT)["shape"] != rates.NONE).mean())

    base = {}
    for name, any_hit in SETS:
        rays = rays_of[name]
        t = rates.upload(w, rays)
        ray_ms = rates.block(w, lambda: w.raycast_records(t, any_hit=any_hit, hits=h), a.reps)
        ray_share = share()
        t = rates.upload(w, rates.cast_records(rays, E.SPHERE_CAST, radius=0.75))
        sph_ms = rates.block(w, lambda: w.spherecast_records(t, any_hit=any_hit, hits=h), a.reps)
        sph_share = share()
        t = rates.upload(w, rates.cast_records(rays, E.BOX_CAST, size=0.75))
        box_ms = rates.block(w, lambda: w.boxcast_records(t, any_hit=any_hit, hits=h), a.reps)
        base[name] = dict(ray_ms=ray_ms, ray_hits=ray_share, sphere_ms=sph_ms, sphere_hits=sph_share, box_ms=box_ms, box_hits=share())
    rows = []
    for name, any_hit in SETS:
        for rad, hh in ((0.5, 0.5), (1.0, 2.0)):
            for rot_name, rot in (("identity", None), ("random", random_rot)):
                t = rates.upload(w, rates.cast_records(rays_of[name], E.CAPSULE_CAST, rotation=rot, radius=rad, half_height=hh))
                cast = lambda: w.capsulecast_records(t, any_hit=any_hit, hits=h)          # noqa: E731
                ms = rates.block(w, cast, a.reps)
                hs = share()
                kms = rates.kernel_times(w, cast).get("q_capsulecast", (float("nan"), 0))[0]
                b = base[name]
                rows.append(dict(set=name, radius=rad, half_height=hh, rotation=rot_name, ms=ms, kernel_ms=kms, per_s=n / (ms * 1e-3), hit_share=hs,
                                 ray_ms=b["ray_ms"], sphere_ms=b["sphere_ms"], box_ms=b["box_ms"], vs_ray=ms / b["ray_ms"], vs_sphere=ms / b["sphere_ms"],
                                 vs_box=ms / b["box_ms"]))
    # hh = 0 is a sphere cast: the same walk, for the cost of the entry point itself
    t = rates.upload(w, rates.cast_records(incoherent, E.CAPSULE_CAST, radius=0.75))
    hh0_ms = rates.block(w, lambda: w.capsulecast_records(t, hits=h), a.reps)

    # 1 M capsule overlap queries around the world: half on a body, (r, hh) = (0.5, 0.5), random rotations; the same centres as spheres of radius 1
    orng = np.random.default_rng(3)
    live = scene["body_transforms"]["position"][1:].astype(np.float64)
    near = orng.random(n) < 0.5
    centres = np.where(near[:, None], live[orng.integers(0, len(live), size=n)] + orng.normal(scale=0.5, size=(n, 3)),
                       orng.uniform(lo, hi + np.array([0, 10, 0]), size=(n, 3)))
    qs = rates.overlap_queries(centres, (0.5, 0.5, 0.0), E.NH_SHAPE_CAPSULE, rotation=random_rot)
    sp = qs.copy()
    sp["shape"] = E.NH_SHAPE_SPHERE
    sp["size"][:, 0] = 1.0
    overlaps = []
    for oname, arr in (("capsule r 0.5 hh 0.5, random", qs), ("sphere r 1.0", sp)):
        qt = rates.upload(w, arr)
        ot = torch.empty(n + 1, dtype=torch.int32, device=w.dev)
        count_ms = rates.block(w, lambda: w.overlap_records(qt, offsets=ot), a.reps)
        total = rates.total_of(ot)
        ht = torch.empty((max(total, 1), 16), dtype=torch.uint8, device=w.dev)
        list_ms = rates.block(w, lambda: (w.overlap_records(qt, offsets=ot), w.overlap_records(qt, offsets=ot, hits=ht, capacity=total)), a.reps)
        overlaps.append(dict(query=oname, count_ms=count_ms, count_then_list_ms=list_ms, records=total))

    log = rates.Log()
    log.say(f"landed {land.name} world: {C:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; GPU {rates.gpu_name(w)}; {n:,} casts per set")
    log.say(f"{'set':<20}{'r':>5}{'hh':>5}{'rotation':>10}{'ms':>9}{'kernel ms':>11}{'M casts/s':>11}{'hits':>8}{'ray ms':>9}{'sphere ms':>11}{'box ms':>9}"
            f"{'/ray':>7}{'/sphere':>9}{'/box':>7}")
    for row in rows:
        log.say(f"{row['set']:<20}{row['radius']:5.2f}{row['half_height']:5.2f}{row['rotation']:>10}{row['ms']:9.3f}{row['kernel_ms']:11.3f}{row['per_s'] / 1e6:11.1f}"
                f"{100 * row['hit_share']:7.1f}%{row['ray_ms']:9.3f}{row['sphere_ms']:11.3f}{row['box_ms']:9.3f}{row['vs_ray']:7.2f}{row['vs_sphere']:9.2f}{row['vs_box']:7.2f}")
    for name, b in base.items():
        log.say(f"{name}: rays {b['ray_ms']:.3f} ms ({100 * b['ray_hits']:.1f}% hit), sphere casts r 0.75 {b['sphere_ms']:.3f} ms ({100 * b['sphere_hits']:.1f}% hit), "
                f"box casts h 0.75 {b['box_ms']:.3f} ms ({100 * b['box_hits']:.1f}% hit)")
    log.say(f"incoherent, hh 0 r 0.75 through nh_capsulecast: {hh0_ms:.3f} ms (nh_spherecast {base['incoherent']['sphere_ms']:.3f} ms)")
    for o in overlaps:
        log.say(f"overlap, {n:,} {o['query']}: count {o['count_ms']:.3f} ms, count + list {o['count_then_list_ms']:.3f} ms, {o['records']:,} records")
    log.say(json.dumps(dict(colliders=C, casts=n, base=base, capsules=rows, hh0_ms=hh0_ms, overlaps=overlaps)))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
