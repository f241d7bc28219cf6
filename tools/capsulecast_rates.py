"""Capsule-cast and capsule-overlap rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "scene queries"):
1 M casts per set -- incoherent closest hit at (r, hh) = (0.5, 0.5) and (1.0, 2.0), each with the identity (upright) and with random rotations, any
hit, a coherent downward grid -- beside the same sets through nh_raycast, nh_spherecast at radius 0.75 and nh_boxcast at half extent 0.75 in the same
run, so the cost of the capsule is a ratio measured on one box; then 1 M capsule overlap queries, count only and list.  Timed with device events;
the per-kernel times of one call come from nh_kernel_times.

    python tools/capsulecast_rates.py [--steps 70] [--reps 10]        (on a GPU box; prints the table, writes profiles/capsulecast_rates.log)
"""
import argparse
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=70)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--casts", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capsulecast_rates.log"))
    a = ap.parse_args()
    import torch
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
    C = len(scene["box_tags"]) + len(scene["sphere_tags"])
    w = E.World(scene, flags=E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP, max_contacts=6 * nb)
    w.step(a.steps)
    w.query_build()
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

    # the ray sets of tools/query_rates.py, spherecast_rates.py and boxcast_rates.py (same seed, same construction)
    rng = np.random.default_rng(1)
    n = a.casts
    slab_p, slab_h = scene["box_transforms"]["position"][:124].astype(np.float64), scene["box_data"]["size"][:124].astype(np.float64)
    lo, hi = (slab_p - slab_h).min(axis=0), (slab_p + slab_h).max(axis=0)
    r = np.zeros(n, dtype=E.RAY)
    r["max_t"] = np.inf; r["ignore_body"] = 0xFFFFFFFF
    r["origin"] = rng.uniform(lo, hi + np.array([0, 60, 0]), size=(n, 3))
    d = rng.normal(size=(n, 3)); r["direction"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    incoherent = r.copy()
    side = 1024
    gx, gz = np.meshgrid(np.linspace(lo[0], hi[0], side), np.linspace(lo[2], hi[2], n // side))
    r["origin"][:, 0] = gx.reshape(-1); r["origin"][:, 1] = 30.0; r["origin"][:, 2] = gz.reshape(-1)
    r["direction"] = (0.0, -1.0, 0.0)
    coherent = r.copy()
    q = np.random.default_rng(2).normal(size=(n, 4))
    random_rot = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)

    h = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)

    def share():
        hits = np.frombuffer(h.cpu().numpy().tobytes(), dtype=E.RAY_HIT)
        return float((hits["shape"] != 0xFFFFFFFF).mean())

    def kernel_ms(fn, names):
        w.enable_timing(True)
        w.kernel_times(reset=True)
        fn()
        w.synchronize()
        kt = w.kernel_times(reset=True)
        w.enable_timing(False)
        return sum(kt.get(name, (float("nan"), 0))[0] for name in names)

    def upload(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).to(w.dev)

    def fill(dtype, rays):
        c = np.zeros(len(rays), dtype=dtype)
        for k in ("origin", "max_t", "direction", "ignore_body"):
            c[k] = rays[k]
        return c

    sets = (("incoherent", incoherent, False), ("incoherent any-hit", incoherent, True), ("coherent", coherent, False))
    base = {}
    for name, rays, any_hit in sets:
        t = upload(rays)
        ray_ms = timed(lambda: w.raycast_records(t, any_hit=any_hit, hits=h), a.reps)
        ray_share = share()
        c = fill(E.SPHERE_CAST, rays)
        c["radius"] = 0.75
        t = upload(c)
        sph_ms = timed(lambda: w.spherecast_records(t, any_hit=any_hit, hits=h), a.reps)
        sph_share = share()
        c = fill(E.BOX_CAST, rays)
        c["size"] = 0.75
        c["rotation"][:, 3] = 1.0
        t = upload(c)
        box_ms = timed(lambda: w.boxcast_records(t, any_hit=any_hit, hits=h), a.reps)
        base[name] = dict(ray_ms=ray_ms, ray_hits=ray_share, sphere_ms=sph_ms, sphere_hits=sph_share, box_ms=box_ms, box_hits=share())
    rows = []
    for name, rays, any_hit in sets:
        for rad, hh in ((0.5, 0.5), (1.0, 2.0)):
            for rot_name, rot in (("identity", None), ("random", random_rot)):
                c = fill(E.CAPSULE_CAST, rays)
                c["radius"], c["half_height"] = rad, hh
                if rot is None:
                    c["rotation"][:, 3] = 1.0
                else:
                    c["rotation"] = rot
                t = upload(c)
                ms = timed(lambda: w.capsulecast_records(t, any_hit=any_hit, hits=h), a.reps)
                hs = share()
                kms = kernel_ms(lambda: w.capsulecast_records(t, any_hit=any_hit, hits=h), ("q_capsulecast",))
                b = base[name]
                rows.append(dict(set=name, radius=rad, half_height=hh, rotation=rot_name, ms=ms, kernel_ms=kms, per_s=n / (ms * 1e-3), hit_share=hs,
                                 ray_ms=b["ray_ms"], sphere_ms=b["sphere_ms"], box_ms=b["box_ms"], vs_ray=ms / b["ray_ms"], vs_sphere=ms / b["sphere_ms"],
                                 vs_box=ms / b["box_ms"]))
    # hh = 0 is a sphere cast: the same walk, for the cost of the entry point itself
    c = fill(E.CAPSULE_CAST, incoherent)
    c["radius"] = 0.75
    c["rotation"][:, 3] = 1.0
    t = upload(c)
    hh0_ms = timed(lambda: w.capsulecast_records(t, hits=h), a.reps)

    # 1 M capsule overlap queries around the world: half on a body, (r, hh) = (0.5, 0.5), random rotations; the same centres as spheres of radius 1
    orng = np.random.default_rng(3)
    live = scene["body_transforms"]["position"][1:].astype(np.float64)
    qs = np.zeros(n, dtype=E.OVERLAP_QUERY)
    near = orng.random(n) < 0.5
    qs["center"] = np.where(near[:, None], live[orng.integers(0, len(live), size=n)] + orng.normal(scale=0.5, size=(n, 3)),
                            orng.uniform(lo, hi + np.array([0, 10, 0]), size=(n, 3)))
    qs["shape"] = E.NH_SHAPE_CAPSULE
    qs["size"][:, 0], qs["size"][:, 1] = 0.5, 0.5
    qs["rotation"] = random_rot
    qs["ignore_body"] = 0xFFFFFFFF
    sp = qs.copy()
    sp["shape"] = E.NH_SHAPE_SPHERE
    sp["size"][:, 0] = 1.0
    overlaps = []
    for oname, arr in (("capsule r 0.5 hh 0.5, random", qs), ("sphere r 1.0", sp)):
        qt = upload(arr)
        ot = torch.empty(n + 1, dtype=torch.int32, device=w.dev)
        count_ms = timed(lambda: w.overlap_records(qt, offsets=ot), a.reps)
        total = int(ot[n].item()) & 0xFFFFFFFF
        ht = torch.empty((max(total, 1), 16), dtype=torch.uint8, device=w.dev)
        list_ms = timed(lambda: (w.overlap_records(qt, offsets=ot), w.overlap_records(qt, offsets=ot, hits=ht, capacity=total)), a.reps)
        overlaps.append(dict(query=oname, count_ms=count_ms, count_then_list_ms=list_ms, records=total))

    out = io.StringIO()
    print(f"landed config-2 world: {C:,} colliders, {nb:,} bodies, after {a.steps} steps; GPU {torch.cuda.get_device_name(w.dev)}; {n:,} casts per set", file=out)
    print(f"{'set':<20}{'r':>5}{'hh':>5}{'rotation':>10}{'ms':>9}{'kernel ms':>11}{'M casts/s':>11}{'hits':>8}{'ray ms':>9}{'sphere ms':>11}{'box ms':>9}"
          f"{'/ray':>7}{'/sphere':>9}{'/box':>7}", file=out)
    for row in rows:
        print(f"{row['set']:<20}{row['radius']:5.2f}{row['half_height']:5.2f}{row['rotation']:>10}{row['ms']:9.3f}{row['kernel_ms']:11.3f}{row['per_s'] / 1e6:11.1f}"
              f"{100 * row['hit_share']:7.1f}%{row['ray_ms']:9.3f}{row['sphere_ms']:11.3f}{row['box_ms']:9.3f}{row['vs_ray']:7.2f}{row['vs_sphere']:9.2f}{row['vs_box']:7.2f}",
              file=out)
    for name, b in base.items():
        print(f"{name}: rays {b['ray_ms']:.3f} ms ({100 * b['ray_hits']:.1f}% hit), sphere casts r 0.75 {b['sphere_ms']:.3f} ms ({100 * b['sphere_hits']:.1f}% hit), "
              f"box casts h 0.75 {b['box_ms']:.3f} ms ({100 * b['box_hits']:.1f}% hit)", file=out)
    print(f"incoherent, hh 0 r 0.75 through nh_capsulecast: {hh0_ms:.3f} ms (nh_spherecast {base['incoherent']['sphere_ms']:.3f} ms)", file=out)
    for o in overlaps:
        print(f"overlap, {n:,} {o['query']}: count {o['count_ms']:.3f} ms, count + list {o['count_then_list_ms']:.3f} ms, {o['records']:,} records", file=out)
    print(json.dumps(dict(colliders=C, casts=n, base=base, capsules=rows, hh0_ms=hh0_ms, overlaps=overlaps)), file=out)
    text = out.getvalue()
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    w.close()


if __name__ == "__main__":
    main()
