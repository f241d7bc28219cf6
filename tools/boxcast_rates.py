"""Box-cast rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "scene queries"): 1 M casts per set --
incoherent closest hit at two half extents (0.75, one body; 3.0) each with the identity and with random rotations, any hit, a coherent downward
grid -- and the same sets through nh_raycast and through nh_spherecast at radius 0.75 in the same run, so the cost of the box is a ratio measured on
one box.  Timed with device events; the per-kernel times of one cast of each set come from nh_kernel_times.

    python tools/boxcast_rates.py [--steps 70] [--reps 10]        (on a GPU box; prints the table, writes profiles/boxcast_rates.log)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boxcast_rates.log"))
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

    # the ray sets of tools/query_rates.py and tools/spherecast_rates.py (same seed, same construction)
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

    def kernel_ms(fn, name):
        w.enable_timing(True, only=name)
        w.kernel_times(reset=True)
        fn()
        w.synchronize()
        t = w.kernel_times(reset=True).get(name, (float("nan"), 0))[0]
        w.enable_timing(False)
        return t

    base = {}
    for name, rays, any_hit in (("incoherent", incoherent, False), ("incoherent any-hit", incoherent, True), ("coherent", coherent, False)):
        t = torch.from_numpy(rays.view(np.uint8).copy()).to(w.dev)
        ray_ms = timed(lambda: w.raycast_records(t, any_hit=any_hit, hits=h), a.reps)
        ray_share = share()
        c = np.zeros(n, dtype=E.SPHERE_CAST)
        for k in ("origin", "max_t", "direction", "ignore_body"):
            c[k] = rays[k]
        c["radius"] = 0.75
        t = torch.from_numpy(c.view(np.uint8).copy()).to(w.dev)
        sph_ms = timed(lambda: w.spherecast_records(t, any_hit=any_hit, hits=h), a.reps)
        base[name] = dict(ray_ms=ray_ms, ray_hits=ray_share, sphere_ms=sph_ms, sphere_hits=share())
    rows = []
    for name, rays, any_hit in (("incoherent", incoherent, False), ("incoherent any-hit", incoherent, True), ("coherent", coherent, False)):
        for size in (0.75, 3.0):
            for rot_name, rot in (("identity", None), ("random", random_rot)):
                c = np.zeros(n, dtype=E.BOX_CAST)
                for k in ("origin", "max_t", "direction", "ignore_body"):
                    c[k] = rays[k]
                c["size"] = size
                if rot is None:
                    c["rotation"][:, 3] = 1.0
                else:
                    c["rotation"] = rot
                t = torch.from_numpy(c.view(np.uint8).copy()).to(w.dev)
                ms = timed(lambda: w.boxcast_records(t, any_hit=any_hit, hits=h), a.reps)
                hs = share()
                kms = kernel_ms(lambda: w.boxcast_records(t, any_hit=any_hit, hits=h), "q_boxcast")
                b = base[name]
                rows.append(dict(set=name, size=size, rotation=rot_name, ms=ms, kernel_ms=kms, per_s=n / (ms * 1e-3), hit_share=hs,
                                 ray_ms=b["ray_ms"], sphere_ms=b["sphere_ms"], vs_ray=ms / b["ray_ms"], vs_sphere=ms / b["sphere_ms"]))
    # size 0 is a ray: the same walk, for the cost of the entry point itself
    c = np.zeros(n, dtype=E.BOX_CAST)
    for k in ("origin", "max_t", "direction", "ignore_body"):
        c[k] = incoherent[k]
    c["rotation"][:, 3] = 1.0
    t = torch.from_numpy(c.view(np.uint8).copy()).to(w.dev)
    s0_ms = timed(lambda: w.boxcast_records(t, hits=h), a.reps)

    out = io.StringIO()
    print(f"landed config-2 world: {C:,} colliders, {nb:,} bodies, after {a.steps} steps; GPU {torch.cuda.get_device_name(w.dev)}; {n:,} casts per set", file=out)
    print(f"{'set':<20}{'size':>6}{'rotation':>10}{'ms':>9}{'kernel ms':>11}{'M casts/s':>11}{'hits':>8}{'ray ms':>9}{'sphere ms':>11}{'box/ray':>9}{'box/sphere':>12}", file=out)
    for row in rows:
        print(f"{row['set']:<20}{row['size']:6.2f}{row['rotation']:>10}{row['ms']:9.3f}{row['kernel_ms']:11.3f}{row['per_s'] / 1e6:11.1f}{100 * row['hit_share']:7.1f}%"
              f"{row['ray_ms']:9.3f}{row['sphere_ms']:11.3f}{row['vs_ray']:9.2f}{row['vs_sphere']:12.2f}", file=out)
    for name, b in base.items():
        print(f"{name}: rays {b['ray_ms']:.3f} ms ({100 * b['ray_hits']:.1f}% hit), sphere casts r 0.75 {b['sphere_ms']:.3f} ms ({100 * b['sphere_hits']:.1f}% hit)", file=out)
    print(f"incoherent, size 0 through nh_boxcast: {s0_ms:.3f} ms (nh_raycast {base['incoherent']['ray_ms']:.3f} ms)", file=out)
    print(json.dumps(dict(colliders=C, casts=n, base=base, boxes=rows, size0_ms=s0_ms)), file=out)
    text = out.getvalue()
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    w.close()


if __name__ == "__main__":
    main()
