"""Sphere-cast rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "scene queries"): 1 M casts per set --
incoherent closest hit at two radii (about half a body's size and about two bodies' size), any hit, a coherent downward grid -- and the same ray sets
through nh_raycast in the same run, so the cost of the radius is a ratio measured on one box.  Timed with device events.

    python tools/spherecast_rates.py [--steps 70] [--reps 10]        (on a GPU box; prints the table, one JSON line at the end)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=70)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--casts", type=int, default=1 << 20)
    a = ap.parse_args()
    import torch
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
    C = len(scene["box_tags"]) + len(scene["sphere_tags"])
    body_half = float(np.median(scene["box_data"]["size"][124:]))
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

    # the ray sets of tools/query_rates.py (same seed, same construction)
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

    small, large = 0.5 * 2 * body_half, 2.0 * 2 * body_half          # about half a body's size, about two bodies' size
    sets = [("incoherent", incoherent, False, small), ("incoherent", incoherent, False, large), ("incoherent any-hit", incoherent, True, small),
            ("incoherent any-hit", incoherent, True, large), ("coherent", coherent, False, small), ("coherent", coherent, False, large)]
    h = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
    ray_rows = {}
    for name, rays, any_hit in (("incoherent", incoherent, False), ("incoherent any-hit", incoherent, True), ("coherent", coherent, False)):
        t = torch.from_numpy(rays.view(np.uint8).copy()).to(w.dev)
        ms = timed(lambda: w.raycast_records(t, any_hit=any_hit, hits=h), a.reps)
        hits = np.frombuffer(h.cpu().numpy().tobytes(), dtype=E.RAY_HIT)
        ray_rows[name] = dict(ms=ms, per_s=n / (ms * 1e-3), hit_share=float((hits["shape"] != 0xFFFFFFFF).mean()))
    rows = []
    for name, rays, any_hit, radius in sets:
        c = np.zeros(n, dtype=E.SPHERE_CAST)
        for k in ("origin", "max_t", "direction", "ignore_body"):
            c[k] = rays[k]
        c["radius"] = radius
        t = torch.from_numpy(c.view(np.uint8).copy()).to(w.dev)
        ms = timed(lambda: w.spherecast_records(t, any_hit=any_hit, hits=h), a.reps)
        hits = np.frombuffer(h.cpu().numpy().tobytes(), dtype=E.RAY_HIT)
        rows.append(dict(set=name, radius=radius, ms=ms, per_s=n / (ms * 1e-3), hit_share=float((hits["shape"] != 0xFFFFFFFF).mean()),
                         ray_ms=ray_rows[name]["ms"], cost=ms / ray_rows[name]["ms"]))
    # radius 0 is a ray: the same walk, for the cost of the entry point itself
    c = np.zeros(n, dtype=E.SPHERE_CAST)
    for k in ("origin", "max_t", "direction", "ignore_body"):
        c[k] = incoherent[k]
    t = torch.from_numpy(c.view(np.uint8).copy()).to(w.dev)
    r0_ms = timed(lambda: w.spherecast_records(t, hits=h), a.reps)

    print(f"landed config-2 world: {C:,} colliders, {nb:,} bodies, after {a.steps} steps; GPU {torch.cuda.get_device_name(w.dev)}; "
          f"median body half extent {body_half:.3f}")
    print(f"{'set':<20}{'radius':>8}{'ms':>9}{'M casts/s':>11}{'hits':>8}{'ray ms':>9}{'M rays/s':>10}{'ray hits':>10}{'cast / ray':>12}")
    for row in rows:
        rr = ray_rows[row["set"]]
        print(f"{row['set']:<20}{row['radius']:8.3f}{row['ms']:9.3f}{row['per_s'] / 1e6:11.1f}{100 * row['hit_share']:7.1f}%{rr['ms']:9.3f}"
              f"{rr['per_s'] / 1e6:10.1f}{100 * rr['hit_share']:9.1f}%{row['cost']:12.2f}")
    print(f"incoherent, radius 0 through nh_spherecast: {r0_ms:.3f} ms (nh_raycast {ray_rows['incoherent']['ms']:.3f} ms)")
    print(json.dumps(dict(colliders=C, casts=n, body_half=body_half, rays=ray_rows, sweeps=rows, radius0_ms=r0_ms)))
    w.close()


if __name__ == "__main__":
    main()
