"""nh_sense rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "sensors"), and beside them in the same
process the yardstick: nh_raycast -- a kernel this change does not touch -- on the very nh_Ray records nh_sense_rays materialised for the same sensors
and pattern, and the cost of nh_sense_rays itself.  A caller without nh_sense pays (its own ray generation or an upload) + nh_raycast and reads 32 bytes
a ray; nh_sense reads 48 bytes a sensor and writes 4 bytes a ray and channel.

    cases     --cameras sensors x (--side x --side) pinhole beams in 8 x 8 tiles, and the same pattern in row-major order;
              --lidars sensors x a (--rings x --azimuths) lidar.  The sensors ride on dynamic bodies, two units above their centres, and ignore them.
    per case  nh_sense writing t only, t + body, the full hit records; nh_sense_rays; nh_raycast on those rays (32-byte hits).
              ms per call as the best (and median) of --reps blocks of --inner calls after a warm-up, by device events around the block; G rays / s
              from the best.  t of nh_sense and of nh_raycast's records are compared byte for byte.

    python tools/sense_rates.py [--steps 70] [--reps 5] [--inner 5] [--out profiles/sense_rates.log]
    (on a GPU box; prints the table, one JSON line at the end, and writes both to --out)
"""
import json

import numpy as np

import rates
from nudge_amd import engine as E           # noqa: E402


def main():
    ap = rates.parser("sense_rates", side_flag="--world-side")          # (--side is the camera image's here)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--cameras", type=int, default=4096)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--lidars", type=int, default=256)
    ap.add_argument("--rings", type=int, default=64)
    ap.add_argument("--azimuths", type=int, default=1024)
    a = ap.parse_args()
    import torch
    land = rates.landed(a)
    w, scene, log = land.world, land.scene, rates.Log()
    rng = np.random.default_rng(1)
    dynamic = np.unique(np.concatenate([scene["box_transforms"]["body"], scene["sphere_transforms"]["body"]]))
    dynamic = dynamic[dynamic != 0]

    def riders(n):
        """n sensors on random dynamic bodies: two units up their local y, a random turn about it, the carrier ignored."""
        s = np.zeros(n, dtype=E.SENSOR)
        s["body"] = s["ignore_body"] = rng.choice(dynamic, size=n)
        s["position"] = (0.0, 2.0, 0.0)
        yaw = rng.uniform(0.0, 2 * np.pi, size=n)
        s["rotation"][:, 1], s["rotation"][:, 3] = np.sin(0.5 * yaw), np.cos(0.5 * yaw)
        return s

    def timed(fn):
        return rates.best_median(rates.blocks(w, fn, a.reps, a.inner))

    tiled, _ = E.pinhole_beams(a.side, a.side, np.radians(60.0), 200.0)
    rows, _ = E.pinhole_beams(a.side, a.side, np.radians(60.0), 200.0, tile=1)
    lidar = E.lidar_beams(np.linspace(0.0, 2 * np.pi, a.azimuths, endpoint=False), np.radians(np.linspace(-25.0, 15.0, a.rings)), 200.0)
    cams, lids = riders(a.cameras), riders(a.lidars)
    cases = [(f"pinhole {a.side} x {a.side}, 8 x 8 tiles", cams, tiled), (f"pinhole {a.side} x {a.side}, row-major", cams, rows),
             (f"lidar {a.rings} x {a.azimuths}", lids, lidar)]
    log.say(f"landed {land.name} world: {w.nbox + w.nsph:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; GPU {rates.gpu_name(w)}")
    log.say(f"ms per call: the best (median) of {a.reps} blocks of {a.inner} calls after a warm-up, device events around the block; one box, one run.  "
            f"G/s: 1e9 rays a second from the best.")
    log.say(f"  {'case':36s} {'sensors':>8s} {'rays':>12s} {'hit share':>9s} | {'sense t':>16s} {'t + body':>16s} {'full hits':>16s} | {'sense_rays':>16s} {'nh_raycast':>16s} | raycast / sense t")
    out = {}
    for name, sensors, beams in cases:
        st, bm = rates.upload(w, sensors), rates.upload(w, beams)
        n = len(sensors) * len(beams)
        t = torch.empty(n, dtype=torch.float32, device=w.dev)
        body = torch.empty(n, dtype=torch.int32, device=w.dev)
        hits = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
        rays = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
        cast = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
        w.sense_rays_records(st, bm, rays=rays)
        r = {}
        r["sense_t"] = timed(lambda: w.sense_records(st, bm, t=t))
        r["sense_t_body"] = timed(lambda: w.sense_records(st, bm, t=t, body=body))
        r["sense_hits"] = timed(lambda: w.sense_records(st, bm, hits=hits))
        r["sense_rays"] = timed(lambda: w.sense_rays_records(st, bm, rays=rays))
        r["raycast"] = timed(lambda: w.raycast_records(rays, hits=cast))
        w.sense_records(st, bm, t=t, body=body)
        torch.cuda.current_stream(w.dev).synchronize()
        same = bool(torch.equal(t.view(torch.int32), cast.view(torch.int32).reshape(n, 8)[:, 0])) and bool(torch.equal(hits, cast))
        assert same, f"{name}: nh_sense differs from nh_raycast on nh_sense_rays' records"
        share = float((body != -1).float().mean())
        cell = lambda k: f"{r[k][0]:7.3f} ({r[k][1]:7.3f})"      # noqa: E731
        log.say(f"  {name:36s} {len(sensors):8,d} {n:12,d} {share:9.3f} | {cell('sense_t')} {cell('sense_t_body')} {cell('sense_hits')} | {cell('sense_rays')} {cell('raycast')} | "
                f"{r['raycast'][0] / r['sense_t'][0]:.2f} x  ({n / r['sense_t'][0] / 1e6:.2f} against {n / r['raycast'][0] / 1e6:.2f} G/s)")
        out[name] = dict(sensors=len(sensors), beams=len(beams), rays=n, hit_share=share, same_bytes=same,
                         **{k: dict(best_ms=v[0], median_ms=v[1], grays_per_s=n / v[0] / 1e6) for k, v in r.items()})
        del t, body, hits, rays, cast
    log.say("  every case: t and the hit records of nh_sense equal nh_raycast's on nh_sense_rays' records byte for byte")
    log.say()
    log.say(json.dumps(dict(colliders=w.nbox + w.nsph, steps=a.steps, cases=out)))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
