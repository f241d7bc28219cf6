"""nh_sweep / nh_sweep_limit rates on the landed config-2 world (include/nudge_hip.h, "fast bodies"), and beside them in the same process the
yardstick of the walk: nh_boxcast -- a kernel this feature does not touch -- on the very cast records nh_sweep wrote.  What a guarded step pays is
the select pass (flag, scan, gather) over every collider, whoever moves; the walk is paid per fast collider.

    cases     (a) the world at rest: the select pass alone;  (b) --thrown bodies (2,048) thrown at --speed (100 m/s) over the world at rest;
              (c) every body given --speed.  The momentum is written with set_bodies before each case and the world is not stepped.
    per case  nh_sweep without and with `hits`; nh_sweep_limit (on a list whose momentum is put back between blocks: it scales what it reads);
              nh_boxcast on the records nh_sweep wrote; a still nh_step(1) and an nh_query_refit from the same run, for scale (case (a) only:
              stepping moves the world).  ms per call as the best (and median) of --reps blocks of --inner calls after a warm-up, by device events
              around the block.  walk = nh_sweep with hits - nh_sweep without; the ratio walk / nh_boxcast and the select pass as a share of a step
              are what DESIGN 10.27 quotes.  A spot check of 258 entries against the host oracle (tests/hostsweep_util.py) in cases (b) and (c).

(On rates.py; not a *_rates.py: it also times the step and the refit beside its series.)

    python tools/fast_bodies.py [--steps 70] [--reps 5] [--inner 5] [--out profiles/sweep_rates.log]
    (on a GPU box; prints the table, one JSON line at the end, and writes both to --out)
"""
import json

import numpy as np

import rates
from nudge_amd import engine as E           # noqa: E402


def main():
    ap = rates.parser("sweep_rates")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--thrown", type=int, default=2048)
    ap.add_argument("--speed", type=float, default=100.0)
    a = ap.parse_args()
    import torch
    import hostcast_util as HC
    import hostsweep_util as HS
    land = rates.landed(a)
    w, scene, log = land.world, land.scene, rates.Log()
    rng = np.random.default_rng(1)
    n = w.nbox + w.nsph
    dt = scene["params"]["time_step"]

    def timed(fn):
        return rates.best_median(rates.blocks(w, fn, a.reps, a.inner))

    log.say(f"landed {land.name} world: {n:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; GPU {rates.gpu_name(w)}")
    log.say(f"ms per call: the best (median) of {a.reps} blocks of {a.inner} calls after a warm-up, device events around the block; one box, one run.")
    step_ms = timed(lambda: w.step(1))
    refit_ms = timed(lambda: w.query_refit())
    w.synchronize()
    w.query_refit()
    rest = w.get_bodies()["momentum"].copy()
    log.say(f"  for scale: nh_step(1) {step_ms[0]:.3f} ({step_ms[1]:.3f})   nh_query_refit {refit_ms[0]:.3f} ({refit_ms[1]:.3f})")
    nb = land.bodies
    some = rest.copy()
    fast = rng.choice(np.arange(1, nb), size=min(a.thrown, nb - 1), replace=False)
    some["velocity"][fast] = a.speed * rates.unit_rows(rng.normal(size=(len(fast), 3)))
    every = rest.copy()
    every["velocity"][1:] = a.speed * rates.unit_rows(rng.normal(size=(nb - 1, 3)))
    cases = [("(a) at rest", rest), (f"(b) {len(fast):,} bodies at {a.speed:g} m/s", some), (f"(c) every body at {a.speed:g} m/s", every)]
    log.say(f"  {'case':34s} {'selected':>10s} {'hit share':>9s} | {'sweep, no hits':>16s} {'sweep, hits':>16s} {'sweep_limit':>16s} {'nh_boxcast':>16s} | walk / boxcast   select / step")
    counts = torch.zeros(2, dtype=torch.int32, device=w.dev)
    colliders = torch.empty(n, dtype=torch.int32, device=w.dev)
    casts = torch.empty((n, 64), dtype=torch.uint8, device=w.dev)
    hits = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
    cast_hits = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
    out = {}
    for name, bm in cases:
        w.set_bodies(momentum=bm)
        lst = w.sweep_records(dt, capacity=n, counts=counts, colliders=colliders, casts=casts, hits=hits)
        w.synchronize()
        k = int(counts.sum())
        r = {}
        r["select"] = timed(lambda: w.sweep_records(dt, capacity=n, counts=counts, colliders=colliders, casts=casts))
        r["sweep"] = timed(lambda: w.sweep_records(dt, capacity=n, counts=counts, colliders=colliders, casts=casts, hits=hits))
        # (the limit scales the momentum it reads: each block starts from the case's own)
        limit = []
        for _ in range(a.reps):
            w.set_bodies(momentum=bm)
            limit += rates.blocks(w, lambda: w.sweep_limit_records(lst), 1, 1, warm=0)
        r["limit"] = rates.best_median(limit)
        w.set_bodies(momentum=bm)
        r["boxcast"] = timed(lambda: w.boxcast_records(casts[:max(k, 1)], hits=cast_hits)) if k else (0.0, 0.0)
        w.synchronize()
        got = rates.download(hits[:k], E.RAY_HIT)
        share = float((got["shape"] != rates.NONE).mean()) if k else 0.0
        if k:
            # the box entries against nh_boxcast's records (every entry of this world is a box but the few of tiles with spheres)
            kb = int(counts[0])
            assert torch.equal(hits[:kb], cast_hits[:kb]), f"{name}: nh_sweep differs from nh_boxcast on its own records"
            at = rates.spot(k)
            rec, bodies = land.records, w.get_bodies()
            ref = HS.sweep(rec, w.nbox, bodies["transforms"], bm, time_step=dt, channels=("colliders", "casts"))
            assert ref["total"] == k and np.array_equal(ref["colliders"][:k], rates.download(colliders[:k], np.uint32))
            mine = rates.download(casts[:k], E.BOX_CAST)[at]
            assert mine.tobytes() == ref["casts"][:k][at].tobytes(), f"{name}: cast records differ from the oracle"
            box = ref["colliders"][:k][at] < w.nbox
            want = np.zeros(len(at), dtype=E.RAY_HIT)
            want[box] = HC.cast(HC.BOX, rec, w.nbox, mine[box])
            want[~box] = HC.cast(HC.CAPSULE, rec, w.nbox, mine[~box].view(E.CAPSULE_CAST))
            assert got[at].tobytes() == want.tobytes(), f"{name}: hits differ from the oracle"
        walk = r["sweep"][0] - r["select"][0]
        ratio = walk / r["boxcast"][0] if k else float("nan")
        cell = lambda key: f"{r[key][0]:7.3f} ({r[key][1]:7.3f})"      # noqa: E731
        log.say(f"  {name:34s} {k:10,d} {share:9.3f} | {cell('select')} {cell('sweep')} {cell('limit')} {cell('boxcast')} | {ratio:14.2f}   {r['select'][0] / step_ms[0]:13.2f}")
        out[name] = dict(selected=k, hit_share=share, walk_ms=walk, walk_over_boxcast=ratio, select_over_step=r["select"][0] / step_ms[0],
                         **{key: dict(best_ms=v[0], median_ms=v[1]) for key, v in r.items()})
    log.say("  cases (b), (c): the hits equal nh_boxcast's on nh_sweep's own records byte for byte, and 258 entries equal the host oracle")
    log.say()
    log.say(json.dumps(dict(colliders=n, steps=a.steps, step_ms=step_ms[0], refit_ms=refit_ms[0], cases=out)))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
