"""nh_walk rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "nh_walk"): 1,048,576 walks of the upright
capsule r = 0.3, hh = 0.4 (skin 0.01, max_slides 4, snap distance 0.3) that stand one skin above the ground slab beside a resting body (half of them) or above
a resting body's top (the other half) and are sent 0.5 - 2 units horizontally -- those on the slab towards their body -- in four CONFIGURATIONS: step height 0
or 1.0, slope limit off or 45 degrees.  BESIDE each, in the same process, nh_capsulecast on the first casts { origin, 1, displacement, ... } -- device events,
interleaved, the median [min .. max] of --repeats blocks of --reps calls after two warm-ups.  Logged with the times: how the walks ended, the mean number
of casts a walk made, and THE RATIO the documents quote: the walk call's time over (mean casts per walk x the capsule cast's time) -- 1 if a walk cost
exactly its casts; what is above it is divergence (a lane that has finished waits for the slowest of its wave) and the later casts being short and
incoherent.  For step height 1.0 with the limit off, the HOST LOOP of the REPLAY identity is timed as well (wall clock, its uploads and downloads included: nh_move
calls for the phases, an nh_capsulecast call for the probe and one per round of the first slide, tests/hostmover_util.py replay_walk) and compared byte for
byte.  258 walks of every configuration are compared byte for byte with the brute force over all colliders (tests/hostmover_util.py).

With NUDGE_HIP_LIBRARY naming another build of the library (the parent commit's: tools/build_variant.sh parent "" <rev>), a second world on THAT library
answers nh_move and nh_capsulecast on the same records, filter off, interleaved with this library's: the same bytes, and the ratio of the times.

    [NUDGE_HIP_LIBRARY=.../libparent.so] python tools/walk_rates.py [--steps 70] [--reps 10] [--repeats 5] [--out profiles/walk_rates.log]
    (on a GPU box; prints the table, one JSON line at the end, and writes both to --out)
"""
import json
import os
import time

import numpy as np

import rates
OTHER = rates.other_library()
from nudge_amd import engine as E           # noqa: E402

CONFIGS = (("step 0, limit off", 0.0, 0.0), ("step 0, limit 45", 0.0, 45.0), ("step 1.0, limit off", 1.0, 0.0), ("step 1.0, limit 45", 1.0, 45.0))


def main():
    ap = rates.parser("walk_rates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--walks", type=int, default=1 << 20)
    ap.add_argument("--max-slides", type=int, default=4)
    ap.add_argument("--no-check", action="store_true", help="skip the brute-force spot check")
    a = ap.parse_args()
    import torch
    import hostmover_util as MV
    from hostmover_util import CAPSULE as HW
    import walk_batches as WB
    land = rates.landed(a)
    other = rates.landed(a, OTHER, like=land).world if OTHER else None
    w, C, n, rec = land.world, land.colliders, a.walks, land.records
    up, down, fmt, log = rates.upload, rates.download, rates.fmt, rates.Log()
    R, HH = 0.3, 0.4
    x, top, z, d = rates.walk_batch(np.random.default_rng(1), n, rec, WB._tops(rec, w.nbox))
    base = HW.walks(WB.stand(x, top, z, R, HH), d, R, HH, skin=WB.SKIN, max_slides=a.max_slides, snap_distance=0.3)
    casts = HW.first_casts(HW.head(base))
    ct = up(w, casts)
    ht = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
    rt = torch.empty((n, 112), dtype=torch.uint8, device=w.dev)
    log.say(f"landed {land.name} world: {C:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; GPU {rates.gpu_name(w)}")
    log.say(f"{n:,} walks (r {R}, hh {HH}, max_slides {a.max_slides}, snap 0.3; half on the slab beside a body, half on a body's top); median of {a.repeats} blocks of "
            f"{a.reps} calls, interleaved (min .. max of the blocks); one box, one run")
    result = dict(colliders=C, steps=a.steps, walks=n, max_slides=a.max_slides, configs={})
    pick = rates.spot(n)
    for name, step, limit in CONFIGS:
        wk = base.copy()
        wk["step_height"], wk["min_ground_up"] = step, MV.cos_deg(limit)
        wt = up(w, wk)
        t = rates.spreads(rates.interleaved(w, dict(walk=lambda: w.walk_records(wt, results=rt), capsulecast=lambda: w.capsulecast_records(ct, hits=ht)), a.reps, a.repeats))
        got = down(rt, E.WALK_RESULT)
        checked = 0
        if not a.no_check:
            assert got[pick].tobytes() == HW.walk(rec, w.nbox, wk[pick]).tobytes(), "the GPU differs from the brute force"
            checked = len(pick)
        s = MV.shares(wk, got)
        s["start_overlap"] = float(((got["flags"] & E.NH_MOVE_START_OVERLAP) != 0).mean())
        mean_casts = float(got["casts"].mean())
        ratio = t["walk"]["ms"] / (mean_casts * t["capsulecast"]["ms"])
        log.say(f"{name}:")
        log.say(f"  nh_walk                               {fmt(t['walk'])} ms")
        log.say(f"  nh_capsulecast, the first casts       {fmt(t['capsulecast'])} ms")
        log.say(f"  shares: {({k: round(v, 4) for k, v in s.items()})}")
        log.say(f"  casts per walk, mean                  {mean_casts:.3f}   (most in one walk {int(got['casts'].max())})")
        log.say(f"  nh_walk / (mean casts x capsulecast)  {ratio:.2f}")
        log.say(f"  {checked} walks equal the brute force byte for byte")
        result["configs"][name] = dict(walk=t["walk"], capsulecast=t["capsulecast"], shares=s, mean_casts=mean_casts, ratio=ratio, checked_against_brute_force=checked)
        if step > 0 and limit == 0:
            # the host loop of the REPLAY identity, on the whole batch: wall clock, its transfers included
            def move(m):
                return down(w.move_records(up(w, m)), E.MOVE_RESULT)

            def cast(c):
                return down(w.capsulecast_records(up(w, c)), E.RAY_HIT)
            HW.replay_walk(wk[:4096], move, cast)
            torch.cuda.current_stream(w.dev).synchronize()
            t0 = time.perf_counter()
            ref, calls = HW.replay_walk(wk, move, cast)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert ref.tobytes() == got.tobytes(), "the host loop differs from nh_walk"
            log.say(f"  the host loop of the REPLAY identity   {host_ms:.1f} ms wall clock, {calls} GPU calls with their uploads and downloads; the same bytes;"
                    f" nh_walk is {host_ms / t['walk']['ms']:.0f} times faster")
            result["configs"][name]["host_loop"] = dict(ms=host_ms, calls=calls)
    if other is not None:
        mv = HW.head(base)
        mt, mto, cto = up(w, mv), up(other, mv), up(other, casts)
        r64 = {k: torch.empty((n, 64), dtype=torch.uint8, device=w.dev) for k in ("this", "other")}
        h32 = {k: torch.empty((n, 32), dtype=torch.uint8, device=w.dev) for k in ("this", "other")}
        t = rates.spreads(rates.interleaved(w, {"move this": lambda: w.move_records(mt, results=r64["this"]), "move other": lambda: other.move_records(mto, results=r64["other"]),
                                                "capsulecast this": lambda: w.capsulecast_records(ct, hits=h32["this"]),
                                                "capsulecast other": lambda: other.capsulecast_records(cto, hits=h32["other"])}, a.reps, a.repeats))
        assert torch.equal(r64["this"], r64["other"]) and torch.equal(h32["this"], h32["other"]), "the two libraries differ"
        log.say(f"filter off, this library beside {os.path.basename(OTHER)} (the same bytes from both):")
        for call in ("move", "capsulecast"):
            ratio = t[call + " this"]["ms"] / t[call + " other"]["ms"]
            log.say(f"  nh_{call:<12} this {fmt(t[call + ' this'])} ms   other {fmt(t[call + ' other'])} ms   this / other {ratio:.3f} (medians)")
            result[call + "_beside_other"] = dict(this=t[call + " this"], other=t[call + " other"], ratio=ratio)
        other.close()
    else:
        log.say("filter off, this library beside another build: no NUDGE_HIP_LIBRARY given, not measured")
    log.say()
    log.say(json.dumps(result))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
