"""nh_boxmove and nh_boxwalk rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "nh_boxmove, nh_boxwalk"),
2^20 records each, timed by the LIBRARY'S KERNEL TIMERS (nh_enable_timing / nh_kernel_times: device events around each launch, summed per label) -- the
median [min .. max] of --repeats blocks of --reps calls, the calls of a comparison interleaved block by block, after two warm-ups:

  nh_boxmove   move_rates' batch with a box: the box of half extents (0.3, 0.5, 0.4) under a random rotation, from points just above resting bodies by
               0.75 - 3 units that lean downwards, max_slides 4, BESIDE nh_boxcast on the first casts { origin, 1, displacement, ... }.
  nh_boxwalk   walk_rates' batch with a box: the upright box (0.3, 0.7, 0.3) turned about y by a random angle, one skin above the ground slab beside a
               resting body (half) or above a resting body's top (half), sent 0.5 - 2 units horizontally, snap 0.3, max_slides 4, in four
               CONFIGURATIONS: step height 0 or 1.0, slope limit off or 45 degrees, BESIDE nh_boxcast on the first casts.

Logged with the times: how the records ended, the mean number of casts a record made and THE RATIO the documents quote: the call's time over (mean
casts per record x the box cast's time) -- 1 if a record cost exactly its casts.  258 records of every batch are compared byte for byte with the brute
force over all colliders (tests/hostmover_util.py).

With NUDGE_HIP_LIBRARY naming another build of the library (the parent commit's: tools/build_variant.sh parent "" <rev>), two more worlds on THAT
library answer nh_move, nh_walk, nh_boxcast and nh_capsulecast on the same records, filter off, interleaved with this library's.  Per block: this /
parent, and parent's second world / parent -- the spread the parent shows against itself in this session, inside which this library's ratios must lie.

    [NUDGE_HIP_LIBRARY=.../libparent.so] python tools/boxmove_rates.py [--steps 70] [--reps 10] [--repeats 5] [--out profiles/boxmove_rates.log]
    (on a GPU box; prints the table, one JSON line at the end, and writes both to --out)
"""
import json
import os

import numpy as np

import rates
OTHER = rates.other_library()
from nudge_amd import engine as E           # noqa: E402
from move_rates import move_ends            # noqa: E402

CONFIGS = (("step 0, limit off", 0.0, 0.0), ("step 0, limit 45", 0.0, 45.0), ("step 1.0, limit off", 1.0, 0.0), ("step 1.0, limit 45", 1.0, 45.0))
MOVE_BOX, WALK_BOX = (0.3, 0.5, 0.4), (0.3, 0.7, 0.3)
# what the kernels were compiled for (nh_query.hip): waves per SIMD
OCCUPANCY = dict(boxmove=3, boxwalk=2)


def main():
    ap = rates.parser("boxmove_rates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--max-slides", type=int, default=4)
    ap.add_argument("--no-check", action="store_true", help="skip the brute-force spot checks")
    a = ap.parse_args()
    import torch
    import boxwalk_batches as BWB
    import hostmover_util as MV
    from hostmover_util import BOX as HBM, CAPSULE as HM
    import walk_batches as WB
    from query_util import unit_quats
    land = rates.landed(a)
    others = []
    if OTHER:
        first = rates.landed(a, OTHER, like=land)
        others = [first.world, rates.landed(a, first, like=land).world]
    w, C, n, rec = land.world, land.colliders, a.records, land.records
    up, down, fmt, log = rates.upload, rates.download, rates.fmt, rates.Log()

    def timed(fns):
        return rates.spreads(rates.interleaved_kernels(fns, a.reps, a.repeats))

    pick = rates.spot(n)
    log.say(f"landed {land.name} world: {C:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; GPU {rates.gpu_name(w)}")
    log.say(f"{n:,} records per call, max_slides {a.max_slides}; the library's kernel timers, median of {a.repeats} blocks of {a.reps} calls, interleaved "
            f"(min .. max of the blocks); one box, one run")
    result = dict(colliders=C, steps=a.steps, records=n, max_slides=a.max_slides, occupancy=OCCUPANCY, walk_configs={})

    # ---- nh_boxmove beside nh_boxcast on the first casts: move_rates' batch
    rng = np.random.default_rng(1)
    o, d = rates.move_batch(rng, n, land.positions)
    bm = HBM.moves(o, d, MOVE_BOX, rotations=unit_quats(rng, n), skin=0.01, max_slides=a.max_slides)
    bcasts = HBM.first_casts(bm)
    bmt, bct = up(w, bm), up(w, bcasts)
    r64 = torch.empty((n, 64), dtype=torch.uint8, device=w.dev)
    h32 = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
    t = timed(dict(boxmove=(w, "q_boxmove", lambda: w.boxmove_records(bmt, results=r64)), boxcast=(w, "q_boxcast", lambda: w.boxcast_records(bct, hits=h32))))
    got, first_hits = down(r64, E.MOVE_RESULT), down(h32, E.RAY_HIT)
    checked = 0
    if not a.no_check:
        assert got[pick].tobytes() == HBM.move(rec, w.nbox, bm[pick]).tobytes(), "nh_boxmove differs from the brute force"
        checked = len(pick)
    hist, ends, made = move_ends(got, a.max_slides)
    mean_casts = float(made.mean())
    ratio = t["boxmove"]["ms"] / (mean_casts * t["boxcast"]["ms"])
    log.say(f"nh_boxmove, the box {MOVE_BOX} under random rotations ({OCCUPANCY['boxmove']} waves per SIMD):")
    log.say(f"  nh_boxmove                              {fmt(t['boxmove'])} ms")
    log.say(f"  nh_boxcast, the first casts             {fmt(t['boxcast'])} ms   ({float((first_hits['shape'] != rates.NONE).mean()):.3f} of them hit)")
    log.say(f"  slides histogram (0, 1, 2, ...)         {hist}")
    log.say(f"  ends: {ends}")
    log.say(f"  casts per move, mean                    {mean_casts:.3f}   (most in one move {int(made.max())})")
    log.say(f"  nh_boxmove / (mean casts x boxcast)     {ratio:.2f}")
    log.say(f"  {checked} moves equal the brute force byte for byte")
    result["boxmove"] = dict(boxmove=t["boxmove"], boxcast=t["boxcast"], slides=hist, ends=ends, mean_casts=mean_casts, ratio=ratio, checked_against_brute_force=checked)

    # ---- nh_boxwalk beside nh_boxcast on the first casts: walk_rates' batch
    rng = np.random.default_rng(2)
    x, top, z, d = rates.walk_batch(rng, n, rec, WB._tops(rec, w.nbox))
    base = HBM.walks(BWB.stand(x, top, z, WALK_BOX[1]), d, WALK_BOX, rotations=BWB._yaw(rng, n, 1.0), skin=WB.SKIN, max_slides=a.max_slides, snap_distance=0.3)
    wcasts = HBM.first_casts(HBM.head(base))
    wct = up(w, wcasts)
    r112 = torch.empty((n, 112), dtype=torch.uint8, device=w.dev)
    log.say(f"nh_boxwalk, the upright box {WALK_BOX} turned about y, snap 0.3; half on the slab beside a body, half on a body's top ({OCCUPANCY['boxwalk']} waves per SIMD):")
    for name, step, limit in CONFIGS:
        wk = base.copy()
        wk["step_height"], wk["min_ground_up"] = step, MV.cos_deg(limit)
        wt = up(w, wk)
        t = timed(dict(boxwalk=(w, "q_boxwalk", lambda: w.boxwalk_records(wt, results=r112)), boxcast=(w, "q_boxcast", lambda: w.boxcast_records(wct, hits=h32))))
        got = down(r112, E.WALK_RESULT)
        checked = 0
        if not a.no_check:
            assert got[pick].tobytes() == HBM.walk(rec, w.nbox, wk[pick]).tobytes(), "nh_boxwalk differs from the brute force"
            checked = len(pick)
        s = MV.shares(wk, got)
        s["start_overlap"] = float(((got["flags"] & E.NH_MOVE_START_OVERLAP) != 0).mean())
        mean_casts = float(got["casts"].mean())
        ratio = t["boxwalk"]["ms"] / (mean_casts * t["boxcast"]["ms"])
        log.say(f" {name}:")
        log.say(f"  nh_boxwalk                              {fmt(t['boxwalk'])} ms")
        log.say(f"  nh_boxcast, the first casts             {fmt(t['boxcast'])} ms")
        log.say(f"  shares: {({k: round(v, 4) for k, v in s.items()})}")
        log.say(f"  casts per walk, mean                    {mean_casts:.3f}   (most in one walk {int(got['casts'].max())})")
        log.say(f"  nh_boxwalk / (mean casts x boxcast)     {ratio:.2f}")
        log.say(f"  {checked} walks equal the brute force byte for byte")
        result["walk_configs"][name] = dict(boxwalk=t["boxwalk"], boxcast=t["boxcast"], shares=s, mean_casts=mean_casts, ratio=ratio, checked_against_brute_force=checked)

    # ---- the calls that were there before, beside the other library
    if others:
        # move_rates' and walk_rates' capsule batches on the records drawn above
        cm = HM.moves(bm["origin"], bm["displacement"], 0.5, 0.5, skin=0.01, max_slides=a.max_slides)
        cw = HM.walks(WB.stand(x, top, z, 0.3, 0.4), d, 0.3, 0.4, skin=WB.SKIN, max_slides=a.max_slides, snap_distance=0.3, step_height=1.0)
        calls = (("move", "q_move", cm, 64, lambda wd, t_, r_: wd.move_records(t_, results=r_)),
                 ("walk", "q_walk", cw, 112, lambda wd, t_, r_: wd.walk_records(t_, results=r_)),
                 ("boxcast", "q_boxcast", bcasts, 32, lambda wd, t_, r_: wd.boxcast_records(t_, hits=r_)),
                 ("capsulecast", "q_capsulecast", HM.first_casts(cm), 32, lambda wd, t_, r_: wd.capsulecast_records(t_, hits=r_)))
        log.say(f"filter off, this library beside {os.path.basename(OTHER)} loaded twice (the same bytes from all three); per block this / parent, and parent again / parent:")
        result["beside_other"] = rates.beside_parent(log, dict(this=w, parent=others[0], again=others[1]), calls, n, a.reps, a.repeats)
        for wd in others:
            wd.close()
    else:
        log.say("filter off, this library beside another build: no NUDGE_HIP_LIBRARY given, not measured")
    log.say()
    log.say(json.dumps(result))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
