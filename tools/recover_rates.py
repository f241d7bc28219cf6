"""nh_recover rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "nh_recover"): 1,048,576 spheres (r = 0.5),
upright capsules (r = 0.5, hh = 0.5) and boxes (half extents 0.5, random rotations), skin 0.01, max_iterations 4, placed so that most start sunk into the
top of a resting body, and BESIDE each in the same process, for the same first 48 bytes, nh_overlap count-only and nh_penetration's count call + list call
(the capacity is the total, read once before the timing) -- device events, interleaved, per call the best and the median [min .. max] of --repeats blocks
of --reps calls after two warm-ups.  Logged with the times: the histogram of `iterations`, how the recovers ended, the mean number of walks a recover made
(iterations + 1), and THE RATIOS the documents quote: the recover call's time over nh_penetration's count + list (what one round of the host loop costs on
the device alone, before its download and upload), and over (mean walks x the nh_overlap count walk).  258 records per shape are compared byte for byte
with the brute force over all colliders (tests/hostrecover_util.py).

With NUDGE_HIP_LIBRARY naming another build of the library (the parent commit's: tools/build_variant.sh parent "" <rev>), a second world on THAT library
is stepped and built in the same process, and the filter-off times of nh_overlap (count-only, the sphere queries) and nh_move (the capsules moved by 1 - 2
units) of the two libraries are logged side by side: the new kernels are added beside the old ones, not into them.

    [NUDGE_HIP_LIBRARY=.../libparent.so] python tools/recover_rates.py [--steps 70] [--reps 10] [--repeats 5] [--out profiles/recover_rates.log]
    (on a GPU box; prints the table, one JSON line at the end, and writes both to --out)
"""
import json
import os

import numpy as np

import rates
OTHER = rates.other_library()
from nudge_amd import engine as E           # noqa: E402

SHAPES = ("sphere", "capsule", "box")


def main():
    ap = rates.parser("recover_rates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--max-iterations", type=int, default=4)
    ap.add_argument("--no-check", action="store_true", help="skip the brute-force spot check")
    a = ap.parse_args()
    import torch
    from hostmover_util import CAPSULE as HM
    import hostrecover_util as HR
    from query_util import unit_quats
    land = rates.landed(a)
    other = rates.landed(a, OTHER, like=land).world if OTHER else None
    w, C, n, pos = land.world, land.colliders, a.queries, land.positions

    def interleaved(fns):
        return rates.spreads(rates.interleaved(w, fns, a.reps, a.repeats))

    log, fmt = rates.Log(), rates.fmt_best
    rng = np.random.default_rng(1)
    at = rng.integers(0, len(pos), size=n)
    # a body is ~1.5 across: the shape's centre 0.3 - 1.2 above a body's centre, so its lowest point is in the body for most
    c = pos[at] + np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(0.3, 1.2, n), rng.uniform(-0.5, 0.5, n)], axis=1)
    batches = dict(sphere=HR.recovers(c, radii=0.5, skin=0.01, max_iterations=a.max_iterations),
                   capsule=HR.recovers(c, radii=0.5, half_heights=0.5, skin=0.01, max_iterations=a.max_iterations),
                   box=HR.recovers(c, half_extents=(0.5, 0.5, 0.5), rotations=unit_quats(rng, n), skin=0.01, max_iterations=a.max_iterations))
    log.say(f"landed {land.name} world: {C:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; GPU {rates.gpu_name(w)}")
    log.say(f"{n:,} queries per shape, skin 0.01, max_iterations {a.max_iterations}; ms per call by device events: the best, and the median (min .. max), of {a.repeats} "
            f"blocks of {a.reps} calls, interleaved; one box, one run")
    result = dict(colliders=C, steps=a.steps, queries=n, max_iterations=a.max_iterations, shapes={})
    for shape in SHAPES:
        m = batches[shape]
        mt, qt = rates.upload(w, m), rates.upload(w, HR.queries(m))
        rt = torch.empty((n, 64), dtype=torch.uint8, device=w.dev)
        ot = torch.empty(n + 1, dtype=torch.int32, device=w.dev)
        w.penetration_records(qt, offsets=ot)
        total = rates.total_of(ot)
        assert 0 < total < rates.NONE
        ht = torch.empty((total, 32), dtype=torch.uint8, device=w.dev)

        def pen():
            w.penetration_records(qt, offsets=ot)
            w.penetration_records(qt, offsets=ot, hits=ht, capacity=total)

        t = interleaved(dict(recover=lambda: w.recover_records(mt, results=rt), overlap=lambda: w.overlap_records(qt, offsets=ot), penetration=pen))
        got = rates.download(rt, E.RECOVER_RESULT)
        checked = 0
        if not a.no_check:
            pick = rates.spot(n)
            assert got[pick].tobytes() == HR.recover(land.records, w.nbox, m[pick]).tobytes(), "the GPU differs from the brute force"
            checked = len(pick)
        fl = got["flags"]
        hist = [int(x) for x in np.bincount(got["iterations"], minlength=a.max_iterations + 1)]
        ends = dict(free_at_once=int((fl == 0).sum()), freed=int((fl == E.NH_RECOVER_PUSHED).sum()), overlapping=int(((fl & E.NH_RECOVER_OVERLAPPING) != 0).sum()),
                    touching=int(((fl & E.NH_RECOVER_TOUCHING) != 0).sum()))
        walks = float((got["iterations"] + 1).mean())
        r_pen = t["recover"]["min"] / t["penetration"]["min"]
        r_walks = t["recover"]["min"] / (walks * t["overlap"]["min"])
        log.say(f"{shape}:")
        log.say(f"  nh_recover                                  {fmt(t['recover'])} ms")
        log.say(f"  nh_overlap, count only                      {fmt(t['overlap'])} ms")
        log.say(f"  nh_penetration, count + list                {fmt(t['penetration'])} ms   ({total:,} records)")
        log.say(f"  iterations histogram (0, 1, 2, ...)         {hist}")
        log.say(f"  ends: {ends}")
        log.say(f"  walks per query, mean                       {walks:.3f}")
        log.say(f"  nh_recover / nh_penetration (count + list)  {r_pen:.2f}   (best over best)")
        log.say(f"  nh_recover / (mean walks x nh_overlap)      {r_walks:.2f}")
        log.say(f"  {checked} records equal the brute force byte for byte")
        result["shapes"][shape] = dict(recover=t["recover"], overlap=t["overlap"], penetration=t["penetration"], records=total, iterations=hist, ends=ends,
                                       mean_walks=walks, ratio_to_penetration=r_pen, ratio_to_walks=r_walks, checked_against_brute_force=checked)
    if other is not None:
        q = HR.queries(batches["sphere"])
        d = rng.normal(size=(n, 3))
        d *= rng.uniform(1.0, 2.0, size=(n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
        moves = HM.moves(c + (0.0, 1.0, 0.0), d, 0.5, 0.5, skin=0.01, max_slides=4)
        qt, mvt = rates.upload(w, q), rates.upload(w, moves)
        ot = {k: torch.empty(n + 1, dtype=torch.int32, device=w.dev) for k in ("this", "other")}
        rt = {k: torch.empty((n, 64), dtype=torch.uint8, device=w.dev) for k in ("this", "other")}
        t = interleaved({"overlap this": lambda: w.overlap_records(qt, offsets=ot["this"]), "overlap other": lambda: other.overlap_records(qt, offsets=ot["other"]),
                         "move this": lambda: w.move_records(mvt, results=rt["this"]), "move other": lambda: other.move_records(mvt, results=rt["other"])})
        assert torch.equal(ot["this"], ot["other"]) and torch.equal(rt["this"], rt["other"]), "the two libraries differ"
        log.say(f"filter off, this library beside {os.path.basename(OTHER)} (the same bytes from both):")
        for call in ("overlap", "move"):
            ratio = t[call + " this"]["ms"] / t[call + " other"]["ms"]
            log.say(f"  nh_{call:<8} this {fmt(t[call + ' this'])} ms   other {fmt(t[call + ' other'])} ms   this / other {ratio:.3f} (medians)")
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
