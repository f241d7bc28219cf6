"""nh_move rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "nh_move"): 1,048,576 moves of the upright
capsule r = 0.5, hh = 0.5 (skin 0.01, max_slides 4) from points just above resting bodies, by displacements of 0.5 - 2 body sizes (a body is ~1.5 across:
0.75 - 3 units) that lean downwards, and BESIDE it in the same process nh_capsulecast on the same first-cast records { origin, 1, displacement, ... } --
device events, interleaved, the median [min .. max] of --repeats blocks of --reps calls after two warm-ups.  Logged with the times: the histogram of
`slides`, how the moves ended, the mean number of casts a move made (slides + 1 where the last cast missed or started in overlap, else slides), and THE
RATIO the documents quote: the move call's time over (mean casts per move x the capsule cast's time) -- 1 if a move cost exactly its casts; what is above
it is divergence (a lane that has finished waits for the slowest of its wave) and the later casts being short and incoherent.  258 moves are compared
byte for byte with the brute force over all colliders (tests/hostmover_util.py).

    python tools/move_rates.py [--steps 70] [--reps 10] [--repeats 5] [--out profiles/move_rates.log]
    (on a GPU box; prints the table, one JSON line at the end, and writes both to --out)
"""
import json

import numpy as np

import rates
from nudge_amd import engine as E           # noqa: E402

NONE = rates.NONE


def move_ends(got, max_slides):
    """(the slides histogram, how the moves ended, the casts each move made) of nh_MoveResult records."""
    fl = got["flags"]
    made = got["slides"] + (((got["last_hit"]["shape"] == NONE) | ((fl & E.NH_MOVE_START_OVERLAP) != 0)) & (fl != E.NH_MOVE_INVALID))
    hist = [int(x) for x in np.bincount(got["slides"], minlength=max_slides + 2)]
    ends = {name: int(((fl & bit) != 0).sum()) for name, bit in (("hit", E.NH_MOVE_HIT), ("start_overlap", E.NH_MOVE_START_OVERLAP), ("slides_out", E.NH_MOVE_SLIDES_OUT),
                                                                 ("wedged", E.NH_MOVE_WEDGED))}
    ends["free"] = int((fl == 0).sum())
    return hist, ends, made


def main():
    ap = rates.parser("move_rates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--moves", type=int, default=1 << 20)
    ap.add_argument("--max-slides", type=int, default=4)
    ap.add_argument("--no-check", action="store_true", help="skip the brute-force spot check")
    a = ap.parse_args()
    import torch
    from hostmover_util import CAPSULE as HM
    land = rates.landed(a)
    w, C, n = land.world, land.colliders, a.moves
    o, d = rates.move_batch(np.random.default_rng(1), n, land.positions)          # the capsule's foot 0.2 - 1 above a body's top
    m = HM.moves(o, d, 0.5, 0.5, skin=0.01, max_slides=a.max_slides)
    mt, ct = rates.upload(w, m), rates.upload(w, HM.first_casts(m))
    rt = torch.empty((n, 64), dtype=torch.uint8, device=w.dev)
    ht = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
    t = rates.spreads(rates.interleaved(w, dict(move=lambda: w.move_records(mt, results=rt), capsulecast=lambda: w.capsulecast_records(ct, hits=ht)), a.reps, a.repeats))
    got, first = rates.download(rt, E.MOVE_RESULT), rates.download(ht, E.RAY_HIT)
    checked = 0
    if not a.no_check:
        pick = rates.spot(n)
        assert got[pick].tobytes() == HM.move(land.records, w.nbox, m[pick]).tobytes(), "the GPU differs from the brute force"
        checked = len(pick)
    hist, ends, made = move_ends(got, a.max_slides)
    mean_casts = float(made.mean())
    ratio = t["move"]["ms"] / (mean_casts * t["capsulecast"]["ms"])
    log, fmt = rates.Log(), rates.fmt
    log.say(f"landed {land.name} world: {C:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; GPU {rates.gpu_name(w)}")
    log.say(f"{n:,} moves, max_slides {a.max_slides}; median of {a.repeats} blocks of {a.reps} calls, interleaved (min .. max of the blocks); one box, one run")
    log.say(f"  nh_move                               {fmt(t['move'])} ms")
    log.say(f"  nh_capsulecast, the first casts       {fmt(t['capsulecast'])} ms   ({float((first['shape'] != NONE).mean()):.3f} of them hit)")
    log.say(f"  slides histogram (0, 1, 2, ...)       {hist}")
    log.say(f"  ends: {ends}")
    log.say(f"  casts per move, mean                  {mean_casts:.3f}   (most in one move {int(made.max())})")
    log.say(f"  nh_move / nh_capsulecast              {t['move']['ms'] / t['capsulecast']['ms']:.2f}")
    log.say(f"  nh_move / (mean casts x capsulecast)  {ratio:.2f}")
    log.say(f"  {checked} moves equal the brute force byte for byte")
    log.say()
    log.say(json.dumps(dict(colliders=C, steps=a.steps, moves=n, max_slides=a.max_slides, move=t["move"], capsulecast=t["capsulecast"], slides=hist, ends=ends,
                            mean_casts=mean_casts, ratio=ratio, checked_against_brute_force=checked)))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
