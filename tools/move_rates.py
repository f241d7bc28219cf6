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
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

NONE = 0xFFFFFFFF


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=70)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--moves", type=int, default=1 << 20)
    ap.add_argument("--max-slides", type=int, default=4)
    ap.add_argument("--no-check", action="store_true", help="skip the brute-force spot check")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "move_rates.log"))
    a = ap.parse_args()
    import torch
    from hostmover_util import CAPSULE as HM
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
    C = len(scene["box_tags"]) + len(scene["sphere_tags"])
    w = E.World(scene, flags=E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP, max_contacts=6 * nb)
    w.step(a.steps)
    w.synchronize()
    w.query_build()
    stream = torch.cuda.current_stream(w.dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, reps):
        ev0.record(stream)
        for _ in range(reps):
            fn()
        ev1.record(stream)
        ev1.synchronize()
        return ev0.elapsed_time(ev1) / reps

    def med(v):
        return dict(ms=float(np.median(v)), min=min(v), max=max(v))

    rng = np.random.default_rng(1)
    n = a.moves
    pos = w.get_bodies()["transforms"]["position"][1:].astype(np.float64)           # the dynamic bodies, landed
    at = rng.integers(0, len(pos), size=n)
    o = pos[at] + np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(2.2, 3.0, n), rng.uniform(-0.5, 0.5, n)], axis=1)      # the capsule's foot 0.2 - 1 above a body's top
    d = rng.normal(size=(n, 3))
    d[:, 1] = -np.abs(d[:, 1]) - 0.5
    d *= rng.uniform(0.75, 3.0, size=(n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    m = HM.moves(o, d, 0.5, 0.5, skin=0.01, max_slides=a.max_slides)
    casts = HM.first_casts(m)
    mt = torch.from_numpy(m.view(np.uint8).copy()).to(w.dev)
    ct = torch.from_numpy(casts.view(np.uint8).copy()).to(w.dev)
    rt = torch.empty((n, 64), dtype=torch.uint8, device=w.dev)
    ht = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
    fns = dict(move=lambda: w.move_records(mt, results=rt), capsulecast=lambda: w.capsulecast_records(ct, hits=ht))
    for fn in fns.values():
        fn(); fn()
    stream.synchronize()
    times = {key: [] for key in fns}
    for _ in range(a.repeats):
        for key, fn in fns.items():
            times[key].append(timed(fn, a.reps))
    t = {key: med(v) for key, v in times.items()}
    got = np.frombuffer(rt.cpu().numpy().tobytes(), dtype=E.MOVE_RESULT)
    first = np.frombuffer(ht.cpu().numpy().tobytes(), dtype=E.RAY_HIT)
    checked = 0
    if not a.no_check:
        import hostquery_util as Q
        rec = Q.records(w.get_bodies()["transforms"], scene)
        pick = np.sort(np.random.default_rng(3).choice(n, size=258, replace=False))
        assert got[pick].tobytes() == HM.move(rec, w.nbox, m[pick]).tobytes(), "the GPU differs from the brute force"
        checked = len(pick)
    fl = got["flags"]
    made = got["slides"] + (((got["last_hit"]["shape"] == NONE) | ((fl & E.NH_MOVE_START_OVERLAP) != 0)) & (fl != E.NH_MOVE_INVALID))
    hist = np.bincount(got["slides"], minlength=a.max_slides + 2)
    ends = {name: int(((fl & bit) != 0).sum()) for name, bit in (("hit", E.NH_MOVE_HIT), ("start_overlap", E.NH_MOVE_START_OVERLAP), ("slides_out", E.NH_MOVE_SLIDES_OUT),
                                                                 ("wedged", E.NH_MOVE_WEDGED))}
    ends["free"] = int((fl == 0).sum())
    mean_casts = float(made.mean())
    ratio = t["move"]["ms"] / (mean_casts * t["capsulecast"]["ms"])
    fmt = lambda v: f"{v['ms']:.3f} ({v['min']:.3f} .. {v['max']:.3f})"                       # noqa: E731
    say(f"landed config-2 world: {C:,} colliders, {nb:,} bodies, after {a.steps} steps; GPU {torch.cuda.get_device_name(w.dev)}")
    say(f"{n:,} moves, max_slides {a.max_slides}; median of {a.repeats} blocks of {a.reps} calls, interleaved (min .. max of the blocks); one box, one run")
    say(f"  nh_move                               {fmt(t['move'])} ms")
    say(f"  nh_capsulecast, the first casts       {fmt(t['capsulecast'])} ms   ({float((first['shape'] != NONE).mean()):.3f} of them hit)")
    say(f"  slides histogram (0, 1, 2, ...)       {[int(x) for x in hist]}")
    say(f"  ends: {ends}")
    say(f"  casts per move, mean                  {mean_casts:.3f}   (most in one move {int(made.max())})")
    say(f"  nh_move / nh_capsulecast              {t['move']['ms'] / t['capsulecast']['ms']:.2f}")
    say(f"  nh_move / (mean casts x capsulecast)  {ratio:.2f}")
    say(f"  {checked} moves equal the brute force byte for byte")
    say()
    say(json.dumps(dict(colliders=C, steps=a.steps, moves=n, max_slides=a.max_slides, move=t["move"], capsulecast=t["capsulecast"], slides=[int(x) for x in hist], ends=ends,
                        mean_casts=mean_casts, ratio=ratio, checked_against_brute_force=checked)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    w.close()


if __name__ == "__main__":
    main()
