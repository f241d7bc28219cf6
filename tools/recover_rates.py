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
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OTHER = os.environ.pop("NUDGE_HIP_LIBRARY", None)          # (engine reads it on import: this process loads the tree's library first)
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

NONE = 0xFFFFFFFF
SHAPES = ("sphere", "capsule", "box")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=70)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--max-iterations", type=int, default=4)
    ap.add_argument("--no-check", action="store_true", help="skip the brute-force spot check")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recover_rates.log"))
    a = ap.parse_args()
    import torch
    from hostmover_util import CAPSULE as HM
    import hostrecover_util as HR
    from query_util import unit_quats
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
    C = len(scene["box_tags"]) + len(scene["sphere_tags"])

    def world():
        w = E.World(scene, flags=E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP, max_contacts=6 * nb)
        w.step(a.steps)
        w.synchronize()
        w.query_build()
        return w

    w = world()
    other = None
    if OTHER:
        E._LIB, E._LIB_PATH = None, os.path.abspath(OTHER)
        other = world()
        assert other.L is not w.L
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

    def interleaved(fns):
        for fn in fns.values():                                # warm-up: scratch grows here, not in a timed call
            fn(); fn()
        stream.synchronize()
        times = {key: [] for key in fns}
        for _ in range(a.repeats):
            for key, fn in fns.items():
                times[key].append(timed(fn, a.reps))
        return {key: med(v) for key, v in times.items()}

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).to(w.dev)

    fmt = lambda v: f"{v['min']:.3f} best, {v['ms']:.3f} ({v['min']:.3f} .. {v['max']:.3f})"       # noqa: E731
    rng = np.random.default_rng(1)
    n = a.queries
    pos = w.get_bodies()["transforms"]["position"][1:].astype(np.float64)           # the dynamic bodies, landed
    at = rng.integers(0, len(pos), size=n)
    # a body is ~1.5 across: the shape's centre 0.3 - 1.2 above a body's centre, so its lowest point is in the body for most
    c = pos[at] + np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(0.3, 1.2, n), rng.uniform(-0.5, 0.5, n)], axis=1)
    batches = dict(sphere=HR.recovers(c, radii=0.5, skin=0.01, max_iterations=a.max_iterations),
                   capsule=HR.recovers(c, radii=0.5, half_heights=0.5, skin=0.01, max_iterations=a.max_iterations),
                   box=HR.recovers(c, half_extents=(0.5, 0.5, 0.5), rotations=unit_quats(rng, n), skin=0.01, max_iterations=a.max_iterations))
    say(f"landed config-2 world: {C:,} colliders, {nb:,} bodies, after {a.steps} steps; GPU {torch.cuda.get_device_name(w.dev)}")
    say(f"{n:,} queries per shape, skin 0.01, max_iterations {a.max_iterations}; ms per call by device events: the best, and the median (min .. max), of {a.repeats} "
        f"blocks of {a.reps} calls, interleaved; one box, one run")
    rec = None
    result = dict(colliders=C, steps=a.steps, queries=n, max_iterations=a.max_iterations, shapes={})
    for shape in SHAPES:
        m = batches[shape]
        mt, qt = up(m), up(HR.queries(m))
        rt = torch.empty((n, 64), dtype=torch.uint8, device=w.dev)
        ot = torch.empty(n + 1, dtype=torch.int32, device=w.dev)
        w.penetration_records(qt, offsets=ot)
        total = int(ot[n].item()) & NONE
        assert 0 < total < NONE
        ht = torch.empty((total, 32), dtype=torch.uint8, device=w.dev)

        def pen():
            w.penetration_records(qt, offsets=ot)
            w.penetration_records(qt, offsets=ot, hits=ht, capacity=total)

        t = interleaved(dict(recover=lambda: w.recover_records(mt, results=rt), overlap=lambda: w.overlap_records(qt, offsets=ot), penetration=pen))
        got = np.frombuffer(rt.cpu().numpy().tobytes(), dtype=E.RECOVER_RESULT)
        checked = 0
        if not a.no_check:
            import hostquery_util as Q
            rec = Q.records(w.get_bodies()["transforms"], scene) if rec is None else rec
            pick = np.sort(np.random.default_rng(3).choice(n, size=258, replace=False))
            assert got[pick].tobytes() == HR.recover(rec, w.nbox, m[pick]).tobytes(), "the GPU differs from the brute force"
            checked = len(pick)
        fl = got["flags"]
        hist = [int(x) for x in np.bincount(got["iterations"], minlength=a.max_iterations + 1)]
        ends = dict(free_at_once=int((fl == 0).sum()), freed=int((fl == E.NH_RECOVER_PUSHED).sum()), overlapping=int(((fl & E.NH_RECOVER_OVERLAPPING) != 0).sum()),
                    touching=int(((fl & E.NH_RECOVER_TOUCHING) != 0).sum()))
        walks = float((got["iterations"] + 1).mean())
        r_pen = t["recover"]["min"] / t["penetration"]["min"]
        r_walks = t["recover"]["min"] / (walks * t["overlap"]["min"])
        say(f"{shape}:")
        say(f"  nh_recover                                  {fmt(t['recover'])} ms")
        say(f"  nh_overlap, count only                      {fmt(t['overlap'])} ms")
        say(f"  nh_penetration, count + list                {fmt(t['penetration'])} ms   ({total:,} records)")
        say(f"  iterations histogram (0, 1, 2, ...)         {hist}")
        say(f"  ends: {ends}")
        say(f"  walks per query, mean                       {walks:.3f}")
        say(f"  nh_recover / nh_penetration (count + list)  {r_pen:.2f}   (best over best)")
        say(f"  nh_recover / (mean walks x nh_overlap)      {r_walks:.2f}")
        say(f"  {checked} records equal the brute force byte for byte")
        result["shapes"][shape] = dict(recover=t["recover"], overlap=t["overlap"], penetration=t["penetration"], records=total, iterations=hist, ends=ends,
                                       mean_walks=walks, ratio_to_penetration=r_pen, ratio_to_walks=r_walks, checked_against_brute_force=checked)
    if other is not None:
        q = HR.queries(batches["sphere"])
        d = rng.normal(size=(n, 3))
        d *= rng.uniform(1.0, 2.0, size=(n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
        moves = HM.moves(c + (0.0, 1.0, 0.0), d, 0.5, 0.5, skin=0.01, max_slides=4)
        qt, mvt = up(q), up(moves)
        ot = {k: torch.empty(n + 1, dtype=torch.int32, device=w.dev) for k in ("this", "other")}
        rt = {k: torch.empty((n, 64), dtype=torch.uint8, device=w.dev) for k in ("this", "other")}
        t = interleaved({"overlap this": lambda: w.overlap_records(qt, offsets=ot["this"]), "overlap other": lambda: other.overlap_records(qt, offsets=ot["other"]),
                         "move this": lambda: w.move_records(mvt, results=rt["this"]), "move other": lambda: other.move_records(mvt, results=rt["other"])})
        assert torch.equal(ot["this"], ot["other"]) and torch.equal(rt["this"], rt["other"]), "the two libraries differ"
        say(f"filter off, this library beside {os.path.basename(OTHER)} (the same bytes from both):")
        for call in ("overlap", "move"):
            ratio = t[call + " this"]["ms"] / t[call + " other"]["ms"]
            say(f"  nh_{call:<8} this {fmt(t[call + ' this'])} ms   other {fmt(t[call + ' other'])} ms   this / other {ratio:.3f} (medians)")
            result[call + "_beside_other"] = dict(this=t[call + " this"], other=t[call + " other"], ratio=ratio)
        other.close()
    else:
        say("filter off, this library beside another build: no NUDGE_HIP_LIBRARY given, not measured")
    say()
    say(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    w.close()


if __name__ == "__main__":
    main()
