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
CONFIGS = (("step 0, limit off", 0.0, 0.0), ("step 0, limit 45", 0.0, 45.0), ("step 1.0, limit off", 1.0, 0.0), ("step 1.0, limit 45", 1.0, 45.0))
MOVE_BOX, WALK_BOX = (0.3, 0.5, 0.4), (0.3, 0.7, 0.3)
# what the kernels were compiled for (nh_query.hip): waves per SIMD
OCCUPANCY = dict(boxmove=3, boxwalk=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=70)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--max-slides", type=int, default=4)
    ap.add_argument("--no-check", action="store_true", help="skip the brute-force spot checks")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boxmove_rates.log"))
    a = ap.parse_args()
    import torch
    import boxwalk_batches as BWB
    import hostmover_util as MV
    from hostmover_util import BOX as HBM, CAPSULE as HM
    import hostquery_util as Q
    import walk_batches as WB
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
    others = []
    if OTHER:
        E._LIB, E._LIB_PATH = None, os.path.abspath(OTHER)
        others = [world(), world()]
        assert others[0].L is not w.L
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def interleaved(fns):
        """fns: {key: (world, timing label, call)}.  Per key the per-call kernel time of each of --repeats blocks of --reps calls, by the world's timers."""
        for wd, _, fn in fns.values():
            fn(); fn()
            wd.synchronize()
        blocks = {key: [] for key in fns}
        for _ in range(a.repeats):
            for key, (wd, label, fn) in fns.items():
                wd.enable_timing(True, only=label)
                wd.kernel_times(reset=True)
                for _ in range(a.reps):
                    fn()
                ms, launches = wd.kernel_times(reset=True)[label]
                wd.enable_timing(False)
                assert launches == a.reps, (label, launches)
                blocks[key].append(ms / launches)
        return blocks

    def med(v):
        return dict(ms=float(np.median(v)), min=float(min(v)), max=float(max(v)))

    def up(x, wd=None):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).to((wd or w).dev)

    def down(t, dtype):
        return np.frombuffer(t.cpu().numpy().tobytes(), dtype=dtype).copy()

    fmt = lambda v: f"{v['ms']:.3f} ({v['min']:.3f} .. {v['max']:.3f})"                       # noqa: E731
    n = a.records
    rec = Q.records(w.get_bodies()["transforms"], scene)
    pick = np.sort(np.random.default_rng(3).choice(n, size=258, replace=False))
    say(f"landed config-2 world: {C:,} colliders, {nb:,} bodies, after {a.steps} steps; GPU {torch.cuda.get_device_name(w.dev)}")
    say(f"{n:,} records per call, max_slides {a.max_slides}; the library's kernel timers, median of {a.repeats} blocks of {a.reps} calls, interleaved "
        f"(min .. max of the blocks); one box, one run")
    result = dict(colliders=C, steps=a.steps, records=n, max_slides=a.max_slides, occupancy=OCCUPANCY, walk_configs={})

    # ---- nh_boxmove beside nh_boxcast on the first casts: move_rates' batch
    rng = np.random.default_rng(1)
    pos = w.get_bodies()["transforms"]["position"][1:].astype(np.float64)           # the dynamic bodies, landed
    at = rng.integers(0, len(pos), size=n)
    o = pos[at] + np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(2.2, 3.0, n), rng.uniform(-0.5, 0.5, n)], axis=1)
    d = rng.normal(size=(n, 3))
    d[:, 1] = -np.abs(d[:, 1]) - 0.5
    d *= rng.uniform(0.75, 3.0, size=(n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    rot = unit_quats(rng, n)
    bm = HBM.moves(o, d, MOVE_BOX, rotations=rot, skin=0.01, max_slides=a.max_slides)
    bcasts = HBM.first_casts(bm)
    bmt, bct = up(bm), up(bcasts)
    r64 = torch.empty((n, 64), dtype=torch.uint8, device=w.dev)
    h32 = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
    t = {k: med(v) for k, v in interleaved(dict(boxmove=(w, "q_boxmove", lambda: w.boxmove_records(bmt, results=r64)),
                                                boxcast=(w, "q_boxcast", lambda: w.boxcast_records(bct, hits=h32)))).items()}
    got, first = down(r64, E.MOVE_RESULT), down(h32, E.RAY_HIT)
    checked = 0
    if not a.no_check:
        assert got[pick].tobytes() == HBM.move(rec, w.nbox, bm[pick]).tobytes(), "nh_boxmove differs from the brute force"
        checked = len(pick)
    fl = got["flags"]
    made = got["slides"] + (((got["last_hit"]["shape"] == NONE) | ((fl & E.NH_MOVE_START_OVERLAP) != 0)) & (fl != E.NH_MOVE_INVALID))
    hist = [int(x) for x in np.bincount(got["slides"], minlength=a.max_slides + 2)]
    ends = {name: int(((fl & bit) != 0).sum()) for name, bit in (("hit", E.NH_MOVE_HIT), ("start_overlap", E.NH_MOVE_START_OVERLAP),
                                                                 ("slides_out", E.NH_MOVE_SLIDES_OUT), ("wedged", E.NH_MOVE_WEDGED))}
    ends["free"] = int((fl == 0).sum())
    mean_casts = float(made.mean())
    ratio = t["boxmove"]["ms"] / (mean_casts * t["boxcast"]["ms"])
    say(f"nh_boxmove, the box {MOVE_BOX} under random rotations ({OCCUPANCY['boxmove']} waves per SIMD):")
    say(f"  nh_boxmove                              {fmt(t['boxmove'])} ms")
    say(f"  nh_boxcast, the first casts             {fmt(t['boxcast'])} ms   ({float((first['shape'] != NONE).mean()):.3f} of them hit)")
    say(f"  slides histogram (0, 1, 2, ...)         {hist}")
    say(f"  ends: {ends}")
    say(f"  casts per move, mean                    {mean_casts:.3f}   (most in one move {int(made.max())})")
    say(f"  nh_boxmove / (mean casts x boxcast)     {ratio:.2f}")
    say(f"  {checked} moves equal the brute force byte for byte")
    result["boxmove"] = dict(boxmove=t["boxmove"], boxcast=t["boxcast"], slides=hist, ends=ends, mean_casts=mean_casts, ratio=ratio, checked_against_brute_force=checked)

    # ---- nh_boxwalk beside nh_boxcast on the first casts: walk_rates' batch
    rng = np.random.default_rng(2)
    tops = WB._tops(rec, w.nbox)
    dyn = np.nonzero(rec["body"] != 0)[0]
    at = rng.choice(dyn, size=n)
    p = rec["p"].astype(np.float64)
    slab_top = float(np.median(tops[rec["body"] == 0]))
    on_slab = rng.random(n) < 0.5
    ang = rng.uniform(0.0, 2 * np.pi, n)
    away = rng.uniform(1.3, 2.2, n)                                        # a body is ~1.5 across: beside it, not in it
    x = np.where(on_slab, p[at, 0] + np.cos(ang) * away, p[at, 0] + rng.uniform(-0.3, 0.3, n))
    z = np.where(on_slab, p[at, 2] + np.sin(ang) * away, p[at, 2] + rng.uniform(-0.3, 0.3, n))
    top = np.where(on_slab, slab_top, tops[at])
    head = np.where(on_slab, ang + np.pi, rng.uniform(0.0, 2 * np.pi, n))
    length = rng.uniform(0.5, 2.0, n)
    d = np.stack([np.cos(head) * length, np.zeros(n), np.sin(head) * length], axis=1)
    base = HBM.walks(BWB.stand(x, top, z, WALK_BOX[1]), d, WALK_BOX, rotations=BWB._yaw(rng, n, 1.0), skin=WB.SKIN, max_slides=a.max_slides, snap_distance=0.3)
    wcasts = HBM.first_casts(HBM.head(base))
    wct = up(wcasts)
    r112 = torch.empty((n, 112), dtype=torch.uint8, device=w.dev)
    say(f"nh_boxwalk, the upright box {WALK_BOX} turned about y, snap 0.3; half on the slab beside a body, half on a body's top ({OCCUPANCY['boxwalk']} waves per SIMD):")
    for name, step, limit in CONFIGS:
        wk = base.copy()
        wk["step_height"], wk["min_ground_up"] = step, MV.cos_deg(limit)
        wt = up(wk)
        t = {k: med(v) for k, v in interleaved(dict(boxwalk=(w, "q_boxwalk", lambda: w.boxwalk_records(wt, results=r112)),
                                                    boxcast=(w, "q_boxcast", lambda: w.boxcast_records(wct, hits=h32)))).items()}
        got = down(r112, E.WALK_RESULT)
        checked = 0
        if not a.no_check:
            assert got[pick].tobytes() == HBM.walk(rec, w.nbox, wk[pick]).tobytes(), "nh_boxwalk differs from the brute force"
            checked = len(pick)
        s = MV.shares(wk, got)
        s["start_overlap"] = float(((got["flags"] & E.NH_MOVE_START_OVERLAP) != 0).mean())
        mean_casts = float(got["casts"].mean())
        ratio = t["boxwalk"]["ms"] / (mean_casts * t["boxcast"]["ms"])
        say(f" {name}:")
        say(f"  nh_boxwalk                              {fmt(t['boxwalk'])} ms")
        say(f"  nh_boxcast, the first casts             {fmt(t['boxcast'])} ms")
        say(f"  shares: {({k: round(v, 4) for k, v in s.items()})}")
        say(f"  casts per walk, mean                    {mean_casts:.3f}   (most in one walk {int(got['casts'].max())})")
        say(f"  nh_boxwalk / (mean casts x boxcast)     {ratio:.2f}")
        say(f"  {checked} walks equal the brute force byte for byte")
        result["walk_configs"][name] = dict(boxwalk=t["boxwalk"], boxcast=t["boxcast"], shares=s, mean_casts=mean_casts, ratio=ratio, checked_against_brute_force=checked)

    # ---- the calls that were there before, beside the other library
    if others:
        # move_rates' and walk_rates' capsule batches on the records drawn above
        cm = HM.moves(bm["origin"], bm["displacement"], 0.5, 0.5, skin=0.01, max_slides=a.max_slides)
        cw = HM.walks(WB.stand(x, top, z, 0.3, 0.4), d, 0.3, 0.4, skin=WB.SKIN, max_slides=a.max_slides, snap_distance=0.3, step_height=1.0)
        cc = HM.first_casts(cm)
        calls = (("move", "q_move", cm, 64, lambda wd, t_, r_: wd.move_records(t_, results=r_)),
                 ("walk", "q_walk", cw, 112, lambda wd, t_, r_: wd.walk_records(t_, results=r_)),
                 ("boxcast", "q_boxcast", bcasts, 32, lambda wd, t_, r_: wd.boxcast_records(t_, hits=r_)),
                 ("capsulecast", "q_capsulecast", cc, 32, lambda wd, t_, r_: wd.capsulecast_records(t_, hits=r_)))
        say(f"filter off, this library beside {os.path.basename(OTHER)} loaded twice (the same bytes from all three); per block this / parent, and parent again / parent:")
        result["beside_other"] = {}
        for name, label, records, size, call in calls:
            worlds = dict(this=w, parent=others[0], again=others[1])
            ins = {k: up(records, wd) for k, wd in worlds.items()}
            outs = {k: torch.empty((n, size), dtype=torch.uint8, device=w.dev) for k in worlds}
            blocks = interleaved({k: (wd, label, (lambda k=k, wd=wd: call(wd, ins[k], outs[k]))) for k, wd in worlds.items()})
            assert torch.equal(outs["this"], outs["parent"]) and torch.equal(outs["again"], outs["parent"]), f"nh_{name}: the libraries differ"
            this, parent, again = (np.array(blocks[k]) for k in ("this", "parent", "again"))
            r_this, r_self = this / parent, again / parent
            inside = bool(r_self.min() <= np.median(r_this) <= r_self.max())
            say(f"  nh_{name:<12} this {fmt(med(this))} ms   parent {fmt(med(parent))} ms   this / parent {np.median(r_this):.3f} ({r_this.min():.3f} .. {r_this.max():.3f})"
                f"   parent / parent {np.median(r_self):.3f} ({r_self.min():.3f} .. {r_self.max():.3f})   {'inside' if inside else 'OUTSIDE'} the parent's own spread")
            result["beside_other"][name] = dict(this=med(this), parent=med(parent), again=med(again), this_over_parent=med(r_this), parent_over_parent=med(r_self),
                                                inside=inside)
        for wd in others:
            wd.close()
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
