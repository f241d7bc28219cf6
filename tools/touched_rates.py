"""nh_move_touched, nh_boxmove_touched, nh_walk_touched and nh_boxwalk_touched beside their plain movers on the landed config-2 world (1,004,400 boxes +
124 ground slabs; include/nudge_hip.h, "nh_move_touched"), 2^20 records each, timed by the LIBRARY'S KERNEL TIMERS (nh_enable_timing / nh_kernel_times:
device events around each launch, summed per label) -- the median [min .. max] of --repeats blocks of --reps calls, the calls of a comparison interleaved
block by block, after two warm-ups.  The workloads are those of tools/move_rates.py, tools/walk_rates.py and tools/boxmove_rates.py:

  move      the capsule r = hh = 0.5 under a random rotation, from points just above resting bodies by 0.75 - 3 units that lean downwards, max_slides 4
  boxmove   the same origins and displacements with the box of half extents (0.3, 0.5, 0.4)
  walk      the upright capsule r = 0.3, hh = 0.4 one skin above the ground slab beside a resting body (half) or above a resting body's top (half), sent
            0.5 - 2 units horizontally, snap 0.3, step height 1.0, slope limit off, max_slides 4
  boxwalk   the same with the upright box (0.3, 0.7, 0.3) turned about y by a random angle

Per mover: the plain call, the touched call at k = 4 and at k = the maximum (9 for a move, 21 for a walk), each touched time over the plain one per
block, and the mean touches per record.  258 records of every touched batch are compared byte for byte with the brute force over all colliders
(tests/hosttouch_util.py), and every touched call's results with the plain call's.

With NUDGE_HIP_LIBRARY naming another build of the library (the parent commit's: tools/build_variant.sh parent "" <rev>), two more worlds on THAT
library answer the four plain movers on the same records, filter off, interleaved with this library's.  Per block: this / parent, and parent's second
world / parent -- the spread the parent shows against itself in this session, inside which this library's ratios must lie (the plain instantiations
are unchanged).

    [NUDGE_HIP_LIBRARY=.../libparent.so] python tools/touched_rates.py [--steps 70] [--reps 10] [--repeats 7] [--out profiles/touched_rates.log]
    (on a GPU box; prints the table, one JSON line at the end, and writes both to --out)
"""
import json
import os

import numpy as np

import rates
OTHER = rates.other_library()
from nudge_amd import engine as E           # noqa: E402

MOVE_BOX, WALK_BOX = (0.3, 0.5, 0.4), (0.3, 0.7, 0.3)
# what the kernels were compiled for (nh_query.hip): waves per SIMD, plain and touched
OCCUPANCY = dict(move=(4, 4), boxmove=(3, 3), walk=(3, 2), boxwalk=(2, 2))
K_SMALL = 4


def main():
    ap = rates.parser("touched_rates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--max-slides", type=int, default=4)
    ap.add_argument("--no-check", action="store_true", help="skip the brute-force spot checks")
    a = ap.parse_args()
    import torch
    import boxwalk_batches as BWB
    import hosttouch_util as HT
    import walk_batches as WB
    from hostmover_util import BOX as HBM, CAPSULE as HM
    from query_util import unit_quats
    land = rates.landed(a)
    others = []
    if OTHER:
        first = rates.landed(a, OTHER, like=land)
        others = [first.world, rates.landed(a, first, like=land).world]
    w, colliders, n, rec = land.world, land.colliders, a.records, land.records
    med, fmt, log = rates.spread, rates.fmt, rates.Log()
    pick = rates.spot(n)
    log.say(f"landed {land.name} world: {colliders:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; GPU {rates.gpu_name(w)}")
    log.say(f"{n:,} records per call, max_slides {a.max_slides}; the library's kernel timers, median of {a.repeats} blocks of {a.reps} calls, interleaved "
            f"(min .. max of the blocks); one box, one run")

    # ---- the records: move_rates' and boxmove_rates' moves, walk_rates' and boxmove_rates' walks
    rng = np.random.default_rng(1)
    o, d = rates.move_batch(rng, n, land.positions)
    rot = unit_quats(rng, n)
    records = dict(move=HM.moves(o, d, 0.5, 0.5, rotations=rot, skin=0.01, max_slides=a.max_slides),
                   boxmove=HBM.moves(o, d, MOVE_BOX, rotations=rot, skin=0.01, max_slides=a.max_slides))
    rng = np.random.default_rng(2)
    x, top, z, d = rates.walk_batch(rng, n, rec, WB._tops(rec, w.nbox))
    records["walk"] = HM.walks(WB.stand(x, top, z, 0.3, 0.4), d, 0.3, 0.4, skin=WB.SKIN, max_slides=a.max_slides, snap_distance=0.3, step_height=1.0)
    records["boxwalk"] = HBM.walks(BWB.stand(x, top, z, WALK_BOX[1]), d, WALK_BOX, rotations=BWB._yaw(rng, n, 1.0), skin=WB.SKIN, max_slides=a.max_slides,
                                   snap_distance=0.3, step_height=1.0)
    movers = (("move", HT.CAPSULE, "move", 64, E.MOVE_RESULT, HT.MOVE_K), ("boxmove", HT.BOX, "move", 64, E.MOVE_RESULT, HT.MOVE_K),
              ("walk", HT.CAPSULE, "walk", 112, E.WALK_RESULT, HT.WALK_K), ("boxwalk", HT.BOX, "walk", 112, E.WALK_RESULT, HT.WALK_K))
    result = dict(colliders=colliders, steps=a.steps, records=n, max_slides=a.max_slides, occupancy=OCCUPANCY, k_small=K_SMALL, movers={})

    # ---- each mover: plain, touched at k = 4, touched at k = the maximum
    cn = torch.empty(n, dtype=torch.int32, device=w.dev)
    for name, T, kind, size, dtype, k_max in movers:
        rt = rates.upload(w, records[name])
        plain_out = torch.empty((n, size), dtype=torch.uint8, device=w.dev)
        outs = {k: torch.empty((n, size), dtype=torch.uint8, device=w.dev) for k in (K_SMALL, k_max)}
        tch = {k: torch.empty((n, k, 64), dtype=torch.uint8, device=w.dev) for k in (K_SMALL, k_max)}
        plain_call, touched_call = getattr(w, name + "_records"), getattr(w, name + "_touched_records")
        fns = dict(plain=(w, "q_" + name, lambda: plain_call(rt, results=plain_out)))
        for k in (K_SMALL, k_max):
            fns[k] = (w, f"q_{name}_touched", lambda k=k: touched_call(rt, k, results=outs[k], counts=cn, touches=tch[k]))
        blocks = rates.interleaved_kernels(fns, a.reps, a.repeats)
        w.synchronize()
        assert torch.equal(outs[K_SMALL], plain_out) and torch.equal(outs[k_max], plain_out), f"nh_{name}_touched: results differ from nh_{name}'s"
        counts = cn.cpu().numpy().view(np.uint32)
        checked = 0
        if not a.no_check:
            ref, ref_counts, ref_touches = getattr(T, kind)(rec, w.nbox, records[name][pick])
            got_touches = rates.download(tch[k_max][torch.from_numpy(pick).to(w.dev)], E.TOUCH).reshape(len(pick), k_max)
            assert rates.download(outs[k_max], dtype)[pick].tobytes() == ref.tobytes(), f"nh_{name}_touched differs from the brute force"
            HT.same_touches(got_touches, counts[pick], ref_touches, ref_counts, name)
            checked = len(pick)
        hist = [int(v) for v in np.bincount(counts, minlength=2)]
        t = rates.spreads(blocks)
        ratios = {k: med(blocks[k] / blocks["plain"]) for k in (K_SMALL, k_max)}
        mean = float(counts.mean())
        cut = float((counts > K_SMALL).mean())
        plain_waves, touched_waves = OCCUPANCY[name]
        log.say(f"nh_{name} ({plain_waves} waves per SIMD) and nh_{name}_touched ({touched_waves}):")
        log.say(f"  nh_{name:<34} {fmt(t['plain'])} ms")
        for k in (K_SMALL, k_max):
            log.say(f"  {'nh_%s_touched, k = %d' % (name, k):<37} {fmt(t[k])} ms   touched / plain per block {fmt(ratios[k])}")
        log.say(f"  touches per record, mean               {mean:.3f}   (histogram 0, 1, 2, ...: {hist}; {cut:.4f} of the records have more than {K_SMALL})")
        log.say(f"  bytes of touches and counts written    {(64 * np.minimum(counts, k_max).sum() + 4 * n) / 1e6:.1f} MB at k = {k_max} beside {size * n / 1e6:.1f} MB of results")
        log.say(f"  {checked} records equal the brute force byte for byte; all results equal nh_{name}'s")
        result["movers"][name] = dict(plain=t["plain"], touched={str(k): t[k] for k in (K_SMALL, k_max)}, ratio={str(k): ratios[k] for k in (K_SMALL, k_max)},
                                      mean_touches=mean, touches=hist, more_than_k_small=cut, checked_against_brute_force=checked)
        del rt, plain_out, outs, tch

    # ---- the plain movers beside the other library
    if others:
        log.say(f"filter off, this library beside {os.path.basename(OTHER)} loaded twice (the same bytes from all three); per block this / parent, and parent again / parent:")
        calls = [(name, "q_" + name, records[name], size, (lambda wd, t_, r_, name=name: getattr(wd, name + "_records")(t_, results=r_))) for name, _, _, size, _, _ in movers]
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
