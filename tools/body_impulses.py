"""nh_impulse_sums / nh_body_impulses / nh_blast_impulses rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h,
"body impulses").  ms per call as the best of --reps blocks of --inner calls after a warm-up, by device events around the block (rates.blocks):

    the steady step            nh_step(1) before and after the series: the new code is in no step path, so both are the parent's figure
    nh_impulse_sums            one record per body in body order, and four records per body in shuffled order (runs of one record: the sort's worst case)
    nh_body_impulses           the same two lists with ZERO impulses, with and without NH_IMPULSE_WAKE's store -- the work does not depend on the values,
                               and the world stays at rest for the lines behind it (the woken world is put back to sleep by stepping it)
    a blast chain              one sphere over a tile: nh_overlap_wide, nh_overlap_bodies, nh_blast_impulses, nh_impulse_sums
    nh_contact_pairs           on the same world's exported views, for scale

Then one more call of each with nh_enable_timing for the per-label breakdown, and the sums against the host oracle byte for byte.

    python tools/body_impulses.py [--steps 70] [--reps 5] [--inner 10] [--out profiles/body_impulses.log]
    (on a GPU box; prints the table, one JSON line at the end, and writes both to --out)
"""
import json

import numpy as np

import rates


def main():
    ap = rates.parser("body_impulses")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    import torch
    import hostimpulse_util as HI
    from nudge_amd import engine as E
    land = rates.landed(a, build=True)
    w, nb, log = land.world, land.bodies, rates.Log()
    res = {}

    def row(name, fn, with_labels=True):
        best, median = rates.best_median(rates.blocks(w, fn, a.reps, a.inner))
        res[name] = dict(ms=best, median_ms=median)
        log.say(f"  {name:86s} {best:9.3f} {median:9.3f}")
        if with_labels:
            res[name]["labels"] = rates.labels(w, fn)
            log.say(f"      labels, ms: {res[name]['labels']}")
        return best

    c0 = w.counts()
    log.say(f"landed {land.name} world: {nb:,} bodies, {c0['contacts']:,} contacts after {a.steps} steps; GPU {rates.gpu_name(w)}")
    log.say(f"ms per call: the best of {a.reps} blocks of {a.inner} calls after a warm-up, device events around the block; one box, one run")
    log.say(f"  {'':86s} {'ms':>9s} {'median':>9s}")
    row("nh_step(1) before the series", lambda: w.step(1), with_labels=False)
    res["still_steps_before"] = w.counts()["still_steps"] - c0["still_steps"]

    rng = np.random.default_rng(7)
    transforms = w.get_bodies()["transforms"]
    body = np.arange(1, nb, dtype=np.uint32)
    lists = {"one record per body, body order": body, "four records per body, shuffled": rng.permutation(np.repeat(body, 4))}
    for name, bodies in lists.items():
        n = len(bodies)
        lst = HI.records(bodies, rng.normal(size=(n, 3)).astype(np.float32), point=transforms["position"][bodies] + rng.normal(size=(n, 3)).astype(np.float32))
        dl = rates.upload(w, lst)
        out = (torch.zeros(1, dtype=torch.int32, device=w.dev), torch.empty((nb, 32), dtype=torch.uint8, device=w.dev), nb)
        row(f"nh_impulse_sums, {name} ({n:,} records)", lambda: w.impulse_sums_records(dl, capacity=n, out=out))
        total, want = HI.sums(transforms, lst)
        got = rates.download(out[1].reshape(-1)[:32 * total], E.IMPULSE_SUM)
        assert int(out[0].item()) == total == nb - 1 and got.tobytes() == want[:total].tobytes(), "the GPU's sums differ from the host oracle's"
        log.say("      the sums equal the host oracle byte for byte")
        res[f"checked {name}"] = total
        lst["impulse"] = 0.0
        dz = rates.upload(w, lst)
        row(f"nh_body_impulses, {name}, zero impulses", lambda: w.body_impulses_records(dz, capacity=n))
        if n == nb - 1:
            row(f"nh_body_impulses, {name}, zero impulses, NH_IMPULSE_WAKE", lambda: w.body_impulses_records(dz, capacity=n, wake=True), with_labels=False)

    # a blast: one sphere of half a tile's size on the middle of tile 0
    pos = transforms["position"].astype(np.float64)
    size = rates.tile_size(land.scene, pos)
    centre = pos[np.nonzero(np.asarray(land.scene["tile_of_body"]) == 0)[0]].mean(axis=0)
    qt = rates.upload(w, rates.overlap_queries(centre[None], (size / 2, 0.0, 0.0), E.NH_SHAPE_SPHERE))
    blast = np.zeros(1, dtype=E.BLAST)
    blast["centre"], blast["radius"], blast["strength"], blast["falloff"] = centre, size / 2, 5.0, 1.0
    bt = rates.upload(w, blast)
    ot, _ = w.overlap_wide_records(qt)
    cap = rates.total_of(ot)
    ht, hb = (torch.empty((max(cap, 1), 16), dtype=torch.uint8, device=w.dev) for _ in range(2))
    ob = torch.empty(2, dtype=torch.int32, device=w.dev)
    rec = torch.empty((max(cap, 1), 32), dtype=torch.uint8, device=w.dev)
    sums = (torch.zeros(1, dtype=torch.int32, device=w.dev), torch.empty((max(cap, 1), 32), dtype=torch.uint8, device=w.dev), cap)

    def chain():
        w.overlap_wide_records(qt, offsets=ot, hits=ht, capacity=cap)
        w.overlap_bodies_records(1, (ot, ht, cap), offsets=ob, hits=hb, capacity=cap)
        w.blast_impulses_records(bt, 1, (ob, hb, cap), out=rec)
        w.impulse_sums_records(rec, count=ob[1:], capacity=cap, out=sums)

    row(f"blast chain: overlap_wide, overlap_bodies, blast_impulses, impulse_sums ({cap:,} colliders in the sphere)", chain)
    res["blast_bodies_pushed"] = int(sums[0].item())
    log.say(f"      {res['blast_bodies_pushed']:,} bodies pushed")

    w.export_views(E.NH_VIEW_CONTACTS | E.NH_VIEW_CACHE)
    K = w.counts()["contacts"]
    count_word = torch.tensor([K], dtype=torch.int32, device=w.dev)
    pairs = (torch.zeros(1, dtype=torch.int32, device=w.dev), torch.empty((max(K, 1), 64), dtype=torch.uint8, device=w.dev), K)
    row("nh_contact_pairs on the exported views, for scale", lambda: w.contact_pairs_records(w._keep["cd"], w._keep["cb"], w._keep["kd"], count=count_word,
                                                                                             capacity=w.max_contacts, body_count=nb, out=pairs))
    c1 = w.counts()
    w.step(4)          # (NH_IMPULSE_WAKE invalidated the sleep prediction and the speculation: a few steps bring both back)
    row("nh_step(1) after the series", lambda: w.step(1), with_labels=False)
    res["still_steps_after"] = w.counts()["still_steps"] - c1["still_steps"]
    log.say(f"      still steps among the steps timed: {res['still_steps_before']} before, {res['still_steps_after']} after (4 untimed steps in between)")

    log.say()
    log.say(json.dumps(dict(bodies=nb, contacts=c0["contacts"], steps=a.steps, **res)))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
