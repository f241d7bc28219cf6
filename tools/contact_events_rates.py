"""nh_contact_pairs / nh_step_contact_pairs / nh_contact_events rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs, about 4 M
contacts and 1 M body pairs; include/nudge_hip.h, "contact events").  ms per call as the best of --reps blocks of --inner calls after a warm-up, by
device events around the block:

    the steady step                      nh_step(1), still steps and -- option no_still -- full steps: the price of a call in steps
    nh_contact_pairs                     on the exported views, the cache's impulses as the contacts' (in the landed world entry i is contact i's)
    nh_step_contact_pairs                with the views current (no export), and as the DIFFERENCE of blocks of step + call and blocks of steps alone:
                                         after a still step the call pays the view export as well, after a full step it does not
    nh_contact_events                    on the lists of two consecutive steps
    nh_overlap_bodies                    on a list of as many records as there are pairs' runs to sort here: the nearest existing sort-and-compact

Then one more call of each with nh_enable_timing for the per-label breakdown, and the pair list against the host oracle byte for byte.

    python tools/contact_events_rates.py [--steps 70] [--reps 5] [--inner 10] [--out profiles/contact_events_rates.log]
    (on a GPU box; prints the table, one JSON line at the end, and writes both to --out)
"""
import json

import rates


def main():
    ap = rates.parser("contact_events_rates")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    import torch
    import hostcontacts_util as HC
    import hostregion_util as R
    land = rates.landed(a, build=False)
    w, nb, log = land.world, land.bodies, rates.Log()

    def new_list(cap):
        return torch.zeros(1, dtype=torch.int32, device=w.dev), torch.empty((max(cap, 1), 64), dtype=torch.uint8, device=w.dev), cap

    res = {}

    def row(name, fn, with_labels=True):
        best, median = rates.best_median(rates.blocks(w, fn, a.reps, a.inner))
        res[name] = dict(ms=best, median_ms=median)
        log.say(f"  {name:74s} {best:9.3f} {median:9.3f}")
        if with_labels:
            res[name]["labels"] = rates.labels(w, fn)
            log.say(f"      labels, ms: {res[name]['labels']}")
        return best

    c0 = w.counts()
    K = c0["contacts"]
    cur = w.step_contact_pairs(out=new_list(K))
    pairs, _ = w.pair_records(cur)
    log.say(f"landed {land.name} world: {nb:,} bodies, {K:,} contacts, {pairs:,} body pairs after {a.steps} steps; GPU {rates.gpu_name(w)}")
    log.say(f"ms per call: the best of {a.reps} blocks of {a.inner} calls after a warm-up, device events around the block; one box, one run")
    log.say(f"  {'':74s} {'ms':>9s} {'median':>9s}")

    # the views are current here (step_contact_pairs exported them): nh_contact_pairs on them
    count_word = torch.tensor([K], dtype=torch.int32, device=w.dev)
    out = new_list(pairs)
    row("nh_contact_pairs on the exported views", lambda: w.contact_pairs_records(w._keep["cd"], w._keep["cb"], w._keep["kd"], count=count_word,
                                                                                capacity=w.max_contacts, body_count=nb, out=out))
    row("nh_contact_pairs, count only", lambda: w.contact_pairs_records(w._keep["cd"], w._keep["cb"], w._keep["kd"], count=count_word,
                                                                      capacity=w.max_contacts, body_count=nb, out=(out[0], None, 0)), with_labels=False)
    row("nh_step_contact_pairs, views current (no export)", lambda: w.step_contact_pairs(out=out))
    same = w.pair_records(out)[1].tobytes() == w.pair_records(cur)[1].tobytes()
    log.say(f"      nh_contact_pairs with the cache's impulses equals nh_step_contact_pairs byte for byte: {same}")

    # against the host oracle
    contacts, cache = w.get_contacts(), w.get_cache()
    n, rec = HC.step_pairs(contacts, cache)
    ok = n == pairs and rec[:n].tobytes() == w.pair_records(cur)[1].tobytes()
    assert ok, "the GPU's pair list differs from the host oracle's"
    log.say("      the pair list equals the host oracle byte for byte")
    del contacts, cache, rec

    # two consecutive steps' lists
    prev = new_list(pairs + 1024)
    w.step_contact_pairs(out=prev)
    w.step(1)
    nxt = new_list(pairs + 1024)
    w.step_contact_pairs(out=nxt)
    began, ended = new_list(pairs + 1024), new_list(pairs + 1024)
    row("nh_contact_events on two consecutive steps' lists", lambda: w.contact_events_records(prev, nxt, began=began, ended=ended))
    log.say(f"      prev {w.pair_records(prev)[0]:,}, cur {w.pair_records(nxt)[0]:,} pairs; began {w.pair_records(began)[0]:,}, ended {w.pair_records(ended)[0]:,}")
    row("nh_contact_events, the first frame (everything begins)", lambda: w.contact_events_records(None, nxt, began=began, ended=ended), with_labels=False)

    # the step, and the call behind every step
    s0 = w.counts()["still_steps"]
    step_still = row("nh_step(1), still steps", lambda: w.step(1), with_labels=False)
    both = row("nh_step(1) + nh_step_contact_pairs, still steps", lambda: (w.step(1), w.step_contact_pairs(out=out)), with_labels=False)
    s1 = w.counts()["still_steps"]
    log.say(f"      nh_step_contact_pairs after a still step (view export included), by difference: {both - step_still:9.3f} ms = {(both - step_still) / step_still:.2f} steps"
            f"   ({s1 - s0} still steps among the steps timed)")
    res["after_still_step"] = dict(ms=both - step_still, steps=(both - step_still) / step_still, still_steps=s1 - s0)
    w.set_option("no_still", 1)
    w.step(2)
    step_full = row("nh_step(1), full steps (option no_still)", lambda: w.step(1), with_labels=False)
    both = row("nh_step(1) + nh_step_contact_pairs, full steps", lambda: (w.step(1), w.step_contact_pairs(out=out)), with_labels=False)
    log.say(f"      nh_step_contact_pairs after a full step, by difference: {both - step_full:9.3f} ms = {(both - step_full) / step_full:.2f} steps"
            f"   ({w.counts()['still_steps'] - s1} still steps among the steps timed)")
    res["after_full_step"] = dict(ms=both - step_full, steps=(both - step_full) / step_full)

    # the nearest existing sort-and-compact: nh_overlap_bodies on one region that is the world (the world has moved: its records are read here, not land.records)
    w.synchronize()
    w.query_build()
    lo, hi = rates.reach_bounds(R.records(w.get_bodies()["transforms"], land.scene))
    qt = rates.upload(w, R.regions(rates.box_planes(lo, hi)))
    ot, _ = w.region_records(qt)
    total = rates.total_of(ot)
    ht = torch.empty((max(total, 1), 16), dtype=torch.uint8, device=w.dev)
    w.region_records(qt, offsets=ot, hits=ht, capacity=total)
    bo, bh = torch.empty(2, dtype=torch.int32, device=w.dev), torch.empty((max(total, 1), 16), dtype=torch.uint8, device=w.dev)
    row(f"nh_overlap_bodies on one list of {total:,} records", lambda: w.overlap_bodies_records(1, (ot, ht, total), bo, bh, total))

    log.say()
    log.say(json.dumps(dict(bodies=nb, contacts=K, pairs=pairs, steps=a.steps, **res)))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
