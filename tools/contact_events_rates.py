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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--tiles", type=int, default=124, help="tiles of the world (a smaller world: a quick check of the tool itself)")
    ap.add_argument("--side", type=int, default=90)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contact_events_rates.log"))
    a = ap.parse_args()
    import torch
    import hostcontacts_util as HC
    import hostregion_util as R
    from events_rates import box_planes
    scene = S.grid_tiles(a.tiles, side=a.side, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP, max_contacts=6 * nb)
    w.step(a.steps)
    w.synchronize()
    stream = torch.cuda.current_stream(w.dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def blocks(fn):
        fn()
        stream.synchronize()
        ts = []
        for _ in range(a.reps):
            ev0.record(stream)
            for _ in range(a.inner):
                fn()
            ev1.record(stream)
            ev1.synchronize()
            ts.append(ev0.elapsed_time(ev1) / a.inner)
        return min(ts), float(np.median(ts))

    def labels(fn):
        w.enable_timing(True)
        w.kernel_times()
        fn()
        out = {k: round(v[0], 4) for k, v in sorted(w.kernel_times().items()) if v[1]}
        w.enable_timing(False)
        return out

    def new_list(cap):
        return torch.zeros(1, dtype=torch.int32, device=w.dev), torch.empty((max(cap, 1), 64), dtype=torch.uint8, device=w.dev), cap

    res = {}

    def row(name, fn, with_labels=True):
        best, median = blocks(fn)
        res[name] = dict(ms=best, median_ms=median)
        say(f"  {name:74s} {best:9.3f} {median:9.3f}")
        if with_labels:
            res[name]["labels"] = labels(fn)
            say(f"      labels, ms: {res[name]['labels']}")
        return best

    c0 = w.counts()
    K = c0["contacts"]
    cur = w.step_contact_pairs(out=new_list(K))
    pairs, _ = w.pair_records(cur)
    say(f"landed config-2 world: {nb:,} bodies, {K:,} contacts, {pairs:,} body pairs after {a.steps} steps; GPU {torch.cuda.get_device_name(w.dev)}")
    say(f"ms per call: the best of {a.reps} blocks of {a.inner} calls after a warm-up, device events around the block; one box, one run")
    say(f"  {'':74s} {'ms':>9s} {'median':>9s}")

    # the views are current here (step_contact_pairs exported them): nh_contact_pairs on them
    count_word = torch.tensor([K], dtype=torch.int32, device=w.dev)
    out = new_list(pairs)
    row("nh_contact_pairs on the exported views", lambda: w.contact_pairs_records(w._keep["cd"], w._keep["cb"], w._keep["kd"], count=count_word,
                                                                                capacity=w.max_contacts, body_count=nb, out=out))
    row("nh_contact_pairs, count only", lambda: w.contact_pairs_records(w._keep["cd"], w._keep["cb"], w._keep["kd"], count=count_word,
                                                                      capacity=w.max_contacts, body_count=nb, out=(out[0], None, 0)), with_labels=False)
    row("nh_step_contact_pairs, views current (no export)", lambda: w.step_contact_pairs(out=out))
    same = w.pair_records(out)[1].tobytes() == w.pair_records(cur)[1].tobytes()
    say(f"      nh_contact_pairs with the cache's impulses equals nh_step_contact_pairs byte for byte: {same}")

    # against the host oracle
    contacts, cache = w.get_contacts(), w.get_cache()
    n, rec = HC.step_pairs(contacts, cache)
    ok = n == pairs and rec[:n].tobytes() == w.pair_records(cur)[1].tobytes()
    assert ok, "the GPU's pair list differs from the host oracle's"
    say("      the pair list equals the host oracle byte for byte")
    del contacts, cache, rec

    # two consecutive steps' lists
    prev = new_list(pairs + 1024)
    w.step_contact_pairs(out=prev)
    w.step(1)
    nxt = new_list(pairs + 1024)
    w.step_contact_pairs(out=nxt)
    began, ended = new_list(pairs + 1024), new_list(pairs + 1024)
    row("nh_contact_events on two consecutive steps' lists", lambda: w.contact_events_records(prev, nxt, began=began, ended=ended))
    say(f"      prev {w.pair_records(prev)[0]:,}, cur {w.pair_records(nxt)[0]:,} pairs; began {w.pair_records(began)[0]:,}, ended {w.pair_records(ended)[0]:,}")
    row("nh_contact_events, the first frame (everything begins)", lambda: w.contact_events_records(None, nxt, began=began, ended=ended), with_labels=False)

    # the step, and the call behind every step
    s0 = w.counts()["still_steps"]
    step_still = row("nh_step(1), still steps", lambda: w.step(1), with_labels=False)
    both = row("nh_step(1) + nh_step_contact_pairs, still steps", lambda: (w.step(1), w.step_contact_pairs(out=out)), with_labels=False)
    s1 = w.counts()["still_steps"]
    say(f"      nh_step_contact_pairs after a still step (view export included), by difference: {both - step_still:9.3f} ms = {(both - step_still) / step_still:.2f} steps"
        f"   ({s1 - s0} still steps among the steps timed)")
    res["after_still_step"] = dict(ms=both - step_still, steps=(both - step_still) / step_still, still_steps=s1 - s0)
    w.set_option("no_still", 1)
    w.step(2)
    step_full = row("nh_step(1), full steps (option no_still)", lambda: w.step(1), with_labels=False)
    both = row("nh_step(1) + nh_step_contact_pairs, full steps", lambda: (w.step(1), w.step_contact_pairs(out=out)), with_labels=False)
    say(f"      nh_step_contact_pairs after a full step, by difference: {both - step_full:9.3f} ms = {(both - step_full) / step_full:.2f} steps"
        f"   ({w.counts()['still_steps'] - s1} still steps among the steps timed)")
    res["after_full_step"] = dict(ms=both - step_full, steps=(both - step_full) / step_full)

    # the nearest existing sort-and-compact: nh_overlap_bodies on one region that is the world
    w.synchronize()
    w.query_build()
    rc = R.records(w.get_bodies()["transforms"], scene)
    reach = np.linalg.norm(rc["h"].astype(np.float64), axis=1, keepdims=True)
    lo, hi = (rc["p"] - reach).min(axis=0) - 1.0, (rc["p"] + reach).max(axis=0) + 1.0
    qt = torch.from_numpy(np.ascontiguousarray(R.regions(box_planes(lo, hi))).view(np.uint8).copy()).to(w.dev)
    ot, _ = w.region_records(qt)
    total = int(ot[-1].item()) & NONE
    ht = torch.empty((max(total, 1), 16), dtype=torch.uint8, device=w.dev)
    w.region_records(qt, offsets=ot, hits=ht, capacity=total)
    bo, bh = torch.empty(2, dtype=torch.int32, device=w.dev), torch.empty((max(total, 1), 16), dtype=torch.uint8, device=w.dev)
    row(f"nh_overlap_bodies on one list of {total:,} records", lambda: w.overlap_bodies_records(1, (ot, ht, total), bo, bh, total))

    say()
    say(json.dumps(dict(bodies=nb, contacts=K, pairs=pairs, steps=a.steps, **res)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    w.close()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
