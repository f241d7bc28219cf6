"""nh_overlap_wide / nh_penetration_wide rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h,
"nh_overlap_wide"), beside nh_overlap / nh_penetration on identical queries in the same process -- their kernels are the parent commit's, so that is
the parent's time -- and beside nh_region on the matching cubes.  Per case the count-only call and the count + exactly sized list call, ms per call as
the best of --reps blocks of --inner calls after a warm-up, by device events around the block (tools/region_rates.py's method; the one-lane twins one
call a block); then one more pair of calls with nh_enable_timing for the per-label breakdown.

    (a)  one box equal to the world's AABB                     nh_overlap_wide / nh_overlap (one lane walks it all) / nh_region
    (d)  4,096 cubes of one tile's size around random bodies   nh_overlap_wide / nh_overlap / nh_region
    (s)  4,096 spheres around the same bodies at each of --radii, from a body's size to a tile's: where the two calls cross
    (dp) the cubes of (d) through nh_penetration_wide / nh_penetration

Every pair of calls is compared byte for byte (offsets and records) before it is timed.

With NUDGE_HIP_LIBRARY naming another build of the library (the parent commit's: tools/build_variant.sh parent "" <rev>), a second world on THAT library
is stepped and built in the same process -- and a second world on each library, since two worlds of one build differ by where their memory lies -- and
nh_overlap, nh_penetration and nh_region of the four worlds are timed side by side in alternating blocks: this / other beside each build against itself.

    [NUDGE_HIP_LIBRARY=.../libparent.so] python tools/overlap_wide_rates.py [--steps 70] [--reps 5] [--inner 20] [--out profiles/overlap_wide_rates.log]
    (on a GPU box; prints the table, one JSON line at the end, and writes both to --out)
"""
import json
import os

import numpy as np

import rates
OTHER = rates.other_library()
from rates import box_planes
from nudge_amd import engine as E           # noqa: E402


def main():
    ap = rates.parser("overlap_wide_rates")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="wide and nh_region calls per timed block (calls that take 20 ms or more are timed one a block)")
    ap.add_argument("--walk-reps", type=int, default=1, help="calls of the one-lane nh_overlap twin of (a): each takes seconds")
    ap.add_argument("--cubes", type=int, default=4096)
    ap.add_argument("--radii", type=float, nargs="+", default=[1.5, 6.0, 12.0, 24.0, 96.0, 267.0])
    a = ap.parse_args()
    import torch
    import hostregion_util as R
    land = rates.landed(a)
    w = land.world
    other = other2 = this2 = None
    if OTHER:
        first = rates.landed(a, OTHER, like=land)
        other, other2 = first.world, rates.landed(a, first, like=land).world          # (each library twice: what two worlds of ONE build differ by)
        this2 = rates.landed(a, land, like=land).world
    st = w.query_stats()
    up, log = rates.upload, rates.Log()
    rec = land.records
    C = len(rec)
    lo, hi = rates.reach_bounds(rec)
    dyn = rec["p"][rec["body"] != 0].astype(np.float64)
    tile_size = rates.tile_size(land.scene, w.get_bodies()["transforms"]["position"])
    rng = np.random.default_rng(1)
    centres = dyn[rng.integers(0, len(dyn), size=a.cubes)]
    half = 0.5 * tile_size

    def spheres(r):
        return rates.overlap_queries(centres, np.repeat([[r, 0.0, 0.0]], a.cubes, axis=0), E.NH_SHAPE_SPHERE)

    log.say(f"landed {land.name} world: {C:,} colliders, {land.bodies:,} bodies, after {a.steps} steps; {st['runs']} runs, {st['top_nodes'] + 1} entry nodes; "
            f"GPU {rates.gpu_name(w)}")
    log.say(f"ms per call: the best of {a.reps} blocks of {a.inner} calls after a warm-up (calls of 20 ms or more: blocks of one call), device events around "
            f"the block; one box, one run.  tile size {tile_size:.1f}")
    log.say(f"  {'case':66s} {'queries':>8s} {'records':>11s} {'count ms':>10s} {'count+list ms':>14s}")
    out = {}

    def row(name, n, r):
        log.say(f"  {name:66s} {n:8,d} {r['records']:11,d} {r['count_ms']:10.3f} {r['list_ms']:14.3f}   (medians {r['count_median_ms']:.3f}, {r['list_median_ms']:.3f})")
        if r["labels"]:
            log.say(f"      labels of count + list, ms: {r['labels']}")

    def pair(key, name, q, wide, plain, size, plain_reps, region=None):
        """One case: the wide call, the plain call on the same queries (the same bytes), and nh_region on the matching planes."""
        qt = up(w, q)
        rw, dw = rates.count_then_list(w, wide, qt, len(q), size, a.reps, a.inner, keep=True)
        row(f"{name}, {wide.__name__[:-8]}", len(q), rw)
        # (a plain call of 20 ms or more is timed one call a block; below that, in blocks like the wide one)
        probe = rates.blocks(w, lambda: plain(qt, offsets=torch.empty(len(q) + 1, dtype=torch.int32, device=w.dev)), 1, 1, warm=0)[0]
        rp, dp = rates.count_then_list(w, plain, qt, len(q), size, plain_reps, 1 if probe >= 20.0 else a.inner, breakdown=probe < 1000.0, keep=True)
        row(f"    {plain.__name__[:-8]}, the same queries", len(q), rp)
        assert dw == dp, f"{key}: the wide call and the plain call differ"
        log.say(f"      the same bytes from both ({rw['records']:,} records); plain / wide: count {rp['count_ms'] / rw['count_ms']:.2f} x, "
                f"count + list {rp['list_ms'] / rw['list_ms']:.2f} x")
        out[key], out[key + "_plain"] = rw, rp
        if region is not None:
            rr, _ = rates.count_then_list(w, w.region_records, up(w, region), len(region), 16, a.reps, a.inner)
            row("    nh_region, the same boxes as six planes", len(region), rr)
            more = rr["records"] - rw["records"]
            log.say(f"      wide / nh_region: count {rw['count_ms'] / rr['count_ms']:.2f} x, count + list {rw['list_ms'] / rr['list_ms']:.2f} x"
                    + (f"   (the plane test lists {more:,} more: edges and corners)" if more else ""))
            out[key + "_region"] = rr

    world_box = rates.overlap_queries([0.5 * (lo + hi)], [0.5 * (hi - lo)], E.NH_SHAPE_BOX)
    cubes = rates.overlap_queries(centres, np.full((a.cubes, 3), half), E.NH_SHAPE_BOX)
    cube_planes = R.regions(box_planes(centres - half, centres + half))
    pair("a", "(a) one box equal to the world's AABB", world_box, w.overlap_wide_records, w.overlap_records, 16, a.walk_reps, R.regions(box_planes(lo, hi)))
    assert out["a"]["records"] == C, "the world's AABB does not hold every collider"
    pair("d", f"(d) {a.cubes:,} cubes of a tile's size ({tile_size:.0f})", cubes, w.overlap_wide_records, w.overlap_records, 16, a.reps, cube_planes)
    cross = []
    for r in a.radii:
        key = f"s{r:g}"
        pair(key, f"(s) {a.cubes:,} spheres of radius {r:g}", spheres(r), w.overlap_wide_records, w.overlap_records, 16, a.reps)
        cross.append((r, out[key + "_plain"]["count_ms"] / out[key]["count_ms"], out[key + "_plain"]["list_ms"] / out[key]["list_ms"]))
    log.say("  plain / wide by radius (above 1: the wide call is the faster): " + ", ".join(f"r = {r:g}: count {c:.2f}, count + list {l:.2f}" for r, c, l in cross))
    pair("dp", "(dp) the cubes of (d), penetration", cubes, w.penetration_wide_records, w.penetration_records, 32, a.reps)

    # 8 cubes, 8 spheres and the capsule twins of the spheres, byte for byte against the brute force over all colliders
    import hostoverlap_util as O
    caps = spheres(24.0)[:8]
    caps["shape"], caps["size"][:, 1], caps["rotation"] = E.NH_SHAPE_CAPSULE, 40.0, (0.5, 0.5, 0.5, 0.5)
    pick = np.concatenate([cubes[:8], spheres(24.0)[:8], caps])
    ref_off, ref_hits, total = O.overlap(rec, w.nbox, pick, capsules=True)
    ot, ht = w.overlap_wide_records(up(w, pick), hits=torch.empty((total, 16), dtype=torch.uint8, device=w.dev), capacity=total)
    assert ot.cpu().numpy().view(np.uint32).tobytes() == ref_off.tobytes() and ht.cpu().numpy().tobytes() == ref_hits[:total].tobytes(), "the GPU differs from the brute force"
    log.say(f"  {len(pick)} queries ({total:,} records) equal the brute force byte for byte")

    # the existing calls, this library beside another build: alternating blocks, the spread of each against itself
    if other is not None:
        log.say()
        log.say(f"the existing calls, two worlds on this library beside two worlds on {os.path.basename(OTHER)} (ms per call, count + list; "
                f"min / median / max of {a.reps} alternating blocks each):")
        ab = {}
        small = spheres(1.5)
        for name, q, size, call, inner in (("nh_overlap, 4,096 spheres r = 1.5", small, 16, "overlap_records", a.inner),
                                           ("nh_overlap, (d)", cubes, 16, "overlap_records", 1),
                                           ("nh_penetration, 4,096 spheres r = 1.5", small, 32, "penetration_records", a.inner),
                                           ("nh_region, (d)", cube_planes, 16, "region_records", a.inner)):
            qt = up(w, q)
            fns = {}
            for tag, wd in (("this", w), ("other", other), ("other2", other2), ("this2", this2)):
                rec_fn = getattr(wd, call)
                ot = torch.empty(len(q) + 1, dtype=torch.int32, device=w.dev)
                rec_fn(qt, offsets=ot)
                total = rates.total_of(ot)
                ht = torch.empty((max(total, 1), size), dtype=torch.uint8, device=w.dev)
                fns[tag] = (lambda f=rec_fn, o=ot, h=ht, t=total: (f(qt, offsets=o), f(qt, offsets=o, hits=h, capacity=t)))
                fns[tag]()                                                      # warm-up
            ts = rates.interleaved(w, fns, inner, a.reps, warm=0)
            ab[name] = ts
            log.say(f"  {name:38s} " + "   ".join(f"{tag} {min(v):8.3f} / {np.median(v):8.3f} / {max(v):8.3f}" for tag, v in ts.items()))
            m = {tag: float(np.median(v)) for tag, v in ts.items()}
            log.say(f"  {'':38s} this / other {m['this'] / m['other']:.3f}, this2 / other2 {m['this2'] / m['other2']:.3f}; one build against itself: "
                    f"this2 / this {m['this2'] / m['this']:.3f}, other2 / other {m['other2'] / m['other']:.3f} (medians)")
        out["ab"] = ab
    else:
        log.say("the existing calls, this library beside another build: no NUDGE_HIP_LIBRARY given, not measured")
    log.say()
    log.say(json.dumps(dict(colliders=C, steps=a.steps, entries=st["top_nodes"] + 1, tile_size=tile_size, **out)))
    log.write(a.out)
    for wd in (w, other, other2, this2):
        if wd is not None:
            wd.close()


if __name__ == "__main__":
    main()
