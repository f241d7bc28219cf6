"""nh_region rates on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "nh_region"), and beside them in the same
process the only tool there was for a large question, nh_overlap with a large box.  Per case the count-only call and the count + exactly sized list
call, ms per call as the best of --reps blocks of --inner calls after a warm-up, by device events around the block (the nh_overlap twins one call a
block); then one more call of each with nh_enable_timing for the per-label
breakdown (q_region_count, q_region_list, the scan, the sort, q_overlap_gather).

    (a) one six-plane region that is the world's AABB                     beside nh_overlap with one box query equal to that AABB (one lane walks it all)
    (b) one perspective frustum that sees about a tenth of the colliders  (its far plane found by bisection on the count)
    (c) 64 such frusta, eyes on a ring around the world
    (d) 4,096 cubes of one tile's size around random bodies               beside nh_overlap with the same cubes as box queries (a lane per cube)

The two nh_overlap calls are existing calls: they say which call is for which size of question.  Totals of a region and its nh_overlap twin are
compared; they may differ by the few colliders near edges and corners that the plane-by-plane test keeps and the box test does not.

    python tools/region_rates.py [--steps 70] [--reps 5] [--inner 20] [--out profiles/region_rates.log]
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


def box_planes(lo, hi):
    """The six planes of the axis-aligned boxes [lo, hi] ((n, 3) each), as (n, 6, 4)."""
    lo, hi = np.atleast_2d(lo), np.atleast_2d(hi)
    out = np.zeros((len(lo), 6, 4), dtype=np.float32)
    for k in range(3):
        out[:, 2 * k, k], out[:, 2 * k, 3] = 1.0, -lo[:, k]
        out[:, 2 * k + 1, k], out[:, 2 * k + 1, 3] = -1.0, hi[:, k]
    return out


def camera(eye, target, fov_deg, aspect, near, far):
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, (0.0, 1.0, 0.0))
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    view = np.eye(4)
    view[0, :3], view[1, :3], view[2, :3] = right, up, -fwd
    view[:3, 3] = -view[:3, :3] @ eye
    f = 1.0 / np.tan(np.radians(fov_deg) / 2)
    proj = np.array([[f / aspect, 0, 0, 0], [0, f, 0, 0], [0, 0, (far + near) / (near - far), 2 * far * near / (near - far)], [0, 0, -1, 0]])
    return E.frustum_planes(proj @ view)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=70)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="nh_region calls per timed block (the nh_overlap twins are timed one call at a time)")
    ap.add_argument("--walk-reps", type=int, default=1, help="calls of the one-lane nh_overlap twin of (a): each takes seconds")
    ap.add_argument("--cubes", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_rates.log"))
    a = ap.parse_args()
    import torch
    import hostregion_util as R
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP, max_contacts=6 * nb)
    w.step(a.steps)
    w.synchronize()
    w.query_build()
    st = w.query_stats()
    stream = torch.cuda.current_stream(w.dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def up(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).to(w.dev)

    rec = R.records(w.get_bodies()["transforms"], scene)
    C = len(rec)
    reach = np.linalg.norm(rec["h"].astype(np.float64), axis=1, keepdims=True)
    lo, hi = (rec["p"] - reach).min(axis=0) - 1.0, (rec["p"] + reach).max(axis=0) + 1.0
    dyn = rec["p"][rec["body"] != 0].astype(np.float64)
    dlo, dhi = dyn.min(axis=0), dyn.max(axis=0)
    tile = np.nonzero(np.asarray(scene["tile_of_body"]) == 0)[0]
    tp = w.get_bodies()["transforms"]["position"][tile].astype(np.float64)
    tile_size = float((tp.max(axis=0) - tp.min(axis=0))[[0, 2]].max())

    def count_of(planes):
        off, _ = w.region_records(up(R.regions(planes)))
        return int(off[-1].item()) & 0xFFFFFFFF

    # (b): from outside a corner of the world, looking at its middle; the far plane by bisection on the count
    mid = 0.5 * (dlo + dhi)
    eye = np.array([dlo[0] - 20.0, dhi[1] + 40.0, dlo[2] - 20.0])
    near, f_lo, f_hi = 1.0, 2.0, 2.0 * float(np.linalg.norm(hi - lo))
    for _ in range(24):
        far = 0.5 * (f_lo + f_hi)
        if count_of(camera(eye, mid, 50.0, 1.6, near, far)) < C // 10:
            f_lo = far
        else:
            f_hi = far
    far = f_hi
    rng = np.random.default_rng(1)
    ring = []
    radius = 0.5 * float(np.linalg.norm((dhi - dlo)[[0, 2]])) + 20.0
    for k in range(64):
        ang = 2 * np.pi * k / 64
        e = mid + np.array([radius * np.cos(ang), dhi[1] - mid[1] + 40.0, radius * np.sin(ang)])
        ring.append(camera(e, mid + rng.normal(scale=5.0, size=3), 50.0, 1.6, near, far))
    centres = dyn[rng.integers(0, len(dyn), size=a.cubes)]
    half = 0.5 * tile_size
    cases = {
        "a": R.regions(box_planes(lo, hi)),
        "b": R.regions(camera(eye, mid, 50.0, 1.6, near, far)),
        "c": R.regions(np.stack(ring)),
        "d": R.regions(box_planes(centres - half, centres + half)),
    }

    def boxes(c, h):
        q = np.zeros(len(c), dtype=E.OVERLAP_QUERY)
        q["center"], q["size"], q["shape"], q["rotation"], q["ignore_body"] = c, h, E.NH_SHAPE_BOX, (0, 0, 0, 1), NONE
        return q
    twins = {"a": boxes([0.5 * (lo + hi)], [0.5 * (hi - lo)]), "d": boxes(centres, np.full((a.cubes, 3), half))}

    def measure(records, q, reps, inner, breakdown=True):
        """(total, best and median ms per call of the count-only call and of count + exactly sized list over `reps` blocks of `inner` calls, the labels of
        one more pair of calls where `breakdown`)."""
        qt = up(q)
        ot = torch.empty(len(q) + 1, dtype=torch.int32, device=w.dev)
        records(qt, offsets=ot)
        total = int(ot[-1].item()) & 0xFFFFFFFF
        ht = torch.empty((max(total, 1), 16), dtype=torch.uint8, device=w.dev)
        fns = (lambda: records(qt, offsets=ot), lambda: (records(qt, offsets=ot), records(qt, offsets=ot, hits=ht, capacity=total)))
        fns[1]()                                                          # warm-up: the scratch grows here
        stream.synchronize()
        best = []
        for fn in fns:
            ts = []
            for _ in range(reps):
                ev0.record(stream)
                for _ in range(inner):
                    fn()
                ev1.record(stream)
                ev1.synchronize()
                ts.append(ev0.elapsed_time(ev1) / inner)
            best.append((min(ts), float(np.median(ts))))
        labels = {}
        if breakdown:
            w.enable_timing(True)
            w.kernel_times()
            fns[1]()
            labels = {k: round(v[0], 4) for k, v in sorted(w.kernel_times().items()) if v[1]}
            w.enable_timing(False)
        return total, best[0], best[1], labels

    say(f"landed config-2 world: {C:,} colliders, {nb:,} bodies, after {a.steps} steps; {st['runs']} runs, {st['top_nodes'] + 1} entry nodes; "
        f"GPU {torch.cuda.get_device_name(w.dev)}")
    say(f"ms per call: the best of {a.reps} blocks of {a.inner} calls after a warm-up, device events around the block; one box, one run.  "
        f"tile size {tile_size:.1f}, frustum far plane {far:.1f}")
    say(f"  {'case':58s} {'regions':>8s} {'records':>11s} {'count ms':>10s} {'count+list ms':>14s}")
    names = {"a": "(a) nh_region, the world's AABB", "b": "(b) nh_region, a frustum that sees a tenth", "c": "(c) nh_region, 64 such frusta",
             "d": f"(d) nh_region, {a.cubes:,} cubes of a tile's size"}
    out = {}
    for key, regs in cases.items():
        total, (t_count, m_count), (t_list, m_list), labels = measure(w.region_records, regs, a.reps, a.inner)
        out[key] = dict(regions=len(regs), records=total, count_ms=t_count, list_ms=t_list, count_median_ms=m_count, list_median_ms=m_list, labels=labels)
        say(f"  {names[key]:58s} {len(regs):8,d} {total:11,d} {t_count:10.3f} {t_list:14.3f}   (medians {m_count:.3f}, {m_list:.3f})")
        say(f"      labels of count + list, ms: {labels}")
        if key in twins:
            reps = a.walk_reps if key == "a" else a.reps
            total2, (o_count, mo_count), (o_list, mo_list), labels = measure(w.overlap_records, twins[key], reps, 1, breakdown=key != "a")
            out[key + "_overlap"] = dict(queries=len(twins[key]), records=total2, count_ms=o_count, list_ms=o_list, count_median_ms=mo_count, list_median_ms=mo_list,
                                         labels=labels)
            say(f"  {'    nh_overlap, the same as box queries (%d x 1 call)' % reps:58s} {len(twins[key]):8,d} {total2:11,d} {o_count:10.3f} {o_list:14.3f}"
                f"   (medians {mo_count:.3f}, {mo_list:.3f})")
            say(f"      nh_overlap / nh_region: count {o_count / t_count:.1f} x, count + list {o_list / t_list:.1f} x"
                f"{'' if total2 == total else f'   (the box test lists {total - total2:,} fewer: edges and corners)'}")
    assert out["a"]["records"] == C, "the world's AABB does not hold every collider"
    # 3 regions of (c) and 8 of (d), byte for byte against the brute force over all colliders
    pick = np.concatenate([cases["c"][:3], cases["d"][:8]])
    ref_off, ref_hits, total = R.region(rec, w.nbox, pick)
    ot, ht = w.region_records(up(pick), hits=torch.empty((total, 16), dtype=torch.uint8, device=w.dev), capacity=total)
    assert ot.cpu().numpy().view(np.uint32).tobytes() == ref_off.tobytes() and ht.cpu().numpy().tobytes() == ref_hits[:total].tobytes(), "the GPU differs from the brute force"
    say(f"  {len(pick)} regions ({total:,} records) equal the brute force byte for byte")
    say()
    say(json.dumps(dict(colliders=C, steps=a.steps, entries=st["top_nodes"] + 1, **out)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    w.close()


if __name__ == "__main__":
    main()
