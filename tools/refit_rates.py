"""nh_query_refit against nh_query_build on the landed config-2 world (1,004,400 boxes + 124 ground slabs; include/nudge_hip.h, "scene queries").

A/B: the refit and the build of this tree's library against the build of the PARENT commit's library (tools/build_variant.sh parent "" <rev> ->
nudge_amd/_ab/libparent.so), each library in a fresh child process of its own (engine reads NUDGE_HIP_LIBRARY), alternating A B A B, every child
under its own time limit and the chain ending at the first child that fails.  Device-event time of every repetition apart, so that the spread is
in the log; per-kernel times from nh_kernel_times with a byte model's share of 8 TB/s; the steps of the same run for scale; the number of nodes of
the box pass's top phase and the height of their tree (nh_query_stats).

Decay: from step 0 (everything in the air) one build, then nh_step(1) + nh_query_refit per step; at steps 1, 10, 30 and 70 the time of 1 M
incoherent closest-hit rays and of 1 M unbounded nh_closest queries on the refitted tree beside a fresh build of the same state in a second world
stepped alike, with 2048 records of each compared byte for byte.

    tools/build_variant.sh parent "" <parent rev>                (where the tree is a git repository; hipcc cross-compiles)
    python tools/refit_rates.py [--steps 70] [--reps 10]          (on a GPU box; prints the tables, writes profiles/refit_rates.log)
"""
import json
import os
import subprocess
import sys

import numpy as np

import rates

PARENT = os.path.join(rates.ROOT, "nudge_amd", "_ab", "libparent.so")
HBM = 8.0e12
DECAY_AT = (1, 10, 30, 70)


# bytes each kernel of the box pass moves at C colliders, read + write, every record once (caches not modelled)
#   q_boxes_runs: per leaf index 4 + collider transform 32 + body transform 32 + shape 16 + tag 4 + parent word 4 + escape 4 in, record 48 + leaf node
#                 32 out; per internal node its parent word 4 in and its box 24 out
#   q_boxes_top:  per top node two child boxes 64 + links 12 in, its box 24 out, the counter 8
#   q_links:      last 4 + table 4 in, the link 4 out per internal node
def byte_model(C, top):
    return {"q_boxes_runs": C * (4 + 32 + 32 + 16 + 4 + 4 + 4 + 48 + 32) + (C - 1) * (4 + 24), "q_boxes_top": top * (64 + 12 + 24 + 8), "q_links": (C - 1) * 12,
            "q_xform": C * (32 + 32 + 16 + 4 + 48), "q_keys": C * (16 + 8 + 4), "q_tree": (C - 1) * (4 * 8 + 28)}


def measure_ab(a):
    """The figures of the library this process loaded: one dict.  Every repetition's device-event time apart (blocks of one call after a warm-up)."""
    from nudge_amd import engine as E
    land = rates.landed(a, build=False)
    w, reps = land.world, a.reps
    has_refit = hasattr(w.L, "nh_query_refit")
    out = dict(library=os.path.relpath(E._LIB_PATH, rates.ROOT), gpu=rates.gpu_name(w), colliders=land.colliders, bodies=land.bodies, has_refit=has_refit)
    out["build_ms"] = rates.blocks(w, w.query_build, reps, 1)
    if has_refit:
        out["refit_ms"] = rates.blocks(w, w.query_refit, reps, 1)
        out["stats"] = w.query_stats()

    def kernels(fn):
        return {k: (v[0] / reps, v[1] // reps) for k, v in rates.kernel_times(w, fn, reps).items()}
    out["build_kernels"] = kernels(w.query_build)
    if has_refit:
        out["refit_kernels"] = kernels(w.query_refit)
    # the steps of this run, for scale: one nh_step call of one sub-step; the landed world's step inside a longer call (still steps, as the counters
    # say); the same with the still path switched off (full steps)
    out["step1_ms"] = rates.blocks(w, lambda: w.step(1), reps, 1)
    c0 = w.counts()
    out["still_ms"] = [t / 10 for t in rates.blocks(w, lambda: w.step(10), reps, 1)]
    c1 = w.counts()
    out["still_share"] = (c1["still_steps"] - c0["still_steps"]) / float(10 * (reps + 1))
    w.set_option("no_still", 1)
    out["full_ms"] = [t / 10 for t in rates.blocks(w, lambda: w.step(10), reps, 1)]
    c2 = w.counts()
    out["full_still_share"] = (c2["still_steps"] - c1["still_steps"]) / float(10 * (reps + 1))
    out["error"] = c2["error"]
    w.close()
    return out


def measure_decay(a):
    import torch
    from nudge_amd import engine as E
    land = rates.landed(a, build=False, steps=0)
    refit, fresh = land.world, rates.landed(a, build=False, steps=0, like=land).world
    n, reps, lo, hi = a.queries, a.reps, land.lo, land.hi
    rays, _ = rates.ray_sets(np.random.default_rng(1), n, lo, hi)          # tools/query_rates.py's incoherent rays
    pick = torch.from_numpy(np.linspace(0, n - 1, 2048).astype(np.int64))
    rows = []
    refit.query_build()
    done = 0
    for at in DECAY_AT:
        while done < at:
            refit.step(1)
            refit.query_refit()
            fresh.step(1)
            done += 1
        fresh.query_build()
        refit.synchronize(); fresh.synchronize()
        live = refit.get_bodies()["transforms"]["position"][1:].astype(np.float64)
        q = rates.point_queries(np.random.default_rng(5).uniform(lo, np.maximum(hi, live.max(axis=0)), size=(n, 3)), np.inf)
        row = dict(step=at)
        for w, side in ((refit, "refit"), (fresh, "fresh")):
            rt, qt = rates.upload(w, rays), rates.upload(w, q)
            rh = torch.empty((n, 32), dtype=torch.uint8, device=w.dev)
            qh = torch.empty((n, 48), dtype=torch.uint8, device=w.dev)
            row[f"rays_{side}_ms"] = float(np.mean(rates.blocks(w, lambda: w.raycast_records(rt, hits=rh), reps, 1)))
            row[f"closest_{side}_ms"] = float(np.mean(rates.blocks(w, lambda: w.closest_records(qt, hits=qh), reps, 1)))
            row[f"rays_{side}"] = rh.cpu()[pick].numpy().tobytes().hex()
            row[f"closest_{side}"] = qh.cpu()[pick].numpy().tobytes().hex()
            row[f"hit_share_{side}"] = float((rates.download(rh, E.RAY_HIT)["shape"] != rates.NONE).mean())
        same = [row.pop(f"{k}_refit") == row.pop(f"{k}_fresh") for k in ("rays", "closest")]
        row["same_bytes"] = all(same)
        row["refit_ms"] = float(np.mean(rates.blocks(refit, refit.query_refit, reps, 1)))
        rows.append(row)
    out = dict(rows=rows, error=refit.counts()["error"] | fresh.counts()["error"])
    refit.close(); fresh.close()
    return out


def _child(mode, library, a, limit):
    env = dict(os.environ)
    env.pop("NUDGE_HIP_LIBRARY", None)
    if library:
        env["NUDGE_HIP_LIBRARY"] = library
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--reps", str(a.reps), "--queries", str(a.queries)] + rates.world_flags(a),
                           env=env, capture_output=True, text=True, timeout=limit)
    if child.returncode != 0:
        sys.exit(f"the {mode} child of {library or 'the library'} failed ({child.returncode}); nothing more is started:\n{child.stderr[-3000:]}")
    print(f"[{mode} child of {library or 'the library'}: done]", file=sys.stderr, flush=True)
    return json.loads(child.stdout.strip().split("\n")[-1])


def _span(v):
    return f"{np.mean(v):8.4f}  [{min(v):.4f} .. {max(v):.4f}]"


def main():
    ap = rates.parser("refit_rates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--child", choices=("ab", "decay"), help="measure with the library this process loads and print one JSON line")
    a = ap.parse_args()
    if a.child == "ab":
        print(json.dumps(measure_ab(a)))
        return
    if a.child == "decay":
        print(json.dumps(measure_decay(a)))
        return
    if not os.path.exists(PARENT):
        sys.exit(f"{PARENT} is missing: tools/build_variant.sh parent \"\" <parent rev>")
    runs = [_child("ab", lib, a, 420) for lib in (None, PARENT, None, PARENT)]      # A B A B
    new, old = [runs[0], runs[2]], [runs[1], runs[3]]
    assert all(r["error"] == 0 for r in runs)
    decay = _child("decay", None, a, 900)
    assert decay["error"] == 0

    log = rates.Log()
    r0 = new[0]
    st = r0["stats"]
    log.say(f"landed {rates.world_name(a.tiles, a.world_side)} world: {r0['colliders']:,} colliders, {r0['bodies']:,} bodies, after {a.steps} steps; GPU {r0['gpu']}; "
            f"device-event time per call, {a.reps} repetitions after a warm-up, mean [min .. max] in ms; a fresh process per library, order A B A B")
    log.say(f"box pass: runs of {st['run_length']} leaves, {st['runs']} runs; top phase: {st['top_nodes']} nodes, the tree they form is {st['top_depth']} high")
    for k, (n_, o_) in enumerate(zip(new, old)):
        log.say(f"run {k + 1}  A {n_['library']:<28} nh_query_refit {_span(n_['refit_ms'])}   nh_query_build {_span(n_['build_ms'])}")
        log.say(f"run {k + 1}  B {o_['library']:<28} {'':<14} {'':<30}   nh_query_build {_span(o_['build_ms'])}")
    refit = [t for r in new for t in r["refit_ms"]]
    build_new = [t for r in new for t in r["build_ms"]]
    build_old = [t for r in old for t in r["build_ms"]]
    full = [t for r in new for t in r["full_ms"]]
    still = [t for r in new for t in r["still_ms"]]
    step1 = [t for r in new for t in r["step1_ms"]]
    log.say(f"nh_query_refit                 {_span(refit)}")
    log.say(f"nh_query_build, this library   {_span(build_new)}")
    log.say(f"nh_query_build, parent library {_span(build_old)}")
    verdict = "BEATS" if max(refit) < min(build_old) else "DOES NOT BEAT"
    log.say(f"THE BAR: the slowest refit repetition ({max(refit):.4f}) {verdict} the fastest parent build repetition ({min(build_old):.4f}): "
            f"parent build / refit = {np.mean(build_old) / np.mean(refit):.1f}x; parent build / this build = {np.mean(build_old) / np.mean(build_new):.2f}x")
    log.say(f"steps of the same runs: still step {_span(still)} ({100 * r0['still_share']:.0f} % still steps), full step (option no_still) {_span(full)} "
            f"({100 * r0['full_still_share']:.0f} % still steps), one-sub-step nh_step call {_span(step1)}")
    ratio = np.mean(refit) / np.mean(full)
    log.say(f"EXPECTATION (keeping the hierarchy current costs about one full step): refit = {ratio:.2f} full steps = {np.mean(refit) / np.mean(still):.2f} still steps: "
            f"{'met' if ratio <= 1.0 else 'missed'}; this build = {np.mean(build_new) / np.mean(full):.1f} full steps; parent build = {np.mean(build_old) / np.mean(full):.1f} full steps")
    model = byte_model(r0["colliders"], st["top_nodes"])
    for title, key, src in (("nh_query_refit, this library", "refit_kernels", r0), ("nh_query_build, this library", "build_kernels", r0),
                            ("nh_query_build, parent library", "build_kernels", old[0])):
        log.say(f"{title}: {'kernel':<16}{'ms/call':>10}{'launches':>10}{'MB':>10}{'% of 8 TB/s':>13}")
        for k, (ms, launches) in sorted(src[key].items(), key=lambda kv: -kv[1][0]):
            bts = model.get(k) if src is r0 else None
            share = f"{100.0 * bts / (ms * 1e-3) / HBM:12.1f}" if bts and ms > 0 else f"{'':>12}"
            log.say(f"    {k:<16}{ms:10.4f}{launches:10d}{(bts or 0) / 1e6:10.1f} {share}")
    log.say(f"DECAY: one build at step 0 (everything in the air), then nh_step(1) + nh_query_refit per step; {a.queries:,} incoherent closest-hit rays and "
            f"{a.queries:,} unbounded nh_closest queries (uniform in the scene's bounds), refitted tree / fresh build of the same state")
    log.say(f"{'step':>6}{'rays refit ms':>15}{'fresh ms':>10}{'rate x':>8}{'closest refit ms':>18}{'fresh ms':>10}{'rate x':>8}{'refit ms':>10}{'hits':>7}{'2048 + 2048 records':>22}")
    for r in decay["rows"]:
        assert r["same_bytes"], f"step {r['step']}: the refitted tree and the fresh build answer differently"
        log.say(f"{r['step']:6d}{r['rays_refit_ms']:15.3f}{r['rays_fresh_ms']:10.3f}{r['rays_fresh_ms'] / r['rays_refit_ms']:8.2f}{r['closest_refit_ms']:18.3f}"
                f"{r['closest_fresh_ms']:10.3f}{r['closest_fresh_ms'] / r['closest_refit_ms']:8.2f}{r['refit_ms']:10.4f}{100 * r['hit_share_refit']:6.1f}%{'identical':>22}")
    log.say("(rate x: the refitted tree's query rate as a multiple of the fresh build's)")
    log.say(json.dumps(dict(new=new, parent=old, decay=decay)))
    log.write(a.out)


if __name__ == "__main__":
    main()
