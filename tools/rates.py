"""What the tools/*_rates.py share: the landed config-2 world, the timing procedures, the transfers, the log, and the workloads more than one tool times.
Plain functions and two small classes (Landed, Log); a tool keeps its own main(), its own table and whatever only it needs.

    import rates                                 (first: puts the tree and tests/ on sys.path)
    OTHER = rates.other_library()                (only the tools that time a second build; BEFORE the engine is imported)
    from nudge_amd import engine as E

The timing procedures (a tool's first lines say which it uses); each leaves the differing bits of today's tools -- warm-up calls, which statistic -- to
its caller:

    block                one block of `reps` calls between two device events, after `warm` calls and a stream synchronize
    interleaved          `repeats` rounds over several calls, each round one block of `reps` calls of every call, between device events
    interleaved_kernels  the same rounds, timed by the library's kernel timers for one label per call (nh_enable_timing with a filter)
    blocks               `reps` blocks of `inner` calls of ONE call between device events: the list of ms per call, for a best and a median
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

NONE = 0xFFFFFFFF
RAY_FIELDS = ("origin", "max_t", "direction", "ignore_body")


# ---- bootstrap and arguments -----------------------------------------------------------------------------------------------------------------
def other_library():
    """The build NUDGE_HIP_LIBRARY names, or None -- and the variable gone.  nudge_amd.engine reads it when it is imported: popped before that, this
    process loads the tree's library first and the other build beside it (landed(..., library=...)), not the other build alone."""
    assert "nudge_amd.engine" not in sys.modules, "other_library() comes before the engine is imported"
    return os.environ.pop("NUDGE_HIP_LIBRARY", None)


def world_args(ap, out_name, side_flag="--side"):
    """--steps, --tiles, --side and --out of every rate tool.  124 tiles of side 90 are config 2; --tiles 2 --side 12 is a rehearsal of the tool itself.
    (side_flag: another name for the world's side in a tool whose --side means something else.)"""
    ap.add_argument("--steps", type=int, default=70)
    ap.add_argument("--tiles", type=int, default=124, help="tiles of the world (124: config 2; fewer for a rehearsal of the tool)")
    ap.add_argument(side_flag, dest="world_side", type=int, default=90, help="bodies along a tile's side (90: config 2)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out_name + ".log"))
    return ap


def parser(out_name, **kw):
    return world_args(argparse.ArgumentParser(), out_name, **kw)


def world_flags(a):
    """The world arguments as a child process takes them."""
    return ["--steps", str(a.steps), "--tiles", str(a.tiles), "--side", str(a.world_side)]


# ---- the world -------------------------------------------------------------------------------------------------------------------------------
class Landed:
    """The scene of grid_tiles(tiles, side) and what the tools derive from it; with `world` set, the stepped World and what is read back from it.
    `positions` and `records` are read once: they hold while the world is not stepped again."""

    def __init__(self, scene, tiles, side=90, steps=0):
        self.scene, self.slabs, self.side, self.steps = scene, tiles, side, steps
        self.bodies = len(scene["body_transforms"])                                   # body 0, which carries the slabs, included
        self.colliders = len(scene["box_tags"]) + len(scene["sphere_tags"])
        p = scene["box_transforms"]["position"][:tiles].astype(np.float64)            # the slabs are the first `tiles` boxes
        h = scene["box_data"]["size"][:tiles].astype(np.float64)
        self.lo, self.hi = (p - h).min(axis=0), (p + h).max(axis=0)
        self.world = None
        self._positions = self._records = None

    @property
    def positions(self):
        """The dynamic bodies' positions, landed: (bodies - 1, 3) float64."""
        if self._positions is None:
            self._positions = self.world.get_bodies()["transforms"]["position"][1:].astype(np.float64)
        return self._positions

    @property
    def records(self):
        """tests/hostquery_util.py's collider records of the landed world, for the brute-force spot checks."""
        if self._records is None:
            import hostquery_util as Q
            self._records = Q.records(self.world.get_bodies()["transforms"], self.scene)
        return self._records

    def pile_bounds(self):
        """The slabs' bounds raised to the highest landed body."""
        return self.lo, np.maximum(self.hi, self.positions.max(axis=0))

    @property
    def name(self):
        return world_name(self.slabs, self.side)


def world_name(tiles, side):
    """What the log's first line calls the world."""
    return "config-2" if (tiles, side) == (124, 90) else f"{tiles}-tile side-{side}"


def scene_of(a):
    """The Landed of the arguments, without a World (no GPU)."""
    from nudge_amd import scenes as S
    return Landed(S.grid_tiles(a.tiles, side=a.world_side, seed=2, lattice_cols=11), a.tiles, a.world_side, a.steps)


def landed(a, library=None, build=True, steps=None, like=None):
    """The Landed of the arguments with its World stepped --steps times (`steps` overrides) and, with `build`, nh_query_build done.
    `library`: a path -- the engine loads THAT build for this world, beside whatever it has loaded; a Landed -- its build again.
    `like`: another Landed of the same arguments, whose scene is used instead of a new one."""
    from nudge_amd import engine as E
    land = Landed(like.scene, like.slabs, like.side, like.steps) if like is not None else scene_of(a)
    land.steps = a.steps if steps is None else steps
    if isinstance(library, Landed):
        E._LIB, E._LIB_PATH = library.world.L, library.library
    elif library:
        loaded = E._LIB
        E._LIB, E._LIB_PATH = None, os.path.abspath(library)
    w = E.World(land.scene, flags=E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP, max_contacts=6 * land.bodies)
    land.library = E._LIB_PATH
    if isinstance(library, Landed):
        assert w.L is library.world.L
    elif library:
        assert loaded is not None and w.L is not loaded, "the other build is the one already loaded"
    if land.steps:
        w.step(land.steps)
    w.synchronize()
    if build:
        w.query_build()
    land.world = w
    return land


def gpu_name(world):
    import torch
    return torch.cuda.get_device_name(world.dev)


# ---- timing ----------------------------------------------------------------------------------------------------------------------------------
def _events(world, fn, calls):
    import torch
    stream = torch.cuda.current_stream(world.dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(calls):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def _settle(world):
    import torch
    torch.cuda.current_stream(world.dev).synchronize()


def block(world, fn, reps, warm=1):
    """ms per call of one block of `reps` calls, after `warm` calls (scratch grows there) and a synchronize."""
    for _ in range(warm):
        fn()
    if warm:
        _settle(world)
    return _events(world, fn, reps)


def interleaved(world, fns, reps, repeats, warm=2):
    """{key: [ms per call of each of `repeats` blocks of `reps` calls]} of the calls {key: fn}, a block of each per round; `warm` calls of each first."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    _settle(world)
    times = {key: [] for key in fns}
    for _ in range(repeats):
        for key, fn in fns.items():
            times[key].append(_events(world, fn, reps))
    return times


def interleaved_kernels(fns, reps, repeats, warm=2):
    """{key: array of ms per call} like interleaved(), by the library's kernel timers: fns is {key: (world, timing label, call)}."""
    for wd, _, fn in fns.values():
        for _ in range(warm):
            fn()
        wd.synchronize()
    times = {key: [] for key in fns}
    for _ in range(repeats):
        for key, (wd, label, fn) in fns.items():
            wd.enable_timing(True, only=label)
            wd.kernel_times(reset=True)
            for _ in range(reps):
                fn()
            ms, launches = wd.kernel_times(reset=True)[label]
            wd.enable_timing(False)
            assert launches == reps, (label, launches)
            times[key].append(ms / launches)
    return {key: np.array(v) for key, v in times.items()}


def blocks(world, fn, reps, inner, warm=1):
    """[ms per call of each of `reps` blocks of `inner` calls] of one call, after `warm` calls and a synchronize."""
    for _ in range(warm):
        fn()
    if warm:
        _settle(world)
    return [_events(world, fn, inner) for _ in range(reps)]


def best_median(ts):
    return min(ts), float(np.median(ts))


def kernel_times(world, fn, reps=1, only=None):
    """{label: (ms, launches)} of `reps` calls of fn by the library's kernel timers (nh_kernel_times), summed over the calls."""
    world.enable_timing(True, only=only)
    world.kernel_times(reset=True)
    for _ in range(reps):
        fn()
    world.synchronize()
    kt = world.kernel_times(reset=True)
    world.enable_timing(False)
    return kt


def labels(world, fn):
    """{label: ms} of one more call of fn, the labels that ran."""
    return {k: round(v[0], 4) for k, v in sorted(kernel_times(world, fn).items()) if v[1]}


def count_then_list(world, records, qt, n, size, reps, inner, breakdown=True, keep=False):
    """A list call two ways (tools/region_rates.py's method): count only, and count + exactly sized list of `size`-byte records -- (best, median) ms per
    call of `reps` blocks of `inner` calls after one warm-up of the pair; the labels of one more pair where `breakdown`.  `records` is the bound
    *_records call of `world`; with `keep` the offsets and records come back as bytes too."""
    import torch
    dev = world.dev
    ot = torch.empty(n + 1, dtype=torch.int32, device=dev)
    records(qt, offsets=ot)
    total = total_of(ot)
    ht = torch.empty((max(total, 1), size), dtype=torch.uint8, device=dev)
    fns = (lambda: records(qt, offsets=ot), lambda: (records(qt, offsets=ot), records(qt, offsets=ot, hits=ht, capacity=total)))
    fns[1]()                                                          # warm-up: the scratch grows here
    _settle(world)
    (count, count_median), (lst, list_median) = (best_median(blocks(world, fn, reps, inner, warm=0)) for fn in fns)
    out = dict(records=total, count_ms=count, list_ms=lst, count_median_ms=count_median, list_median_ms=list_median, labels=labels(world, fns[1]) if breakdown else {})
    return out, ((ot.cpu().numpy().tobytes(), ht[:total].cpu().numpy().tobytes()) if keep else None)


def spread(v):
    return dict(ms=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def spreads(times):
    return {key: spread(v) for key, v in times.items()}


def fmt(v):
    return f"{v['ms']:.3f} ({v['min']:.3f} .. {v['max']:.3f})"


def fmt_best(v):
    return f"{v['min']:.3f} best, {v['ms']:.3f} ({v['min']:.3f} .. {v['max']:.3f})"


def beside_parent(log, worlds, calls, n, reps, repeats):
    """The plain calls (name, timing label, records, result size, call(world, records, results)) on this library's world and on the parent's loaded
    twice, interleaved: per block this / parent, and parent again / parent.  {name: the row of the JSON line}."""
    import torch
    med, out = spread, {}
    w = worlds["this"]
    for name, label, records, size, call in calls:
        ins = {k: upload(wd, records) for k, wd in worlds.items()}
        outs = {k: torch.empty((n, size), dtype=torch.uint8, device=w.dev) for k in worlds}
        per_block = interleaved_kernels({k: (wd, label, (lambda k=k, wd=wd: call(wd, ins[k], outs[k]))) for k, wd in worlds.items()}, reps, repeats)
        assert torch.equal(outs["this"], outs["parent"]) and torch.equal(outs["again"], outs["parent"]), f"nh_{name}: the libraries differ"
        this, parent, again = (per_block[k] for k in ("this", "parent", "again"))
        r_this, r_self = this / parent, again / parent
        inside = bool(r_self.min() <= np.median(r_this) <= r_self.max())
        pad = 1 + max(len(c[0]) for c in calls)
        log.say(f"  nh_{name:<{pad}} this {fmt(med(this))} ms   parent {fmt(med(parent))} ms   this / parent {np.median(r_this):.3f} ({r_this.min():.3f} .. {r_this.max():.3f})"
                f"   parent / parent {np.median(r_self):.3f} ({r_self.min():.3f} .. {r_self.max():.3f})   {'inside' if inside else 'OUTSIDE'} the parent's own spread")
        out[name] = dict(this=med(this), parent=med(parent), again=med(again), this_over_parent=med(r_this), parent_over_parent=med(r_self), inside=inside)
    return out


# ---- transfers and the log -------------------------------------------------------------------------------------------------------------------
def upload(world, array):
    """The array's bytes as a uint8 tensor on the world's device."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).copy()).to(world.dev)


def download(tensor, dtype):
    return np.frombuffer(tensor.cpu().numpy().tobytes(), dtype=dtype).copy()


def total_of(offsets):
    """The total of a list call's offsets (their last word, unsigned)."""
    return int(offsets[-1].item()) & NONE


def spot(n, size=258, seed=3):
    """`size` sorted distinct indices below n for a brute-force spot check; all n of them where n < size."""
    return np.sort(np.random.default_rng(seed).choice(n, size=min(size, n), replace=False))


class Log:
    def __init__(self):
        self.lines = []

    def say(self, s=""):
        print(s, flush=True)
        self.lines.append(s)

    def text(self):
        return "\n".join(self.lines) + "\n"

    def write(self, path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(self.text())


# ---- workloads more than one tool times (numpy alone: a seed or generator, a count, bounds or positions) --------------------------------------
def unit_rows(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def ray_sets(rng, n, lo, hi):
    """tools/query_rates.py's rays (nh_Ray records, max_t inf, nobody ignored): `incoherent` -- origins uniform in [lo, hi + 60 up], directions uniform
    on the sphere -- and `coherent` -- a grid of min(1024, n) columns over the bounds at y = 30, straight down.  Any-hit uses the incoherent set."""
    from nudge_amd import engine as E
    r = np.zeros(n, dtype=E.RAY)
    r["max_t"], r["ignore_body"] = np.inf, NONE
    r["origin"] = rng.uniform(lo, hi + np.array([0, 60, 0]), size=(n, 3))
    r["direction"] = unit_rows(rng.normal(size=(n, 3)))
    incoherent = r.copy()
    side = min(1024, n)
    assert n % side == 0, "the coherent grid wants a multiple of 1024 rays"
    gx, gz = np.meshgrid(np.linspace(lo[0], hi[0], side), np.linspace(lo[2], hi[2], n // side))
    r["origin"][:, 0], r["origin"][:, 1], r["origin"][:, 2] = gx.reshape(-1), 30.0, gz.reshape(-1)
    r["direction"] = (0.0, -1.0, 0.0)
    return incoherent, r


def random_rotations(n, seed=2):
    """The casts' random rotations: (n, 4) float32 unit quaternions."""
    return unit_rows(np.random.default_rng(seed).normal(size=(n, 4))).astype(np.float32)


def cast_records(rays, dtype, rotation=None, **fields):
    """Cast records of `dtype` along the rays: `fields` (radius, size, half_height) set, `rotation` the identity where the record has one and None is given."""
    c = np.zeros(len(rays), dtype=dtype)
    for k in RAY_FIELDS:
        c[k] = rays[k]
    for k, v in fields.items():
        c[k] = v
    if "rotation" in dtype.names:
        c["rotation"] = (0.0, 0.0, 0.0, 1.0) if rotation is None else rotation
    return c


def point_sets(rng, n, live, lo, hi, above_first=False):
    """tools/closest_rates.py's three: [(name, (n, 3) float64 points, max_distance)] -- near random bodies (max 2), uniform in [lo, hi] (inf), 20 above
    the highest body (inf).  above_first: the third set's draw comes before the other two (tools/distance_rates.py's order of draws)."""
    def over():
        p = rng.uniform(lo, hi, size=(n, 3))
        p[:, 1] = live[:, 1].max() + 20.0
        return p
    above = over() if above_first else None
    near = live[rng.integers(0, len(live), size=n)] + rng.normal(scale=0.5, size=(n, 3))
    uniform = rng.uniform(lo, hi, size=(n, 3))
    above = over() if above is None else above
    return [("near bodies, max 2", near, 2.0), ("uniform in bounds, inf", uniform, np.inf), ("20 m above the pile, inf", above, np.inf)]


def point_queries(points, max_distance):
    from nudge_amd import engine as E
    q = np.zeros(len(points), dtype=E.POINT_QUERY)
    q["point"], q["max_distance"], q["ignore_body"] = points, max_distance, NONE
    return q


def overlap_queries(centres, size, shape, rotation=(0.0, 0.0, 0.0, 1.0), ignore_body=NONE):
    """nh_OverlapQuery records: `size` is (n, 3) or broadcasts to it."""
    from nudge_amd import engine as E
    q = np.zeros(len(centres), dtype=E.OVERLAP_QUERY)
    q["center"], q["size"], q["shape"], q["rotation"], q["ignore_body"] = centres, size, shape, rotation, ignore_body
    return q


def spheres_on_bodies(rng, n, positions, radius=1.0):
    """tools/overlap_rates.py's first set: spheres of about a box's size centred on random bodies."""
    from nudge_amd import engine as E
    centres = positions[rng.integers(0, len(positions), size=n)] + rng.normal(scale=0.25, size=(n, 3))
    return overlap_queries(centres, (radius, 0.0, 0.0), E.NH_SHAPE_SPHERE)


def box_planes(lo, hi):
    """tools/region_rates.py's cubes and world region: the six planes of the axis-aligned boxes [lo, hi] ((n, 3) each), as (n, 6, 4) float32."""
    lo, hi = np.atleast_2d(lo), np.atleast_2d(hi)
    out = np.zeros((len(lo), 6, 4), dtype=np.float32)
    for k in range(3):
        out[:, 2 * k, k], out[:, 2 * k, 3] = 1.0, -lo[:, k]
        out[:, 2 * k + 1, k], out[:, 2 * k + 1, 3] = -1.0, hi[:, k]
    return out


def reach_bounds(rec):
    """The world's AABB from the collider records, one unit wider than every collider's bounding ball reaches."""
    reach = np.linalg.norm(rec["h"].astype(np.float64), axis=1, keepdims=True)
    return (rec["p"] - reach).min(axis=0) - 1.0, (rec["p"] + reach).max(axis=0) + 1.0


def tile_size(scene, body_positions):
    """The larger horizontal extent of tile 0's bodies (body_positions: every body's, body 0 included)."""
    tp = np.asarray(body_positions)[np.nonzero(np.asarray(scene["tile_of_body"]) == 0)[0]].astype(np.float64)
    return float((tp.max(axis=0) - tp.min(axis=0))[[0, 2]].max())


def move_batch(rng, n, positions):
    """tools/move_rates.py's batch: origins 2.2 - 3 above random bodies' centres, displacements of 0.75 - 3 units that lean downwards."""
    at = rng.integers(0, len(positions), size=n)
    o = positions[at] + np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(2.2, 3.0, n), rng.uniform(-0.5, 0.5, n)], axis=1)
    d = rng.normal(size=(n, 3))
    d[:, 1] = -np.abs(d[:, 1]) - 0.5
    d *= rng.uniform(0.75, 3.0, size=(n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    return o, d


def walk_batch(rng, n, rec, tops):
    """tools/walk_rates.py's batch: (x, top, z, displacement) -- half stand on the slab 1.3 - 2.2 beside a random dynamic collider and head for it, half
    stand on such a collider's top and head anywhere; 0.5 - 2 units, horizontal.  `tops`: every collider's top (tests/walk_batches.py _tops)."""
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
    return x, top, z, np.stack([np.cos(head) * length, np.zeros(n), np.sin(head) * length], axis=1)
