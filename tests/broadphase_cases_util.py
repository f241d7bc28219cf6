"""Crafted worlds for the broadphase of nudge_amd/csrc/nh_collide.hip (k_xform's containment test and stamps, k_grid_setup, k_cell_keys, k_find_pairs, k_large_pairs,
k_reinsert, k_kept_filter, the host's switch to the DIRECT search), shared by tests/test_cpu_broadphase_cases.py (oracles and the trigger model, no GPU) and
tests/test_gpu_broadphase_cases.py.  The oracle is brute force: tests/hostsim's hs_collide / hs_pairs (O(n^2), no grid, no kept list), and the compiled reference
where it can hold the world.

A world is a scene (the keys of nudge_amd.scenes._assemble) plus scene["bp"] = dict(kind="grid" | "kept", oracle, world={E.World keywords}, phases=[...]); oracle is "ref" (hostsim, proven
equal to the reference on this world by the CPU test), "host" (hostsim; too large for the reference), "list" (pairs known by construction) or "ref_only".  Every movable collider sits on a dynamic body of its own with an identity local transform, so a phase places it with set_bodies(transforms=...);
momenta are zero, idle counters 0 (sleeper_edge: 0xff for its cluster), only collide() is called.  A phase is dict(name, transforms (all bodies), edits
[(box index, new half extents)], expect=(rebuilds, inserts) -- the deltas of counts()["broadphase_rebuilds"] / ["broadphase_inserts"] its collide() must show in
the DEFAULT world --, large (counts()["large_colliders"], where it matters, else None), pairs_in / pairs_out (collider index pairs that must / must not be among
the overlapping pairs), trigger (fallbacks: the one reason for its rebuild)).  Coordinates and half extents are dyadic wherever an edge is to be hit, so the
float32 AABBs are the intended numbers; ulp steps are taken on the float32 values.

GRID worlds (one collide(); the default world builds its grid from boxes inflated by the margin -- 0.05 at a world's first call, 1/32 of the last grid's cell
afterwards --, the no_kept_pairs world from the exact boxes, so size classes and cells differ between the two on purpose):
  all_large_64 / _65   64 colliders of mixed size and shape: within the budget max(64, C / 1024), all "large", k_large_pairs and the large x large loop do all the
                       work; and the same with a 65th, by far the smallest, collider: the only grid member.
  size_ladder_64 / _65 ~2000 boxes and spheres, extents 2^k (1, 1.25, 1.5, 1.75) and one ulp below each over 16 quarter-octave classes, rotated boxes, slabs across
                       many cells; exactly 64 / 65 colliders in the classes from [4, 5) up, so the split falls on a class edge: 64 large, or 49 with the cell 5.
  cell_edges           cubes of extent 7/8 (class [7/8, 1): cell 1, origin (0, 0, 0) -- the exact min corner of the lowest cube, the split having "moved" at a first
                       call) with min corners at origin + k cell and one ulp either side; the neighbour touches exactly (face against face: NO pair under the strict
                       test), overlaps by one ulp, or stands two or three cells off; a partner in each of the 26 neighbouring cells; pairs on the lowest and the highest
                       cell of every axis.
  sparse_far           clusters of extent ~0.01 spread over 1000 units -- the 2^16-entry table is too small, the cell doubles many times -- and one cluster near 1e4
                       whose radii are below the ulp of its position: AABBs of zero extent.
  dense_cell           200 spheres, one body each, with the same AABB min corner (Morton ties) and radii of one size class: 19,900 pairs out of one cell.
  compound_static      bodies with several mutually overlapping colliders (no pair), mutually overlapping colliders of body 0 (no pair) that dynamic ones overlap.
  lane_split_16384 / _16385   isolated cubes and a few hundred designated overlapping pairs either side of the host's `many_lanes` (16 lanes per collider or one);
                       hostsim is the oracle (the reference holds 8192 colliders).
KEPT-LIST worlds (base: 16 x 8 x 16 cubes of extent 7/8 that touch their x neighbours face to face -- kept pairs that never overlap, which also keeps the filter
from writing in place, so that raw_pairs counts overlapping pairs --, a static slab under them, two dynamic walls, eight movers resting on the top layer; cell 1,
margin 1/32 after the first rebuild; the first collide() rebuilds):
  wiggle, one_leaver, leavers_meet, stamp_wear, fallbacks, fallbacks_kept (max_pairs 2048: the 7/8 rule), fallbacks_combos (16,400 colliders), fallbacks_esc
  (67,543 colliders: pairs known by construction), direct_and_back, sleeper_edge (reference only here: hostsim models no sleeping; the numpy oracle for islands and sleeping is tests/island_cases_util.islands) -- see each builder.

What the clauses of k_grid_setup allow (asserted by `check_trigger`): moved >= leavers always (a first-time leaver joins the moved list in the same pass), so
"leavers x 16 > C" implies "moved x 32 > C" and can never be the only clause that holds; and more than NH_ESC_MAX leavers imply moved x 32 > C below 131,104
colliders and leavers x (moved + large) > 16 C below 1,049,089: at fallbacks_esc's size the overflow is shown together with those two, clause "leavers x 16 > C" off.

Left out: NH_MOVED_MAX (16384) cannot be reached below 524,288 colliders and stays with the at-size tests; NaN poses; k_reinsert in a still step (movers form),
which tests/test_gpu_still.py covers."""
import numpy as np

from nudge_amd import scenes as S

F = np.float32
H = 0.4375                       # half extent of the base cube: extent 7/8, the size class whose upper edge is 1
ESC_MAX, MOVED_MAX = 4096, 16384
GRID = ["all_large_64", "all_large_65", "size_ladder_64", "size_ladder_65", "cell_edges", "sparse_far", "dense_cell", "compound_static", "lane_split_16384",
        "lane_split_16385"]
KEPT = ["wiggle", "one_leaver", "leavers_meet", "stamp_wear", "fallbacks", "fallbacks_kept", "fallbacks_combos", "fallbacks_esc", "direct_and_back", "sleeper_edge"]
CASES = GRID + KEPT
REF_LIMIT = 8192


def _quat(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([a * np.sin(angle / 2.0), [np.cos(angle / 2.0)]])


class _Builder:
    """Bodies (0: the static world at the origin), boxes and spheres; a handle is ("b" | "s", k) until freeze(), a collider index afterwards (idx)."""

    def __init__(self):
        self.body_pos, self.body_rot, self.idle = [np.zeros(3, F)], [np.array([0, 0, 0, 1], F)], [0]
        self.boxes, self.spheres = [], []          # (body, local position, local rotation, half extents) / (body, local position, radius)
        self.nbox = None

    def body(self, pos, rot=(0, 0, 0, 1), idle=0):
        q = np.asarray(rot, dtype=np.float64)
        self.body_pos.append(np.asarray(pos, dtype=np.float64).astype(F)); self.body_rot.append((q / np.linalg.norm(q)).astype(F)); self.idle.append(idle)
        return len(self.body_pos) - 1

    def box(self, pos, size, rot=(0, 0, 0, 1), body=None, idle=0):
        """A box at world position `pos`: on a new dynamic body (the body carries the pose), on body 0, or at local `pos` on the dynamic body `body`."""
        if body is None:
            self.boxes.append((self.body(pos, rot, idle), np.zeros(3, F), np.array([0, 0, 0, 1], F), np.asarray(size, dtype=np.float64).astype(F)))
        else:
            q = np.asarray(rot, dtype=np.float64)
            self.boxes.append((body, np.asarray(pos, dtype=np.float64).astype(F), (q / np.linalg.norm(q)).astype(F), np.asarray(size, dtype=np.float64).astype(F)))
        return ("b", len(self.boxes) - 1)

    def sphere(self, pos, radius, body=None, idle=0):
        if body is None:
            self.spheres.append((self.body(pos, idle=idle), np.zeros(3, F), F(radius)))
        else:
            self.spheres.append((body, np.asarray(pos, dtype=np.float64).astype(F), F(radius)))
        return ("s", len(self.spheres) - 1)

    def freeze(self):
        self.nbox = len(self.boxes)

    def idx(self, h):
        return h[1] if h[0] == "b" else self.nbox + h[1]

    def body_of(self, h):
        return (self.boxes if h[0] == "b" else self.spheres)[h[1]][0]

    def scene(self, name, kind, oracle, phases, world=None):
        nb, nbox, nsph = len(self.body_pos), len(self.boxes), len(self.spheres)
        bt = S._identity_transforms(nb)
        bt["position"] = np.array(self.body_pos, dtype=F); bt["rotation"] = np.array(self.body_rot, dtype=F)
        props = np.zeros(nb, dtype=S.PROPERTIES)
        props["mass_inverse"][1:] = 1.0; props["inertia_inverse"][1:] = 1.0
        xt, st = S._identity_transforms(nbox), S._identity_transforms(nsph)
        xd, sd = np.zeros(nbox, dtype=S.BOX), np.zeros(nsph, dtype=S.SPHERE)
        for k, (body, lp, lq, size) in enumerate(self.boxes):
            xt["body"][k] = body; xt["position"][k] = lp; xt["rotation"][k] = lq; xd["size"][k] = size
        for k, (body, lp, r) in enumerate(self.spheres):
            st["body"][k] = body; st["position"][k] = lp; sd["radius"][k] = r
        return dict(name=f"broadphase_{name}", body_transforms=bt, body_properties=props, body_momentum=np.zeros(nb, dtype=S.MOMENTUM),
                    idle_counters=np.array(self.idle, dtype=np.uint8), box_tags=np.arange(nbox, dtype=np.uint32), box_data=xd, box_transforms=xt,
                    sphere_tags=np.arange(nbox, nbox + nsph, dtype=np.uint32), sphere_data=sd, sphere_transforms=st, params=dict(S.DEFAULT_PARAMS),
                    bp=dict(kind=kind, oracle=oracle, world=dict(world or {}), phases=phases))


class _Script:
    def __init__(self, b):
        b.freeze()
        self.b, self.phases = b, []
        self.pos = np.array(b.body_pos, dtype=F)
        self.rot = np.array(b.body_rot, dtype=F)

    def phase(self, name, moves=(), expect=(0, 0), large=None, pairs_in=(), pairs_out=(), edits=(), trigger=None):
        """`moves`: (handle, new centre) of colliders that sit alone on their dynamic body; they last."""
        b = self.b
        for h, p in moves:
            self.pos[b.body_of(h)] = np.asarray(p, dtype=np.float64).astype(F)
        t = S._identity_transforms(len(self.pos))
        t["position"] = self.pos; t["rotation"] = self.rot
        pr = lambda prs: [tuple(sorted((b.idx(x), b.idx(y)))) for x, y in prs]
        self.phases.append(dict(name=name, transforms=t, expect=tuple(expect), large=large, pairs_in=pr(pairs_in), pairs_out=pr(pairs_out),
                                edits=[(b.idx(h), np.asarray(s, dtype=F)) for h, s in edits], trigger=trigger))
        return self


def scene_at(scene, upto):
    """The scene with the collider edits of phases 0 .. upto applied (copies only what it changes)."""
    edits = [e for ph in scene["bp"]["phases"][:upto + 1] for e in ph["edits"]]
    if not edits:
        return scene
    out = dict(scene)
    out["box_data"] = scene["box_data"].copy()
    for i, size in edits:
        out["box_data"]["size"][i] = size
    return out


def _centre(target, h, how="eq"):
    """A float32 centre c of a box of half extent h whose min corner float32(c - h) equals `target` ("eq"; None where no centre does), or is the nearest
    attainable value below / above it."""
    target, h = F(target), F(h)
    c0 = F(target + h)
    cands = sorted({float(_ulps(c0, k)) for k in range(-6, 7)})
    mins = [(F(F(c) - h), F(c)) for c in cands]
    if how == "eq":
        hit = [c for m, c in mins if m == target]
        return hit[0] if hit else None
    if how == "below":
        return max(c for m, c in mins if m < target)
    return min(c for m, c in mins if m > target)


def _ulps(x, k):
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


# ---- grid worlds ----------------------------------------------------------------------------------------------------------------------------------------------
def _all_large(b, n):
    sizes = [0.25, 0.75, 1.5, 0.375, 3.0, 0.5, 1.0]
    hs = []
    for i in range(64):
        s = sizes[i % len(sizes)]
        pos = (1.0 * i, 0.5 * (i % 3), 0.25 * (i % 5))
        if i % 2 == 0:
            hs.append(b.box(pos, (s, 0.5 * s + 0.125, s), rot=_quat((1, 2, 3), 0.3 * i) if i % 4 == 0 else (0, 0, 0, 1)))
        elif i % 11 == 1:
            hs.append(b.sphere(pos, s, body=0))          # (on the static body)
        else:
            hs.append(b.sphere(pos, s))
    if n == 65:
        hs.append(b.sphere((10.0, 0.25, 0.25), 1.0 / 64.0))
    return _Script(b).phase("only", expect=(1, 0), large=64).phases


def _size_ladder(b, n):
    rng = np.random.default_rng(41)
    exts = []
    for k in (-2, -1, 0, 1):
        for q in range(4):
            e = F(2.0 ** k * (1.0 + 0.25 * q))
            exts += [e, _ulps(e, -1)]

    def place():
        return np.round(rng.uniform((0.0, 0.5, 0.0), (40.0, 6.0, 40.0)) * 64.0) / 64.0

    for i in range(1900):
        half = F(exts[i % len(exts)] * F(0.5))
        kind = i % 5
        if kind == 0:
            b.sphere(place(), half)
        elif kind == 1:          # rotated: the AABB is larger than the box, by a factor that depends on the turn
            b.box(place(), (half * F(0.375), half * F(0.25), half * F(0.375)), rot=_quat(rng.normal(size=3), rng.uniform(0.2, 2.9)))
        else:
            b.box(place(), (half, half * F(0.5) if kind == 2 else half, half))
    # the top classes: 15 colliders each of extent 4, 5, 6 and 7, four slabs -- 64 -- and for n == 65 a sixteenth of extent 4
    for e in (4.0, 5.0, 6.0, 7.0):
        for i in range(15 + (1 if (n == 65 and e == 4.0) else 0)):
            if i % 2:
                b.sphere(place(), e / 2)
            else:
                b.box(place(), (e / 2, e / 4, e / 2))
    b.box((20.0, -0.25, 20.0), (21.0, 0.5, 21.0), body=0)
    b.box((20.0, 3.0, -0.5), (21.0, 4.0, 0.5), body=0)
    b.box((-0.5, 3.0, 20.0), (0.5, 4.0, 21.0))
    b.box((20.0, 6.5, 20.0), (20.0, 0.25, 0.5), rot=_quat((0, 1, 0), 0.7))
    return _Script(b).phase("only", expect=(1, 0), large=64 if n == 64 else 49).phases


def _cell_edges(b):
    """origin = (0, 0, 0), cell = 1: k_grid_setup takes the origin from the exact min corners at a world's first call (last call's split, none, has "moved") and the
    cell from the upper edge of the size class of extent 7/8 (+ 0.1 in the default world): [7/8, 1) -> 1.  Family n stands at (10 (n % 6), 10 (n // 6), 2) and runs
    along its axis from cell k on."""
    print("cell_edges: grid origin (0, 0, 0), cell 1")
    ins, outs = [], []

    def cube_at(centre):
        return b.box(centre, (H, H, H))

    def cube(mins):
        return cube_at([_centre(m, H) for m in mins])

    n = 0
    for axis in range(3):
        for d in (-1, 0, 1):
            for gap in ("touch", "overlap", "two", "three"):
                base = np.array([10.0 * (n % 6), 10.0 * (n // 6), 2.0])
                k = n % 6
                if d < 0 and base[axis] + k == 0.0:
                    k = 1
                edge = F(base[axis] + k)
                for step in range(4):          # (a centre one ulp further where no partner's min corner can equal this max corner exactly)
                    ca = [_centre(m, H) for m in base.astype(F)]
                    ca[axis] = _centre(edge, H) if d == 0 else _ulps(_centre(edge, H, "below" if d < 0 else "above"), d * step)
                    amin, amax = F(ca[axis] - F(H)), F(ca[axis] + F(H))
                    cb = list(ca)
                    cb[axis] = {"touch": _centre(amax, H), "overlap": _centre(amax, H, "below"), "two": _centre(F(amin + F(2.0)), H, "above"),
                                "three": _centre(F(amin + F(3.0)), H, "above")}[gap]
                    if cb[axis] is not None:
                        break
                assert cb[axis] is not None and (d == 0) == (amin == edge) and (d >= 0 or amin < edge) and (d <= 0 or amin > edge), (n, axis, d, gap)
                (ins if gap == "overlap" else outs).append((cube_at(ca), cube_at(cb)))
                n += 1
    # the 26 neighbouring cells: a cube in the middle of cell (cx, cy, cz) and a partner whose min corner lies 3/4 of a cell off along every combination of axes --
    # in the cell before (a search that looks forward only must find it from the partner's side) or after
    n = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dx, dy, dz) != (0, 0, 0):
                    mins = np.array([1.5 + 4.0 * (n % 13), 4.5 + 4.0 * (n // 13), 6.5])
                    ins.append((cube(mins), cube(mins + 0.75 * np.array([dx, dy, dz]))))
                    n += 1
    # the lowest and the highest cell of every axis
    ins.append((cube((0.0, 0.0, 0.0)), cube((0.5, 0.5, 0.5))))
    ins.append((cube((60.0, 60.0, 10.0)), cube((59.5, 59.5, 9.5))))
    for mins in ((60.0, 0.0, 0.0), (0.0, 60.0, 0.0), (0.0, 0.0, 10.0)):
        ins.append((cube(mins), cube([m + 0.5 if m == 0.0 else m - 0.5 for m in mins])))
    return _Script(b).phase("only", expect=(1, 0), pairs_in=ins, pairs_out=outs).phases


def _sparse_far(b):
    rng = np.random.default_rng(43)
    centres = [(0.0, 0.0, 0.0), (1000.0, 0.0, 0.0), (0.0, 1000.0, 0.0), (0.0, 0.0, 1000.0), (500.0, 500.0, 500.0), (1000.0, 1000.0, 1000.0), (250.0, 750.0, 125.0)]
    for c in centres:
        for i in range(40):
            p = np.asarray(c) + np.round(rng.uniform(0.0, 0.05, size=3) * 4096.0) / 4096.0
            if i % 3:
                b.sphere(p, 0.005)
            else:
                b.box(p, (0.005, 0.00375, 0.005))
    # near 1e4 the ulp is 2^-10: a radius of 1e-4 vanishes, the AABB has zero extent; one sphere large enough to have a box holds them
    pts = [b.sphere((1e4 + i / 1024.0, 1e4, 1e4 + (i % 3) / 1024.0), 1e-4) for i in range(12)]
    big = b.sphere((1e4 + 6 / 1024.0, 1e4, 1e4 + 1 / 1024.0), 0.0078125)
    return _Script(b).phase("only", expect=(1, 0), pairs_in=[(big, p) for p in pts], pairs_out=[(pts[0], pts[3]), (pts[1], pts[2])]).phases


def _dense_cell(b):
    hs = []
    for i in range(200):
        r = F(0.5 + i / 4096.0)
        hs.append(b.sphere((F(1.0) + r, F(1.0) + r, F(1.0) + r), r))
    return _Script(b).phase("only", expect=(1, 0), pairs_in=[(hs[0], hs[199]), (hs[7], hs[8])]).phases


def _compound_static(b):
    ins, outs = [], []
    # body 0: mutually overlapping boxes and spheres
    st = [b.box((2.0 * i, 0.0, 0.0), (1.5, 0.5, 1.5), body=0) for i in range(8)] + [b.sphere((2.0 * i + 1.0, 0.25, 0.0), 1.0, body=0) for i in range(8)]
    outs += [(st[0], st[1]), (st[0], st[8]), (st[8], st[9])]
    for i in range(24):
        body = b.body((0.625 * i, 0.625 + 0.125 * (i % 3), 0.25 * (i % 4) - 0.5), rot=_quat((0, 1, 0), 0.2 * i))
        c0 = b.box((0.0, 0.0, 0.0), (0.25, 0.25, 0.25), body=body)
        c1 = b.sphere((0.125, 0.125, 0.0), 0.25, body=body)
        c2 = b.box((-0.125, 0.0, 0.125), (0.125, 0.375, 0.125), rot=_quat((1, 0, 0), 0.5), body=body)
        outs += [(c0, c1), (c0, c2), (c1, c2)]
        if i == 0:
            ins += [(c0, st[0])]
    # (free-standing compounds above the rest)
    for i in range(8):
        body = b.body((3.0 * i, 6.0, 0.0))
        outs.append((b.sphere((0.0, 0.0, 0.0), 0.5, body=body), b.sphere((0.25, 0.0, 0.0), 0.5, body=body)))
    return _Script(b).phase("only", expect=(1, 0), pairs_in=ins, pairs_out=outs).phases


def _lane_split(b, n):
    ins = []
    lattice = 16384 - 2 * 300 if n == 16384 else 16385 - 2 * 300
    side = 26
    assert side ** 3 >= lattice
    k = 0
    for z in range(side):
        for y in range(side):
            for x in range(side):
                if k < lattice:
                    b.box((2.0 * x + H, 2.0 * y + H, 2.0 * z + H), (H, H, H)); k += 1
    # the designated pairs: beside the lattice, two cells from everybody else
    for i in range(300):
        p = np.array([2.0 * (i % 20), 2.0 * (i // 20), 2.0 * side + 2.0])
        a = b.box(p + H, (H, H, H))
        c = b.sphere(p + H + (0.5, 0.25, 0.5), H) if i % 2 else b.box(p + H + (0.25, 0.5, 0.75), (H, H, H))
        ins.append((a, c))
    return _Script(b).phase("only", expect=(1, 0), pairs_in=ins).phases


# ---- the base of the kept-list worlds ----------------------------------------------------------------------------------------------------------------------------
class _Base:
    def __init__(self, b, nx=16, ny=8, nz=16, movers=8, pitch=(0.875, 2.0, 2.0), slab_top=1.0 / 64.0):
        self.b, self.n, self.pitch = b, (nx, ny, nz), pitch
        self.cube = {}
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    self.cube[i, j, k] = b.box(self.cube_min(i, j, k) + H, (H, H, H))
        px, py, pz = pitch
        self.slab = b.box((px * nx / 2.0, slab_top - 0.5, pz * nz / 2.0), (px * nx / 2.0 + 1.0, 0.5, pz * nz / 2.0 + 1.0), body=0)
        self.wall = [b.box((-3.0, 4.5, 8.0), (0.5, 4.0, 8.0)), b.box((-6.0, 4.5, 8.0), (0.5, 4.0, 8.0))]
        # mover n rests on cubes (2n, top, 2n) and (2n + 1, top, 2n): its home
        self.mover = [b.box(self.home(n), (H, H, H)) for n in range(movers)]

    def cube_min(self, i, j, k):
        return np.array([self.pitch[0] * i, self.pitch[1] * j, self.pitch[2] * k])

    def home(self, n):
        return self.cube_min(2 * n, self.n[1] - 1, 2 * n) + 0.5 + H

    def home_pairs(self, n):
        top = self.n[1] - 1
        return [(self.mover[n], self.cube[2 * n, top, 2 * n]), (self.mover[n], self.cube[2 * n + 1, top, 2 * n])]

    def on(self, i, j, k):
        """Centre of a cube that rests on cubes (i, j, k) and (i + 1, j, k) as a mover rests on its home."""
        return self.cube_min(i, j, k) + 0.5 + H

    def free(self, x, j, k):
        """Centre of a cube in the empty space between the layers: min corner (x, 2 j + 1, 2 k + 1) touches nobody, inflated or not."""
        return np.array([x, 2.0 * j + 1.0, 2.0 * k + 1.0]) + H

    def shifted(self, i, j, k, dy=0.25):
        return self.cube_min(i, j, k) + H + (0.0, dy, 0.0)


def _wiggle(b):
    base = _Base(b)
    s = _Script(b).phase("first", expect=(1, 0))
    c, left, right = base.cube[3, 2, 3], base.cube[2, 2, 3], base.cube[4, 2, 3]
    home = base.cube_min(3, 2, 3) + H
    d = 1.0 / 128.0
    s.phase("small moves", moves=[(base.cube[i, 4, 5], base.cube_min(i, 4, 5) + H + (0.0, d, -d)) for i in range(0, 16, 3)] + [(base.mover[2], base.home(2) + (d, d, d))],
            pairs_out=[(c, left), (c, right)])
    s.phase("touching neighbours now overlap", moves=[(c, home + (d, 0.0, 0.0))], pairs_in=[(c, right)], pairs_out=[(c, left)])
    s.phase("the overlap ends", moves=[(c, home)], pairs_out=[(c, right), (c, left)])
    s.phase("the other neighbour", moves=[(c, home - (d, 0.0, 0.0))], pairs_in=[(c, left)], pairs_out=[(c, right)])
    s.phase("a large collider inside its box", moves=[(base.wall[0], np.array([-3.0, 4.5, 8.0]) + (d, -d, d))])
    return s.phases


def _one_leaver(b):
    base = _Base(b)
    m, m1 = base.mover[0], base.mover[1]
    s = _Script(b).phase("first", expect=(1, 0), pairs_in=base.home_pairs(0), large=3)
    s.phase("to empty space", moves=[(m, base.free(3.0, 2, 3))], expect=(0, 1), pairs_out=base.home_pairs(0))
    s.phase("onto unmoved neighbours", moves=[(m, base.on(5, 3, 5))], expect=(0, 1), pairs_in=[(m, base.cube[5, 3, 5]), (m, base.cube[6, 3, 5])])
    s.phase("onto the static slab", moves=[(m, np.array([4.0, -0.5, 21.0]) + H)], expect=(0, 1), pairs_in=[(m, base.slab)], pairs_out=[(m, base.cube[5, 3, 5])])
    s.phase("onto a dynamic wall", moves=[(m, np.array([-3.25, 3.0, 3.0]) + H)], expect=(0, 1), pairs_in=[(m, base.wall[0])], pairs_out=[(m, base.slab)])
    for name, p in (("low x", (-20.0, 5.0, 7.0)), ("high x", (40.0, 5.0, 7.0)), ("low y", (3.0, -30.0, 7.0)), ("high y", (3.0, 60.0, 7.0)), ("low z", (3.0, 5.0, -25.0)),
                    ("high z", (3.0, 5.0, 80.0))):
        s.phase("beyond the grid, " + name, moves=[(m, np.array(p) + H)], expect=(0, 1), pairs_out=[(m, base.wall[0])])
    s.phase("a second leaver joins it out there", moves=[(m1, np.array([3.5, 5.25, 80.5]) + H)], expect=(0, 1), pairs_in=[(m, m1)], pairs_out=base.home_pairs(1))
    s.phase("a thousand cells away", moves=[(m, np.array([1000.0, 1000.0, 1000.0]) + H)], expect=(0, 1), pairs_out=[(m, m1)])
    s.phase("back to exactly its old place", moves=[(m, base.home(0))], expect=(0, 1), pairs_in=base.home_pairs(0))
    return s.phases


def _leavers_meet(b):
    base = _Base(b)
    m = base.mover
    s = _Script(b).phase("first", expect=(1, 0))
    s.phase("two leavers land on each other", moves=[(m[1], base.free(3.0, 2, 3)), (m[2], base.free(3.0, 2, 3) + (0.25, 0.125, 0.5))], expect=(0, 2), pairs_in=[(m[1], m[2])])
    s.phase("a collider moves to a new place", moves=[(m[3], base.free(7.0, 4, 9))], expect=(0, 1), pairs_out=base.home_pairs(3))
    s.phase("a leaver lands on its new place", moves=[(m[4], base.free(7.0, 4, 9) + (0.5, 0.25, -0.25))], expect=(0, 1), pairs_in=[(m[3], m[4])])
    s.phase("a leaver lands on its old place", moves=[(m[5], base.home(3))], expect=(0, 1), pairs_out=[(m[5], m[3])],
            pairs_in=[(m[5], base.cube[6, 7, 6]), (m[5], base.cube[7, 7, 6])])
    s.phase("the higher index first, three at once", moves=[(m[7], base.free(9.0, 1, 2)), (m[6], base.free(9.0, 1, 2) + (0.5, 0.0, 0.0)), (m[0], base.free(9.0, 1, 2) - (0.5, 0.0, 0.25))],
            expect=(0, 3), pairs_in=[(m[6], m[7]), (m[0], m[7])], pairs_out=[(m[0], m[6])])
    return s.phases


def _stamp_wear(b):
    base = _Base(b)
    m = base.mover[0]
    there = [(m, base.cube[5, 3, 5]), (m, base.cube[6, 3, 5])]
    s = _Script(b).phase("first", expect=(1, 0), pairs_in=base.home_pairs(0))
    for hop in range(1, 131):
        away = hop % 2 == 1
        # 127 re-insertions wear the 7-bit stamp out: the leave after them rebuilds, and re-insertion resumes
        s.phase(f"hop {hop}", moves=[(m, base.on(5, 3, 5) if away else base.home(0))], expect=(1, 0) if hop == 128 else (0, 1),
                pairs_in=there if away else base.home_pairs(0), pairs_out=base.home_pairs(0) if away else there, trigger="stamp" if hop == 128 else None)
    return s.phases


def _row(base, j, count, first=0):
    nx, _, nz = base.n
    out = []
    for n in range(first, first + count):
        out.append((n % nx, j, n // nx))
    assert all(k < nz for _, _, k in out)
    return out


def _fallbacks(b):
    base = _Base(b)
    s = _Script(b).phase("first", expect=(1, 0), large=3)
    mv = lambda cells, dy=0.25: [(base.cube[c], base.shifted(*c, dy=dy)) for c in cells]
    s.phase("140 leave at once", moves=mv(_row(base, 5, 140)), expect=(1, 0), trigger="leavers16")
    s.phase("40 leave", moves=mv(_row(base, 4, 40)), expect=(0, 40))
    s.phase("30 more: 70 have moved", moves=mv(_row(base, 4, 30, first=40)), expect=(1, 0), trigger="moved32")
    s.phase("a large collider moves", moves=[(base.wall[0], (-2.5, 4.5, 8.0))], expect=(1, 0), trigger="large_moved", large=3)
    s.phase("one leaves", moves=mv([(1, 6, 1)]), expect=(0, 1))
    grown = base.cube[8, 6, 8]
    s.phase("a small box grows beyond the small class", edits=[(grown, (4 * H, 4 * H, 4 * H))], expect=(1, 0), trigger="resized", large=4,
            pairs_in=[(grown, base.cube[7, 6, 8]), (grown, base.cube[9, 6, 8]), (grown, base.cube[10, 6, 8])])
    s.phase("one leaves after it", moves=mv([(1, 6, 1)], dy=0.5), expect=(0, 1))
    return s.phases


def _fallbacks_kept(b):
    base = _Base(b)
    s = _Script(b).phase("first", expect=(1, 0))
    mv = lambda cells: [(base.cube[c], base.shifted(*c)) for c in cells]
    s.phase("5 leave", moves=mv(_row(base, 4, 5)), expect=(0, 5))
    s.phase("30 leave: 64 pairs each would fill the kept buffer beyond 7/8", moves=mv(_row(base, 5, 30)), expect=(1, 0), trigger="kept78")
    s.phase("5 leave after it", moves=mv(_row(base, 3, 5)), expect=(0, 5))
    return s.phases


def _fallbacks_combos(b):
    base = _Base(b, nx=32, ny=16, nz=32, movers=13)
    s = _Script(b).phase("first", expect=(1, 0), large=3)
    cells = _row(base, 9, 512)
    s.phase("64 leave", moves=[(base.cube[c], base.shifted(*c)) for c in cells[:64]], expect=(0, 64))
    s.phase("512 leave, 512 have moved: the quadratic tests outgrow the rebuild", moves=[(base.cube[c], base.shifted(*c, dy=0.5 if n < 64 else 0.25)) for n, c in enumerate(cells)],
            expect=(1, 0), trigger="combos")
    s.phase("3 leave after it", moves=[(base.cube[c], base.shifted(*c, dy=0.75)) for c in cells[:3]], expect=(0, 3))
    return s.phases


def _fallbacks_esc(b):
    """A sparse lattice: 41 x 40 x 41 isolated cubes at pitch 1.5 and 300 cubes that each overlap one of them -- the only pairs, whatever moves below."""
    base = _Base(b, nx=41, ny=40, nz=41, movers=0, pitch=(1.5, 1.5, 1.5), slab_top=-1.0)
    extra = [b.box(base.cube_min(2 * (i % 20), 39, 2 * (i // 20)) + H + (0.5, 0.25, 0.5), (H, H, H)) for i in range(300)]
    s = _Script(b)
    pairs = [(e, base.cube[2 * (i % 20), 39, 2 * (i // 20)]) for i, e in enumerate(extra)]
    s.phase("first", expect=(1, 0), pairs_in=pairs)
    cells = [(i, 3, k) for k in range(41) for i in range(41)] + [(i, 5, k) for k in range(41) for i in range(41)] + [(i, 7, k) for k in range(21) for i in range(41)]
    cells = cells[:4200]          # (4200 x 16 <= C: clause "leavers x 16 > C" stays off)
    s.phase("100 leave", moves=[(base.cube[c], base.shifted(*c)) for c in cells[:100]], expect=(0, 100), pairs_in=pairs)
    s.phase("4200 leave: more than the list of leavers holds", moves=[(base.cube[c], base.shifted(*c, dy=0.5 if n < 100 else 0.25)) for n, c in enumerate(cells)],
            expect=(1, 0), trigger="esc_max", pairs_in=pairs)
    s.phase("3 leave after it", moves=[(base.cube[c], base.shifted(*c, dy=0.0)) for c in cells[:3]], expect=(0, 3), pairs_in=pairs)
    s.b.known_pairs = pairs
    return s.phases


def _direct_and_back(b):
    """Call 1 rebuilds as every first call does, calls 2 .. 10 because a wall moves.  After eight rebuilds in a row the host searches DIRECT for 64 calls: calls 9 .. 72
    (rebuilds + 1 each, whatever moves); call 73 is the kept list's again and rebuilds it (the DIRECT search keeps nothing); calls 74 .. 80 re-use it."""
    base = _Base(b)
    s = _Script(b).phase("first", expect=(1, 0))
    wall = np.array([-3.0, 4.5, 8.0])
    for n in range(1, 10):
        s.phase(f"the wall moves ({n})", moves=[(base.wall[0], wall + (0.25 * (n % 2), 0.0, 0.0))], expect=(1, 0))
    d = 1.0 / 128.0
    c, right = base.cube[3, 2, 3], base.cube[4, 2, 3]
    for n in range(70):
        on = n % 2 == 0
        s.phase(f"quiet {n}", moves=[(c, base.cube_min(3, 2, 3) + H + (d if on else 0.0, 0.0, 0.0)), (base.mover[1], base.home(1) + (0.0, d if on else -d, 0.0))],
                expect=(1, 0) if n < 63 else (0, 0), pairs_in=[(c, right)] if on else [], pairs_out=[] if on else [(c, right)])
    return s.phases


def _sleeper_edge(b):
    base = _Base(b)
    # in the empty layer above cubes (., 4, .): spheres of the cubes' extent, some touching, some whose boxes only overlap; all asleep
    c0 = np.array([3.0, 9.0, 7.0]) + H
    sp = [b.sphere(c0, H, idle=0xff), b.sphere(c0 + (0.5, 0.0, 0.5), H, idle=0xff), b.sphere(c0 + (1.25, 0.0, 1.25), H, idle=0xff),
          b.sphere(c0 + (1.75, 0.0, 1.75), H, idle=0xff)]
    bx = b.box(c0 + (2.375, 0.0, 1.75), (H, H, H), idle=0xff)
    m = base.mover
    s = _Script(b)
    s.phase("first: the cluster sleeps", expect=(1, 0), pairs_in=[(sp[0], sp[1]), (sp[1], sp[2]), (sp[2], sp[3]), (sp[3], bx)])
    s.phase("a leaver's box overlaps a sleeper's at a corner", moves=[(m[0], c0 + (1.25 + 0.75, 0.75, 1.25 - 0.75))], expect=(0, 1), pairs_in=[(m[0], sp[2])])
    s.phase("it leaves again", moves=[(m[0], base.free(9.0, 1, 2))], expect=(0, 1), pairs_out=[(m[0], sp[2])])
    s.phase("another lands on the first sleeper", moves=[(m[1], c0 - (0.25, 0.5, 0.25))], expect=(0, 1), pairs_in=[(m[1], sp[0])])
    s.phase("a sleeper is moved by the caller", moves=[(sp[3], c0 + (1.75, 0.5, 1.75))], expect=(0, 1), pairs_in=[(sp[2], sp[3])])
    return s.phases


_BUILDERS = {
    "all_large_64": ("grid", "ref", lambda b: _all_large(b, 64), {}), "all_large_65": ("grid", "ref", lambda b: _all_large(b, 65), {}),
    "size_ladder_64": ("grid", "ref", lambda b: _size_ladder(b, 64), {}), "size_ladder_65": ("grid", "ref", lambda b: _size_ladder(b, 65), {}),
    "cell_edges": ("grid", "ref", _cell_edges, {}), "sparse_far": ("grid", "ref", _sparse_far, {}),
    "dense_cell": ("grid", "ref", _dense_cell, dict(max_contacts=32768, max_pairs=24576)), "compound_static": ("grid", "ref", _compound_static, {}),
    "lane_split_16384": ("grid", "host", lambda b: _lane_split(b, 16384), {}), "lane_split_16385": ("grid", "host", lambda b: _lane_split(b, 16385), {}),
    "wiggle": ("kept", "ref", _wiggle, {}), "one_leaver": ("kept", "ref", _one_leaver, {}), "leavers_meet": ("kept", "ref", _leavers_meet, {}),
    "stamp_wear": ("kept", "ref", _stamp_wear, {}), "fallbacks": ("kept", "ref", _fallbacks, {}), "fallbacks_kept": ("kept", "ref", _fallbacks_kept, dict(max_pairs=2048)),
    "fallbacks_combos": ("kept", "host", _fallbacks_combos, {}), "fallbacks_esc": ("kept", "list", _fallbacks_esc, {}),
    "direct_and_back": ("kept", "ref", _direct_and_back, {}), "sleeper_edge": ("kept", "ref_only", _sleeper_edge, {}),
}
_CACHE = {}


def world(case):
    """The scene of `case`, built once per process; treat it as read-only (scene_at copies what a phase's edits change)."""
    if case not in _CACHE:
        kind, oracle, build, kw = _BUILDERS[case]
        b = _Builder()
        phases = build(b)
        scene = b.scene(case, kind, oracle, phases, world=kw)
        if hasattr(b, "known_pairs"):
            scene["bp"]["known_pairs"] = sorted(tuple(sorted((b.idx(x), b.idx(y)))) for x, y in b.known_pairs)
        _CACHE[case] = scene
    return _CACHE[case]


def ncolliders(scene):
    return len(scene["box_tags"]) + len(scene["sphere_tags"])


# ---- numpy: AABBs of axis-aligned worlds, overlapping pairs by cell hashing -----------------------------------------------------------------------------------------
def plain_aabbs(scene, transforms):
    """float32 AABBs (min, max) of a world in which every collider that matters is axis-aligned and either alone on its dynamic body with an identity local
    transform or on body 0: centre -+ half extents.  (The kept-list worlds; the grid worlds with rotated colliders take theirs from hostsim_util.pairs.)"""
    bx, sx = scene["box_transforms"], scene["sphere_transforms"]
    assert (bx["rotation"] == np.array([0, 0, 0, 1], F)).all() and (transforms["rotation"] == np.array([0, 0, 0, 1], F)).all()
    body = np.concatenate([bx["body"], sx["body"]])
    local = np.concatenate([bx["position"], sx["position"]]).astype(F)
    assert ((local == 0).all(axis=1) | (body == 0)).all()
    c = (local + transforms["position"][body]).astype(F)
    half = np.concatenate([scene["box_data"]["size"], np.repeat(scene["sphere_data"]["radius"][:, None], 3, axis=1)]).astype(F)
    return (c - half).astype(F), (c + half).astype(F), body


def _strict(lo, hi, i, j):
    return ((hi[j] > lo[i]) & (hi[i] > lo[j])).all(axis=1)


def overlap_pairs(lo, hi):
    """All i < j whose boxes overlap strictly, (m, 2) in (i, j) order: the few largest boxes by brute force, the rest by hashing min corners into cells of the
    largest remaining extent (a partner's cell is a neighbour's)."""
    n = len(lo)
    ext = (hi - lo).max(axis=1)
    order = np.argsort(ext, kind="stable")
    nbig = min(n, 72)
    big, small = order[n - nbig:], order[:n - nbig]
    found = []
    allidx = np.arange(n)
    for a in big:
        hit = ((hi > lo[a]) & (hi[a] > lo)).all(axis=1)
        hit[a] = False
        found.append(np.stack([np.minimum(a, allidx[hit]), np.maximum(a, allidx[hit])], axis=1))
    if len(small) > 1:
        cell = max(float(ext[small].max()), 1e-30)
        span = float((lo[small].max(axis=0) - lo[small].min(axis=0)).max())
        cell = max(cell, span / 2000.0)
        q = np.floor((lo[small].astype(np.float64) - lo[small].min(axis=0)) / cell).astype(np.int64) + 1
        dims = q.max(axis=0) + 2
        key = (q[:, 2] * dims[1] + q[:, 1]) * dims[0] + q[:, 0]
        srt = np.argsort(key, kind="stable")
        skey = key[srt]
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                # a row of three neighbouring cells along x is one range of the sorted keys
                base = key + (dz * dims[1] + dy) * dims[0]
                l, r = np.searchsorted(skey, base - 1, side="left"), np.searchsorted(skey, base + 1, side="right")
                cnt = r - l
                tot = int(cnt.sum())
                if not tot:
                    continue
                ii = np.repeat(np.arange(len(small)), cnt)
                jj = np.repeat(l, cnt) + (np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt))
                a, c = small[ii], small[srt[jj]]
                keep = a < c
                a, c = a[keep], c[keep]
                hit = _strict(lo, hi, a, c)
                found.append(np.stack([a[hit], c[hit]], axis=1))
    out = np.unique(np.concatenate(found), axis=0) if found else np.zeros((0, 2), dtype=np.int64)
    return out[np.lexsort((out[:, 1], out[:, 0]))]


# ---- the trigger model: the documented rules of k_xform / k_grid_setup / k_cell_keys and of the host's switch, in numpy; it never calls the library ----------------------
def _class_of(ext):
    return (np.asarray(ext, dtype=F).view(np.uint32) >> np.uint32(21)) & np.uint32(1023)


class Model:
    """One default world's broadphase state across collide() calls.  call(lo, hi) takes the exact float32 AABBs of this call and returns dict(rebuild, inserts,
    large, direct, leavers, moved, clauses, reason): what the counters must show and why."""

    def __init__(self, ncolliders, max_contacts, max_pairs=None, nbodies=None):
        self.C = ncolliders
        pair_cap = max_pairs if max_pairs else max_contacts // 2 + 1024
        self.kept_cap = max(2 * pair_cap, 4096)
        want = 1
        while want < 4 * ncolliders:
            want <<= 1
        self.max_cells = min(max(want, 1 << 16), 1 << 24)
        self.fat_valid, self.cell_inv, self.small_exp, self.moved, self.large, self.fat_count = False, F(0.0), 0, 0, 0, 0
        self.gen = np.zeros(ncolliders, dtype=np.int64)           # 7-bit stamp; is_large apart
        self.is_large = np.zeros(ncolliders, dtype=bool)
        self.flo = self.fhi = None
        self.rebuilds, self.seen, self.streak, self.direct_left = 0, 0, 0, 0

    def _host_direct(self):
        # after eight rebuilds in a row the next 64 calls search DIRECT, then the list gets another chance
        seen = self.rebuilds
        if self.direct_left > 0:
            self.direct_left -= 1
            if self.direct_left == 0:
                self.streak = 0
        else:
            self.streak = self.streak + 1 if seen != self.seen else 0
            if self.streak >= 8:
                self.direct_left = 64
        self.seen = seen
        return self.direct_left > 0

    def call(self, lo, hi):
        C = self.C
        direct = self._host_direct()
        margin = F(0.0) if direct else (F(F(0.03125) / self.cell_inv) if self.cell_inv > 0 else F(0.05))
        f0, f1 = (lo - margin).astype(F), (hi + margin).astype(F)
        fext = (f1 - f0).astype(F).max(axis=1)
        cls = _class_of(fext).astype(np.int64)
        info = dict(direct=direct, leavers=0, clauses={}, reason=None, inserts=0)
        rebuild = direct or not self.fat_valid
        if rebuild:
            info["reason"] = "direct" if direct else "first"
        else:
            # containment: the exact box inside the inflated box on file
            out = ~((lo >= self.flo).all(axis=1) & (hi <= self.fhi).all(axis=1))
            again = out & ~self.is_large & (self.gen < 127) & (cls <= self.small_exp)
            leavers = int(again.sum())
            self.moved += int((again & (self.gen == 0)).sum())
            overflow = leavers > ESC_MAX or self.moved > MOVED_MAX
            escaped = bool((out & ~again).any()) or overflow
            clauses = dict(kept78=self.fat_count + 64 * leavers > self.kept_cap // 8 * 7, leavers16=leavers * 16 > C,
                           combos=leavers * (self.moved + self.large) > 16 * C, moved32=self.moved * 32 > C)
            crowded = leavers != 0 and any(clauses.values())
            why = []
            if (out & self.is_large).any(): why.append("large_moved")
            if (out & ~self.is_large & (self.gen >= 127)).any(): why.append("stamp")
            if (out & ~self.is_large & (cls > self.small_exp)).any(): why.append("resized")
            if overflow: why.append("esc_max")
            info.update(leavers=leavers, moved=self.moved, clauses=clauses if leavers else {k: False for k in clauses}, escaped=why)
            rebuild = escaped or crowded
            if not rebuild:
                if leavers:
                    idx = np.flatnonzero(again)
                    self.gen[idx] += 1
                    self.flo[idx], self.fhi[idx] = f0[idx], f1[idx]
                    # the new boxes' pairs: against everybody (unmoved through the grid, large and moved directly), two leavers of one call once
                    new = 0
                    for a in idx:
                        hit = ((self.fhi > self.flo[a]) & (self.fhi[a] > self.flo)).all(axis=1)
                        hit[a] = False
                        new += int(hit.sum()) - int((hit & again & (np.arange(C) < a)).sum())
                    self.fat_count += new
                info["inserts"] = leavers
        if rebuild:
            self.rebuilds += 1
            self.moved = 0
            self.fat_valid = not direct
            budget = max(C // 1024, 64)
            hist = np.bincount(cls, minlength=1024)
            suffix = np.cumsum(hist[::-1])[::-1]
            over = np.flatnonzero(suffix > budget)
            e = int(over.max()) if len(over) else 0
            e = min(max(e, 64 << 2), 190 << 2)
            split_moved = self.small_exp != e
            was_small = cls <= self.small_exp
            self.small_exp = e
            cell = np.array([(e + 1) << 21], dtype=np.uint32).view(F)[0]
            inv = F(F(1.0) / cell)
            if split_moved:
                gmin, gmax, any_small = lo.min(axis=0), lo.max(axis=0), True
            else:
                any_small = bool(was_small.any())
                gmin, gmax = (f0[was_small].min(axis=0), f0[was_small].max(axis=0)) if any_small else (np.zeros(3, F), np.zeros(3, F))
            origin, dims = np.zeros(3, F), np.ones(3, dtype=np.int64)
            if any_small:
                origin = gmin.astype(F)
                for _ in range(256):
                    d = ((gmax - gmin).astype(F) * inv).astype(F)
                    n = np.minimum(np.maximum(d, F(0.0)), F(1e7)).astype(np.int64) + 2
                    if int(n[0]) * int(n[1]) * int(n[2]) < self.max_cells:
                        dims = n
                        break
                    inv = F(inv * F(0.5))
            self.cell_inv = inv
            coord = lambda x: np.floor(np.minimum(np.maximum(((x - origin).astype(F) * inv).astype(F), F(-1.0)), F(16777216.0))).astype(np.int64)
            span = (coord(f1) - coord(f0)).max(axis=1)
            self.is_large = (cls > e) | (span > 1)
            self.large = int(self.is_large.sum())
            self.gen[:] = 0
            self.flo, self.fhi = f0.copy(), f1.copy()
            self.fat_count = 0 if direct else len(overlap_pairs(f0, f1))
            info.update(origin=origin, cell_inv=inv, dims=dims, small_exp=e)
        info.update(rebuild=bool(rebuild), large=self.large)
        return info


def default_max_contacts(scene):
    return scene["bp"]["world"].get("max_contacts", max(4096, 8 * len(scene["body_transforms"])))


def model_for(scene):
    return Model(ncolliders(scene), default_max_contacts(scene), scene["bp"]["world"].get("max_pairs"))


def check_trigger(phase, info):
    """A fallback phase rebuilds for its trigger alone -- as far as the clauses allow (module docstring): leavers16 implies moved32, esc_max implies moved32 and combos
    at fallbacks_esc's size."""
    t = phase["trigger"]
    if t is None:
        return
    implied = {"leavers16": {"moved32"}, "esc_max": {"moved32", "combos"}}.get(t, set())
    held = {k for k, v in info["clauses"].items() if v} | set(info.get("escaped", []))
    assert t in held, (phase["name"], t, info)
    assert held - {t} <= implied, (phase["name"], t, held)
    if t == "esc_max":
        assert not info["clauses"]["leavers16"], info
