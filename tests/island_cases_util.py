"""Crafted worlds for the islands and the sleeping of nudge_amd/csrc/nh_collide.hip (uf_find / uf_union, k_uf_union_records, k_uf_union_connections, k_uf_flatten, the
coarse unions of emit_pair, k_large_pairs<true> and k_kept_filter, k_active_flags / k_active_write, k_filter_records, the sleeping pairs of k_gather_contacts) and for the
cache kernels behind them (nh_cache.hip: k_cull_flags / k_cull_write, k_write_cache, k_cache_lookup(_listed); nh_solve.hip: cache_probe / cache_search), shared by
tests/test_cpu_island_cases.py (the oracle against the compiled reference, no GPU) and tests/test_gpu_island_cases.py.

THE ORACLE is plain numpy (`islands`): from the overlapping collider pairs, the contacts (key, feature, bodies), the connections and the idle counters it computes what
nudge.cpp:3500-3703 and 3788-4008 do, with a FULL union -- every edge, awake-awake ones included, body 0 never joined; connected sets by label propagation, no union-find --:
the active list (ascending), the surviving contacts and the sorted sleeping pairs (coarse drops: larger tag first; fine drops: the contact's own tag word; both in the wide
format of parity_util.widen_sleeping).  `sleeping_end_only=True` unites only edges with a sleeping end, which is what the kernels do (comment above emit_pair); the CPU test
shows both give the same lists on every world.  `cache_stages` models the cache: cull (entries whose tag equals a sleeping-pair word), lookup (exact (tag, feature)
match, else zero), write (merge by (tag, feature); a culled entry precedes a contact of equal key: nudge.cpp:4110-4158, "if (a < b) contact else culled").

A world is a scene (the keys of nudge_amd.scenes._assemble, plus "connections") with scene["isl"] = dict(kind="graph" | "geometry", oracle="host" | "list", phases=[dict(name,
idle, expect)]).  Tags equal collider indices, momenta are zero, a phase states every body's idle counter (the GPU test sets them through set_bodies(idle=...), so that
nh_bodies_changed is called) and is followed by one collide(); nothing moves; only the staged calls run, never advance.  The connections are a case's own and last
through its phases.  `expect` holds what the case states in words (active / contacts / sleeping counts, where it does); the oracle must agree with it (CPU test).

GRAPH worlds (default N = 6000 bodies; `world(case, n)` builds another size): every dynamic body k = 1 .. N is one sphere of radius 1/4 -- collider k, tag k -- on a square
lattice of pitch 2, resting on ONE static slab (collider 0, body 0) whose top face lies 2^-6 above the spheres' lowest points: exactly one box-sphere contact each, key
k << 32, feature 0, bodies (0, k).  No two spheres' boxes overlap: the overlapping pairs are (slab, sphere k) and nothing else (oracle="list": known by construction,
checked against hostsim at N = 6000), and the graph is the connection list alone.  Every pair has body 0 at one end, so a drop is always a coarse one.
  chain_up / chain_down / chain_shuffled   edges (i, i + 1) listed ascending, descending ((i + 1, i)), and in a seeded random order over randomly relabelled bodies; phase 1:
                    all asleep (0xff) but one end at 0xfe -- everybody active; phase 2: that end at 0xff too -- nobody active, no contact, N sleeping pairs.
  star              a hub in the middle of the index range and N - 1 leaves; hub asleep and one leaf awake, then hub awake and every leaf asleep.
  tree              a complete binary tree (heap numbering), edges leaf level first; one awake leaf.
  two_giants        odd bodies in one random spanning tree, even bodies in another, the two edge lists interleaved at random; one awake body among the odd ones.
  confetti          ~N / 8 components of seeded random size 1 .. 20 over relabelled bodies, random trees plus extra cycle edges; every second component holds exactly one
                    awake member whose idle counter is drawn from {0, 1, 0xfe}.
  noise             confetti plus self edges (a, a), every edge listed twice and in both orders, and edges (0, a), (a, 0) from body 0 into one awake and one sleeping
                    component: the sleeping one stays asleep.
  awake_bridges     paths S-A-A-S, S-A-S and A-S-S-A of mixed idle counters (idle 0 between sleepers included), and lone sleepers: the full union and the sleeping-end
                    union build DIFFERENT sets here.
  nobody_asleep / all_asleep_no_edges     the direct 1 .. B - 1 list; an empty active list with every pair sleeping.
Two LARGE instances (GPU only; LARGE below): chain_shuffled at 140,000 and confetti at 530,000.

GEOMETRY worlds (a few dozen colliders; collider 0 is a small static box under the slab that nobody touches, so that no contact key has a zero high word; the slab is
collider 1; the two sphere near-miss worlds carry 72 more static boxes far below, which makes their spheres members of the grid: see _ground).  Two phases with the same idle counters and nothing moved: the first collide() rebuilds (unions in the grid search), the second goes through k_kept_filter;
the GPU test runs each as a default world and as a world with the DIRECT search (NH_NO_KEPT_PAIRS).
  near_miss_spheres a sleeping sphere S on the slab, an awake sphere A diagonally above: the boxes overlap strictly, the spheres are 0.3 apart.  Coarse set {S, A} active, fine
                    set {S} not: S is off the active list, its slab contact becomes a sleeping pair in the contact's tag-word format.
  near_miss_boxes   the same with two boxes turned 45 degrees about y: the AABBs overlap, the SAT separates them.
  near_miss_chain   S1 .. S12 overlap the next by AABB only, an awake A at the end: all coarse-active, each fine-asleep alone.
  touching          A touches S: both active, no sleeping pair.
  sleeping_heap     44 sleeping boxes and spheres in contact, with box overlaps that do not touch; nothing awake: every overlapping pair is a sleeping pair, larger tag
                    first, contacts 0, active 0.
  far_connection    sleeping_heap plus one connection from a heap member to an awake sphere far away: the whole heap is active.
  compound          a sleeping body with two colliders of which one touches an awake body (both active), and a second such body whose awake neighbour only overlaps a
                    box (fine-asleep: both its slab contacts become sleeping pairs).

CACHE scripts (`crafted_caches`): caches the library did not write, built from a world's own contact list L after collide(); sorted by (tag, feature) without duplicate
keys (what the reference's merge assumes), payload (3 i + 1, 3 i + 2, 3 i + 3) as floats for entry i of the crafted cache, so that a wrong source entry shows.

Left out: a culled entry whose (tag, feature) equals a live contact's cannot be produced by a world's own lists -- a pair is dropped or has contacts, never both -- so the
tie rule of k_write_cache is pushed through contacts appended behind collide()'s list (`tie_script`: nh_append_contacts on the GPU, RefWorld.append_contacts in the
reference); duplicate keys within a cache and unsorted caches (the reference's merge-join and the library's binary searches are both undefined on them)."""
import numpy as np

from nudge_amd import scenes as S
from broadphase_cases_util import _Builder, _quat

F = np.float32
N_DEFAULT = 6000
REF_LIMIT = 8192
PUSH = 2.0 ** -6
# the two sizes beyond the island launches' thread counts (nh_collide.hip, the NH_LAUNCH sites of section 9: nh_grid_for(n, 256, cap) launches at most cap workgroups of 256)
COARSE_THREADS = 512 * 256             # "uf_union_connections" (coarse), "coarse_flatten": nh_grid_for(.., 256, 512)
FINE_THREADS = 2048 * 256              # "uf_union_connections" (fine), "uf_union_records", "uf_flatten", "active_flags", "active_write", "filter_records": nh_grid_for(.., 256, 2048)
LARGE = {"chain_shuffled": 140000, "confetti": 530000}
assert LARGE["chain_shuffled"] > COARSE_THREADS and LARGE["confetti"] > FINE_THREADS

GRAPH = ["chain_up", "chain_down", "chain_shuffled", "star", "tree", "two_giants", "confetti", "noise", "awake_bridges", "nobody_asleep", "all_asleep_no_edges"]
GEOMETRY = ["near_miss_spheres", "near_miss_boxes", "near_miss_chain", "touching", "sleeping_heap", "far_connection", "compound"]
CASES = GRAPH + GEOMETRY
CACHE_WORLDS = ["sleeping_heap", "far_connection", "near_miss_spheres", "confetti"]
CACHES = ["same", "shifted_1", "shifted_5", "shifted_300", "shifted_back", "holes", "feature_only", "empty", "only_foreign", "short", "long", "sleepers", "sleepers_quirk"]


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------------------------------------------
def components(n, a, b):
    """Label (the smallest member) of the connected set of every node 0 .. n - 1 under the edges (a[i], b[i]): labels are hooked to the smaller label across every edge and
    then shortened (label of label) until nothing changes.  At the fixed point both ends of every edge carry one label, and a label is always a member of its node's set."""
    lab = np.arange(n, dtype=np.int64)
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    while len(a):
        la, lb = lab[a], lab[b]
        m = np.minimum(la, lb)
        new = lab.copy()
        for at in (la, lb, a, b):
            np.minimum.at(new, at, m)
        while True:
            nn = new[new]
            if np.array_equal(nn, new):
                break
            new = nn
        if np.array_equal(new, lab):
            break
        lab = new
    return lab


def _active_sets(nb, ea, eb, idle, sleeping_end_only):
    """(label per body, active per body): sets over the edges with body 0 never joined; a set is active iff a member other than body 0 has an idle counter != 0xff."""
    ea, eb = np.asarray(ea, dtype=np.int64), np.asarray(eb, dtype=np.int64)
    keep = (ea != 0) & (eb != 0)
    if sleeping_end_only:
        keep &= (idle[ea] == 0xff) | (idle[eb] == 0xff)
    lab = components(nb, ea[keep], eb[keep])
    awake = np.zeros(nb, dtype=bool)
    awake[lab[1:][idle[1:] != 0xff]] = True
    return lab, awake[lab]


def islands(nbodies, owner, tags, pairs, contacts, connections, idle, sleeping_end_only=False):
    """`owner`: body of every collider; `tags`: tag of every collider; `pairs`: (m, 2) collider indices whose boxes overlap (bodies differ); `contacts`: dict(keys, features,
    bodies) in tag order, keys = a_tag | b_tag << 32; `connections`: (k, 2) bodies; `idle`: uint8 per body.  Returns dict(active, keep (mask over the contacts), sleeping,
    coarse_sleeping, fine_sleeping)."""
    idle = np.asarray(idle, dtype=np.uint8)
    owner, tags = np.asarray(owner, dtype=np.int64), np.asarray(tags, dtype=np.uint64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    con = np.asarray(connections, dtype=np.int64).reshape(-1, 2)
    keys, cb = np.asarray(contacts["keys"], dtype=np.uint64), np.asarray(contacts["bodies"], dtype=np.int64).reshape(-1, 2)
    # coarse level (nudge.cpp:3500-3703): sets over connections and overlapping pairs; a pair of an inactive set is dropped before the narrowphase
    pa, pb = owner[pairs[:, 0]], owner[pairs[:, 1]]
    assert (pa != pb).all()
    lab, act = _active_sets(nbodies, np.concatenate([con[:, 0], pa]), np.concatenate([con[:, 1], pb]), idle, sleeping_end_only)
    drop = ~act[np.where(pa != 0, pa, pb)]                     # sets[a] | sets[b] with sets[0] = 0: the two are one set, or one is body 0
    ta, tb = tags[pairs[drop, 0]], tags[pairs[drop, 1]]
    coarse = np.maximum(ta, tb) | (np.minimum(ta, tb) << np.uint64(32))
    # the contacts of dropped pairs were never made
    lo, hi = keys & np.uint64(0xFFFFFFFF), keys >> np.uint64(32)
    unordered = np.minimum(lo, hi) | (np.maximum(lo, hi) << np.uint64(32))
    dropped = np.minimum(ta, tb) | (np.maximum(ta, tb) << np.uint64(32))
    keep = ~np.isin(unordered, dropped)
    # fine level (3788-4008): sets over connections and the bodies of the contacts that were made
    lab, act = _active_sets(nbodies, np.concatenate([con[:, 0], cb[keep, 0]]), np.concatenate([con[:, 1], cb[keep, 1]]), idle, sleeping_end_only)
    active = np.flatnonzero(act).astype(np.uint32)
    active = active[active != 0]
    asleep = keep & ~act[np.where(cb[:, 0] != 0, cb[:, 0], cb[:, 1])]
    fine = np.unique(keys[asleep])
    keep &= ~asleep
    return dict(active=active, keep=keep, sleeping=np.sort(np.concatenate([coarse, fine])), coarse_sleeping=np.sort(coarse), fine_sleeping=fine)


def cache_stages(cache, contacts, sleeping):
    """`cache` = dict(tags, features, data) sorted by (tag, feature); `contacts` = dict(tags, features) of the surviving contacts in tag order; `sleeping`: the sleeping-pair
    words.  Returns dict(culled (mask over the cache), lookup (S.IMPULSE per contact: the entry of equal (tag, feature), else zero), write = dict(count, tags, features, data):
    the merge of the contacts, carrying their looked-up impulses, with the culled entries)."""
    kt, kf, kd = np.asarray(cache["tags"], dtype=np.uint64), np.asarray(cache["features"], dtype=np.uint32), np.asarray(cache["data"], dtype=S.IMPULSE)
    ct, cf = np.asarray(contacts["tags"], dtype=np.uint64), np.asarray(contacts["features"], dtype=np.uint32)
    culled = np.isin(kt, np.asarray(sleeping, dtype=np.uint64))
    where = {(int(t), int(f)): i for i, (t, f) in enumerate(zip(kt.tolist(), kf.tolist()))}
    assert len(where) == len(kt), "duplicate keys in a crafted cache"
    lookup = np.zeros(len(ct), dtype=S.IMPULSE)
    for i, key in enumerate(zip(ct.tolist(), cf.tolist())):
        if key in where:
            lookup[i] = kd[where[key]]
    # culled entries first, then the contacts: a stable sort by (tag, feature) then puts a culled entry before a contact of equal key
    t, f, d = np.concatenate([kt[culled], ct]), np.concatenate([kf[culled], cf]), np.concatenate([kd[culled], lookup])
    order = np.lexsort((f, t))          # (lexsort is stable)
    return dict(culled=culled, lookup=lookup, write=dict(count=len(t), tags=t[order], features=f[order], data=d[order]))


# ---- graph worlds ---------------------------------------------------------------------------------------------------------------------------------------------------------
def _graph_scene(name, n, edges, phases):
    side = int(np.ceil(np.sqrt(n)))
    nb = n + 1
    k = np.arange(n)
    bt = S._identity_transforms(nb)
    bt["position"][1:, 0] = 2.0 * (k % side); bt["position"][1:, 1] = 0.25 - PUSH; bt["position"][1:, 2] = 2.0 * (k // side)
    props = np.zeros(nb, dtype=S.PROPERTIES)
    props["mass_inverse"][1:] = 1.0; props["inertia_inverse"][1:] = 1.0
    xt, st = S._identity_transforms(1), S._identity_transforms(n)
    xd, sd = np.zeros(1, dtype=S.BOX), np.zeros(n, dtype=S.SPHERE)
    xt["position"][0] = (side - 1.0, -0.5, side - 1.0); xd["size"][0] = (side + 1.0, 0.5, side + 1.0)          # the slab: top face at y = 0
    st["body"] = 1 + k; sd["radius"] = 0.25
    edges = np.asarray(edges, dtype=np.uint32).reshape(-1, 2)
    assert edges.max(initial=0) <= n
    return dict(name=f"island_{name}_{n}", body_transforms=bt, body_properties=props, body_momentum=np.zeros(nb, dtype=S.MOMENTUM), idle_counters=phases[0]["idle"].copy(),
                box_tags=np.zeros(1, dtype=np.uint32), box_data=xd, box_transforms=xt, sphere_tags=np.arange(1, n + 1, dtype=np.uint32), sphere_data=sd, sphere_transforms=st,
                params=dict(S.DEFAULT_PARAMS), connections=edges, isl=dict(kind="graph", oracle="list", phases=phases, n=n))


def _idle(n, fill):
    out = np.full(n + 1, fill, dtype=np.uint8)
    out[0] = 0
    return out


def _phase(name, idle, **expect):
    return dict(name=name, idle=idle, expect=expect)


def _everybody(n):
    return dict(active=n, contacts=n, sleeping=0)


def _nobody(n):
    return dict(active=0, contacts=0, sleeping=n)


def _chain(n, order):
    rng = np.random.default_rng(51)
    label = np.arange(1, n + 1)
    if order == "shuffled":
        label = rng.permutation(n) + 1
    e = np.stack([label[:-1], label[1:]], axis=1)
    if order == "down":
        e = e[::-1, ::-1]
    elif order == "shuffled":
        e = e[rng.permutation(len(e))]
    end = int(label[-1] if order == "down" else label[0])
    one = _idle(n, 0xff); one[end] = 0xfe
    return e, [_phase("one end at 0xfe", one, **_everybody(n)), _phase("that end asleep too", _idle(n, 0xff), **_nobody(n))]


def _star(n):
    hub = n // 2
    leaves = np.concatenate([np.arange(1, hub), np.arange(hub + 1, n + 1)])
    e = np.stack([np.full(n - 1, hub), leaves], axis=1)
    e[::2] = e[::2, ::-1]                          # (the hub at either end of an edge)
    a = _idle(n, 0xff); a[n - 3] = 0
    b = _idle(n, 0xff); b[hub] = 1
    return e, [_phase("hub asleep, one leaf awake", a, **_everybody(n)), _phase("hub awake, every leaf asleep", b, **_everybody(n))]


def _tree(n):
    i = np.arange(n, 1, -1)                        # heap numbering: the parent of i is i // 2; leaf level first
    idle = _idle(n, 0xff); idle[n] = 0x10
    return np.stack([i, i // 2], axis=1), [_phase("one awake leaf", idle, **_everybody(n))]


def _random_tree(rng, members):
    members = rng.permutation(members)
    parent = (rng.random(len(members) - 1) * np.arange(1, len(members))).astype(np.int64)          # member k + 1 hangs under a random earlier one
    return np.stack([members[1:], members[parent]], axis=1)


def _two_giants(n):
    rng = np.random.default_rng(52)
    odd, even = np.arange(1, n + 1, 2), np.arange(2, n + 1, 2)
    e = np.concatenate([_random_tree(rng, odd), _random_tree(rng, even)])
    e = e[rng.permutation(len(e))]
    idle = _idle(n, 0xff); idle[int(odd[len(odd) // 3])] = 0
    return e, [_phase("one awake body among the odd ones", idle, active=len(odd), contacts=len(odd), sleeping=len(even))]


def _confetti(n, seed=53):
    """(edges, idle, components as a list of member arrays, awake flag per component)"""
    rng = np.random.default_rng(seed)
    label = rng.permutation(n) + 1
    sizes = []
    left = n
    while left:
        s = min(int(rng.integers(1, 21)), left)
        sizes.append(s); left -= s
    idle = _idle(n, 0xff)
    edges, comps, awake = [], [], []
    at = 0
    for c, s in enumerate(sizes):
        mem = label[at:at + s]; at += s
        comps.append(mem)
        if s > 1:
            edges.append(_random_tree(rng, mem))
            extra = int(rng.integers(0, 3))
            if s > 2 and extra:
                edges.append(np.stack([rng.choice(mem, extra), rng.choice(mem, extra)], axis=1))          # cycle edges (a self edge now and then)
        awake.append(c % 2 == 0)
        if awake[-1]:
            idle[int(rng.choice(mem))] = (0, 1, 0xfe)[int(rng.integers(0, 3))]
    e = np.concatenate(edges)
    e = e[rng.permutation(len(e))]
    return e, idle, comps, np.array(awake)


def _confetti_case(n):
    e, idle, comps, awake = _confetti(n)
    on = int(sum(len(c) for c, a in zip(comps, awake) if a))
    return e, [_phase("every second component holds one awake member", idle, active=on, contacts=on, sleeping=n - on)]


def _noise(n):
    e, idle, comps, awake = _confetti(n)
    rng = np.random.default_rng(54)
    on = int(sum(len(c) for c, a in zip(comps, awake) if a))
    big = [k for k, c in enumerate(comps) if len(c) > 4]
    wake, sleep = [k for k in big if awake[k]][0], [k for k in big if not awake[k]][0]
    zero = []
    for k in (wake, sleep):
        m = comps[k]
        zero += [(0, int(m[0])), (int(m[1]), 0), (0, int(m[-1]))]
    selfs = rng.integers(1, n + 1, size=n // 16)
    e = np.concatenate([e, e[:, ::-1], np.stack([selfs, selfs], axis=1), np.array(zero), np.array([(0, 0)])])
    e = e[rng.permutation(len(e))]
    return e, [_phase("confetti with self edges, doubled edges and edges to body 0", idle, active=on, contacts=on, sleeping=n - on)]


def _awake_bridges(n):
    rng = np.random.default_rng(55)
    idle = _idle(n, 0xff)
    edges = []
    label = rng.permutation(n) + 1
    at, kind, on = 0, 0, 0
    awake_values = (0, 0, 1, 0x7f, 0xfe)
    while at + 4 <= n - n // 10:                   # (the last tenth: lone sleepers)
        pattern = ("SAAS", "SAS", "ASSA")[kind % 3]
        mem = label[at:at + len(pattern)]; at += len(pattern)
        for m, p in zip(mem, pattern):
            if p == "A":
                idle[int(m)] = awake_values[int(rng.integers(0, len(awake_values)))] if kind % 2 else 0
        path = np.stack([mem[:-1], mem[1:]], axis=1)
        edges.append(path[::-1] if kind % 4 == 1 else path)
        on += len(pattern); kind += 1
    e = np.concatenate(edges)
    e = e[rng.permutation(len(e))]
    return e, [_phase("paths of sleepers and awake bodies", idle, active=on, contacts=on, sleeping=n - on)]


def _nobody_asleep(n):
    e, _, _, _ = _confetti(n, seed=56)
    idle = (np.arange(n + 1) % 0xff).astype(np.uint8)          # every value but 0xff
    idle[0] = 0
    return e, [_phase("nobody asleep", idle, **_everybody(n))]


def _all_asleep(n):
    return np.zeros((0, 2), dtype=np.uint32), [_phase("everybody asleep", _idle(n, 0xff), **_nobody(n))]


_GRAPHS = {"chain_up": lambda n: _chain(n, "up"), "chain_down": lambda n: _chain(n, "down"), "chain_shuffled": lambda n: _chain(n, "shuffled"), "star": _star, "tree": _tree,
           "two_giants": _two_giants, "confetti": _confetti_case, "noise": _noise, "awake_bridges": _awake_bridges, "nobody_asleep": _nobody_asleep,
           "all_asleep_no_edges": _all_asleep}


def graph_lists(scene):
    """The pairs and contacts of a graph world, known by construction: (pairs (n, 2) collider indices, dict(keys, features, bodies))."""
    n = scene["isl"]["n"]
    k = np.arange(1, n + 1, dtype=np.uint64)
    pairs = np.stack([np.zeros(n, dtype=np.int64), k.astype(np.int64)], axis=1)
    return pairs, dict(keys=k << np.uint64(32), features=np.zeros(n, dtype=np.uint32), bodies=np.stack([np.zeros(n, dtype=np.uint32), k.astype(np.uint32)], axis=1))


# ---- geometry worlds -------------------------------------------------------------------------------------------------------------------------------------------------------
ASLEEP = 0xff


def _ground(b, half=12.0, ballast=False):
    b.box((0.0, -3.0, 0.0), (0.25, 0.25, 0.25), body=0)                     # collider 0: touches nobody (module docstring)
    slab = b.box((0.0, -0.5, 0.0), (half, 0.5, half), body=0)             # the slab, top face at y = 0
    if ballast:
        # 72 static boxes of extent 2 far below: more than the 64 colliders the broadphase treats as "large", all of a size class above the spheres', so the spheres
        # are grid members and their pairs come from k_find_pairs -- where the DIRECT search applies spheres_surely_apart -- and not from the large-collider loops
        for i in range(72):
            b.box((3.0 * (i % 9) - 12.0, -10.0, 3.0 * (i // 9) - 12.0), (1.0, 1.0, 1.0), body=0)
    return slab


def _rest(r):
    return r - PUSH                                                             # centre height of a shape of half height r resting on the slab, pushed in by 2^-6


def _near_miss_spheres(b):
    slab = _ground(b, ballast=True)
    s = b.sphere((0.0, _rest(0.5), 0.0), 0.5, idle=ASLEEP)
    a = b.sphere((0.75, _rest(0.5) + 0.75, 0.75), 0.5)
    return dict(near=[(s, a)], touch=[(slab, s)], expect=dict(active=1, contacts=0, sleeping=1, fine=1))


def _near_miss_boxes(b):
    slab = _ground(b)
    q = _quat((0, 1, 0), np.pi / 4)
    s = b.box((0.0, _rest(0.5), 0.0), (0.5, 0.5, 0.5), rot=q, idle=ASLEEP)
    a = b.box((0.75, _rest(0.5) + 0.25, 0.75), (0.5, 0.5, 0.5), rot=q)
    return dict(near=[(s, a)], touch=[(slab, s)], expect=dict(active=1, contacts=0, sleeping=1, fine=1))


def _near_miss_chain(b):
    slab = _ground(b, ballast=True)
    s = [b.sphere((0.75 * i - 4.0, _rest(0.5), 0.75 * (i % 2)), 0.5, idle=ASLEEP) for i in range(12)]
    a = b.sphere((0.75 * 12 - 4.0, _rest(0.5) + 0.25, 0.0), 0.5, idle=3)
    return dict(near=list(zip(s[:-1], s[1:])) + [(s[-1], a)], touch=[(slab, x) for x in s], expect=dict(active=1, contacts=0, sleeping=12, fine=12))


def _touching(b):
    slab = _ground(b)
    s = b.sphere((0.0, _rest(0.5), 0.0), 0.5, idle=ASLEEP)
    a = b.sphere((0.75, _rest(0.5), 0.0), 0.5)
    return dict(near=[], touch=[(slab, s), (slab, a), (s, a)], expect=dict(active=2, contacts=3, sleeping=0, fine=0))


def _heap(b):
    slab = _ground(b)
    pitch = 1.125
    boxes, tops, near, touch = {}, {}, [], []
    for j in range(3):
        for i in range(4):
            x, z = pitch * i - 2.0, pitch * j - 1.0
            boxes[i, j] = b.box((x, _rest(0.5), z), (0.5, 0.5, 0.5), rot=_quat((0, 1, 0), 0.2 + 0.01 * (4 * j + i)), idle=ASLEEP)
            tops[i, j] = b.sphere((x, _rest(0.5) + 0.5 + _rest(0.5), z), 0.5, idle=ASLEEP)
            touch += [(slab, boxes[i, j]), (boxes[i, j], tops[i, j])]
    yb = _rest(0.5) + 0.5 + _rest(0.5) + 0.6875
    for j in range(3):
        for i in range(4):
            x, z = pitch * i - 2.0, pitch * j - 1.0
            if i < 3:
                near.append((boxes[i, j], boxes[i + 1, j]))
                m = b.sphere((x + pitch / 2, yb, z), 0.5, idle=ASLEEP)
                touch += [(m, tops[i, j]), (m, tops[i + 1, j])]
            if j < 2:
                near.append((boxes[i, j], boxes[i, j + 1]))
                m = b.sphere((x, yb, z + pitch / 2), 0.5, idle=ASLEEP)
                touch += [(m, tops[i, j]), (m, tops[i, j + 1])]
    for i, j in ((0, 0), (3, 0), (1, 2)):                                       # small boxes on a corner of a box's top face, beside the sphere on it
        c = b.box((pitch * i - 2.0 + 0.25, 2.0 * _rest(0.5) + _rest(0.125), pitch * j - 1.0 + 0.25), (0.125, 0.125, 0.125), idle=ASLEEP)
        touch.append((c, boxes[i, j]))
    return slab, boxes, near, touch


def _sleeping_heap(b):
    _, _, near, touch = _heap(b)
    return dict(near=near, touch=[], asleep_touch=touch, expect=dict(active=0, contacts=0, fine=0))


def _far_connection(b):
    _, boxes, near, touch = _heap(b)
    far = b.sphere((9.0, 5.0, -9.0), 0.5, idle=0)
    return dict(near=near, touch=touch, connections=[(b.body_of(boxes[2, 1]), b.body_of(far))], expect=dict(active=len(b.body_pos) - 1, sleeping=0, fine=0))


def _compound(b):
    slab = _ground(b)
    y = _rest(0.5)
    one = b.body((0.0, y, 0.0), idle=ASLEEP)
    c0, c1 = b.sphere((-1.5, 0.0, 0.0), 0.5, body=one), b.box((1.5, 0.0, 0.0), (0.5, 0.5, 0.5), body=one)
    a = b.sphere((1.5, y + 0.9375, 0.0), 0.5)                                   # rests on the box of `one`
    two = b.body((0.0, y, 6.0), idle=ASLEEP)
    d0, d1 = b.sphere((-1.5, 0.0, 0.0), 0.5, body=two), b.box((1.5, 0.0, 0.0), (0.5, 0.5, 0.5), rot=_quat((0, 1, 0), np.pi / 4), body=two)
    a2 = b.box((1.5 + 0.75, y + 0.25, 6.0 + 0.75), (0.5, 0.5, 0.5), rot=_quat((0, 1, 0), np.pi / 4), idle=1)          # AABB overlap only
    return dict(near=[(d1, a2)], touch=[(slab, c0), (slab, c1), (c1, a)], asleep_touch=[(slab, d0), (slab, d1)], expect=dict(active=3, sleeping=2, fine=2))


_GEOMETRY = {"near_miss_spheres": _near_miss_spheres, "near_miss_boxes": _near_miss_boxes, "near_miss_chain": _near_miss_chain, "touching": _touching,
             "sleeping_heap": _sleeping_heap, "far_connection": _far_connection, "compound": _compound}


def _geometry_scene(case):
    b = _Builder()
    info = _GEOMETRY[case](b)
    b.freeze()
    idle = np.array(b.idle, dtype=np.uint8)
    pr = lambda prs: [tuple(sorted((b.idx(x), b.idx(y)))) for x, y in prs]
    phases = [_phase("first: the search unites", idle, **info["expect"]), _phase("again, nothing moved: the kept list's filter unites", idle.copy(), **info["expect"])]
    scene = b.scene(case, "geometry", "host", phases)
    del scene["bp"]
    scene["name"] = f"island_{case}"
    scene["connections"] = np.asarray(info.get("connections", []), dtype=np.uint32).reshape(-1, 2)
    scene["isl"] = dict(kind="geometry", oracle="host", phases=phases, near=pr(info["near"]), touch=pr(info["touch"]), asleep_touch=pr(info.get("asleep_touch", [])))
    return scene


_CACHE = {}


def world(case, n=None):
    """The scene of `case` (graph worlds: with `n` bodies, default N_DEFAULT), built once per process; treat it as read-only."""
    key = (case, n)
    if key not in _CACHE:
        if case in _GRAPHS:
            size = n or N_DEFAULT
            edges, phases = _GRAPHS[case](size)
            _CACHE[key] = _graph_scene(case, size, edges, phases)
        else:
            assert n is None
            _CACHE[key] = _geometry_scene(case)
    return _CACHE[key]


def forget(case, n=None):
    _CACHE.pop((case, n), None)


def ncolliders(scene):
    return len(scene["box_tags"]) + len(scene["sphere_tags"])


def owners(scene):
    return np.concatenate([scene["box_transforms"]["body"], scene["sphere_transforms"]["body"]]).astype(np.int64)


def lists(scene):
    """(pairs, contacts) of a world: by construction (graph worlds) or from the brute-force host build."""
    if scene["isl"]["oracle"] == "list":
        return graph_lists(scene)
    import hostsim_util as H
    h = H.collide(scene["body_transforms"], scene, cap=1 << 16)
    return H.pairs(scene["body_transforms"], scene).astype(np.int64), dict(keys=h["keys"], features=h["features"], bodies=h["bodies"], data=h["data"])


def expected(scene, phase, pairs=None, contacts=None, sleeping_end_only=False):
    """The oracle's verdict on one phase: dict(active, tags, features, bodies, keep, sleeping, coarse_sleeping, fine_sleeping)."""
    if pairs is None:
        pairs, contacts = lists(scene)
    tags = np.concatenate([scene["box_tags"], scene["sphere_tags"]])
    o = islands(len(scene["body_transforms"]), owners(scene), tags, pairs, contacts, scene["connections"], phase["idle"], sleeping_end_only)
    keep = o["keep"]
    o.update(tags=contacts["keys"][keep], features=contacts["features"][keep], bodies=np.asarray(contacts["bodies"], dtype=np.uint32).reshape(-1, 2)[keep])
    if "data" in contacts:
        o["data"] = contacts["data"][keep]
    return o


# ---- crafted caches --------------------------------------------------------------------------------------------------------------------------------------------------------
def _entries(tags, features):
    """A cache of the given keys, sorted by (tag, feature), payload by final index."""
    t, f = np.asarray(tags, dtype=np.uint64), np.asarray(features, dtype=np.uint32)
    order = np.lexsort((f, t))
    t, f = t[order], f[order]
    assert len(set(zip(t.tolist(), f.tolist()))) == len(t), "duplicate keys"
    d = np.zeros(len(t), dtype=S.IMPULSE)
    i = np.arange(len(t), dtype=np.float64)
    d["impulse"] = np.stack([3 * i + 1, 3 * i + 2, 3 * i + 3], axis=1).astype(F)
    return dict(count=len(t), tags=t, features=f, data=d)


def crafted_caches(scene, o, capacity):
    """name -> cache for a world whose collide() left the contacts o["tags"] / o["features"] (the list L) and the sleeping pairs o["sleeping"].  Foreign entries (for nobody)
    carry tags of colliders that do not exist: C + j in the low word and nothing in the high word puts them below every live tag (every live key has a high word >= 1),
    (C + j) << 32 | 0xFFFF behind every entry whose high word is a collider's."""
    lt, lf = np.asarray(o["tags"], dtype=np.uint64), np.asarray(o["features"], dtype=np.uint32)
    sl = np.asarray(o["sleeping"], dtype=np.uint64)
    C = ncolliders(scene)
    assert len(lt) == 0 or int(lt.min()) >= 1 << 32
    front = lambda k: (np.arange(C, C + k, dtype=np.uint64), np.arange(k, dtype=np.uint32) % 3)
    cat = lambda *parts: _entries(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    out = {"same": cat((lt, lf)), "empty": cat((lt[:0], lf[:0])), "short": cat((lt[:len(lt) // 4], lf[:len(lt) // 4]))}
    for k in (1, 5, 300):
        out[f"shifted_{k}"] = cat(front(k), (lt, lf))
    # behind every third body's entries: same tag word region, a feature beyond the last (0xFFFFFFFF is no contact's feature) -- misses on both sides of a window
    uniq = np.unique(lt)[::3]
    out["shifted_back"] = cat(front(5), (lt, lf), (uniq, np.full(len(uniq), 0xFFFFFFFF, dtype=np.uint32)))
    hole = np.ones(len(lt), dtype=bool); hole[::3] = False
    out["holes"] = cat((lt[hole], lf[hole]))
    # the right tag, features no contact has (contacts' features are 0 or 0xFFFFxxxx / small words: 0x7F000000 + r is nobody's), in runs of 1 .. 4
    ut = np.unique(lt)
    run = 1 + np.arange(len(ut)) % 4
    ft = np.repeat(ut, run)
    ff = (np.uint32(0x7F000000) + (np.arange(len(ft)) - np.repeat(np.cumsum(run) - run, run)).astype(np.uint32)).astype(np.uint32)
    assert not (set(zip(ft.tolist(), ff.tolist())) & set(zip(lt.tolist(), lf.tolist())))
    out["feature_only"] = cat((ft, ff))
    out["only_foreign"] = cat(front(40))
    room = max(0, capacity - len(lt) - len(sl) * 4 - 8)
    room = min(room, 60000 - C)                                # (foreign tags stay below 2^16 for the reference)
    behind = (np.arange(C, C + room // 2, dtype=np.uint64) << np.uint64(32)) | np.uint64(0xFFFF)
    out["long"] = cat(front(room - room // 2), (lt, lf), (behind, np.zeros(len(behind), dtype=np.uint32)))
    # entries for every sleeping pair, 1 .. 4 features each, among the live entries
    run = 1 + np.arange(len(sl)) % 4
    st_ = np.repeat(sl, run)
    sf = (np.arange(len(st_)) - np.repeat(np.cumsum(run) - run, run)).astype(np.uint32) * np.uint32(0x10001)
    out["sleepers"] = cat((lt, lf), (st_, sf))
    # both word orders of every sleeping pair: only the order that equals the sleeping-pair word is kept
    swapped = (sl >> np.uint64(32)) | ((sl & np.uint64(0xFFFFFFFF)) << np.uint64(32))
    both = np.unique(np.concatenate([sl, swapped]))
    out["sleepers_quirk"] = cat((lt, lf), (both, np.full(len(both), 7, dtype=np.uint32)))
    for c in out.values():
        assert c["count"] <= capacity
    return out


def narrow_cache(cache):
    """A wide cache (tags a | b << 32, features) in the reference's format (feature | (a16 | b16 << 16) << 32): the inverse of the widening the parity tests apply."""
    t = np.asarray(cache["tags"], dtype=np.uint64)
    a, b = t & np.uint64(0xFFFFFFFF), t >> np.uint64(32)
    assert (a < 65536).all() and (b < 65536).all()
    return ((a | (b << np.uint64(16))) << np.uint64(32)) | np.asarray(cache["features"], dtype=np.uint64)


def widen_cache(rc):
    t = rc["tags"]
    hi = t >> np.uint64(32)
    return (hi & np.uint64(0xFFFF)) | ((hi >> np.uint64(16)) << np.uint64(32)), (t & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def tie_script(scene, o):
    """The tie rule of write_cached_impulses (a culled entry precedes a contact of equal key), which a world's own lists cannot reach: in near_miss_chain three custom
    contacts between the static world and the awake sphere A are appended behind collide()'s (empty) list, carrying the tag words of three SLEEPING pairs and feature 0,
    and the cache holds entries of exactly those keys among entries for every sleeping pair.  The entries are kept aside (their tag is a sleeping-pair word), the contacts
    find them as their warm start, and the merge meets three pairs of equal keys.  Returns (contacts = dict(data, bodies, tags, features), cache)."""
    assert scene["name"] == "island_near_miss_chain"
    sl = np.asarray(o["sleeping"], dtype=np.uint64)
    assert len(sl) == 12 and len(o["tags"]) == 0
    tags = sl[[0, 5, 11]]
    a = len(scene["body_transforms"]) - 1                       # the awake sphere's body
    data = np.zeros(3, dtype=S.CONTACT)
    data["position"] = scene["body_transforms"]["position"][a] - np.array([0.0, 0.5, 0.0], dtype=F)
    data["position"][:, 0] += np.array([0.0, 0.125, -0.125], dtype=F)
    data["normal"] = (0.0, 1.0, 0.0); data["penetration"] = 0.0078125; data["friction"] = 0.5
    bodies = np.array([[0, a]] * 3, dtype=np.uint32)
    cache = _entries(np.concatenate([sl, sl[::2]]), np.concatenate([np.zeros(len(sl), dtype=np.uint32), np.full(len(sl[::2]), 5, dtype=np.uint32)]))
    return dict(data=data, bodies=bodies, tags=tags, features=np.zeros(3, dtype=np.uint32)), cache


def restore_cache(w, cache, pristine=None):
    """A checkpoint of the live world `w` (nudge_amd.engine.World) with the crafted cache in place of its own, restored: cache_count plus device tensors for kt, kf, kd; the
    body arrays are those of `pristine` (a snapshot taken before anything ran) or, without one, the world's own, unchanged."""
    torch = w.torch
    snap = pristine if pristine is not None else w.snapshot()
    arrays = dict(snap["arrays"])
    for name, arr in (("kt", np.asarray(cache["tags"], dtype=np.uint64)), ("kf", np.asarray(cache["features"], dtype=np.uint32)), ("kd", np.asarray(cache["data"], dtype=S.IMPULSE))):
        t = torch.zeros_like(arrays[name])
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        if raw.size:
            t[:raw.size] = torch.from_numpy(raw.copy()).to(t.device)
        arrays[name] = t
    w.restore(dict(cache_count=int(cache["count"]), arrays=arrays))
    w.cache.count = int(cache["count"])
