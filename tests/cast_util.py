"""What the cast tests share (tests/test_{cpu,gpu}_{query,spherecast,boxcast,capsulecast,castall,castall_shapes,castk}.py, and the filter and refit
tests that borrow their batches), written once over the shape table of tests/hostcast_util.py: cast records on the heads of rays, the batches of the
all-hits and first-k tests, the GPU calls on numpy records, the byte comparisons, the checks of an all-hits list against the single-collider oracle and
against a plain restatement, and the worlds several of the files step through."""
import functools

import numpy as np

import hostcast_util as HC
from list_util import SENTINEL, gpu_list, same_lists, sentinel_hits
from query_util import FUSED, NONE, bounds, rays as kinds_of_rays, unit_quats, upload
from nudge_amd import engine as E
from nudge_amd import scenes as S

GUARD = 64                                   # records (and count words) behind a first-k call's output that must stay the sentinel
IDENTITY = (0.0, 0.0, 0.0, 1.0)
HOST_WORLDS = {"pile": lambda: S.pile(200, 100, seed=11), "compound": lambda: S.compound(100, seed=12)}      # a few hundred mixed boxes and spheres
BOX_SIZES = np.float32([(0, 0, 0), (0.05, 0.05, 0.05), (0.5, 0.3, 0.2), (0.75, 0.75, 0.75), (3.0, 0.4, 2.0), (0.0, 0.6, 0.0)])      # up to several bodies across
CAPSULES = np.float32([(0, 0), (0.05, 0.5), (0.5, 0.5), (0.5, 0.0), (0.0, 1.0), (1.5, 2.5)])                                         # (radius, half height)
RADII = np.float32([0.0, 0.05, 0.75, 0.3])


# ---- cast records on the heads of rays ---------------------------------------------------------------------------------------------------------
def _head(rays, shape, rotation=None):
    """Records of `shape` with the rays' origin, max_t, direction and ignore_body; `rotation` (n, 4), or the identity where the shape has one."""
    c = np.zeros(len(rays), dtype=shape.record)
    for k in ("origin", "max_t", "direction", "ignore_body"):
        c[k] = rays[k]
    if "rotation" in shape.record.names:
        c["rotation"] = IDENTITY if rotation is None else rotation
    return c


def spheres(rays, radius):
    """nh_SphereCast records from rays: `radius` a number or n values."""
    c = _head(rays, HC.SPHERE)
    c["radius"] = radius
    return c


def boxes(rays, size, rotation=None):
    """nh_BoxCast records from rays: half extents `size` (a number, n values or (n, 3)), `rotation` (n, 4) or identity."""
    c = _head(rays, HC.BOX, rotation)
    size = np.asarray(size, dtype=np.float32)
    c["size"] = size.reshape(-1, 1) if size.ndim == 1 else size
    return c


def capsules(rays, radius, half_height, rotation=None):
    """nh_CapsuleCast records from rays: `radius` / `half_height` numbers or n values, `rotation` (n, 4) or identity."""
    c = _head(rays, HC.CAPSULE, rotation)
    c["radius"] = radius
    c["half_height"] = half_height
    return c


def as_balls(casts):
    """The nh_SphereCast records of capsule casts, their half heights dropped."""
    return spheres(casts, casts["radius"])


# ---- the batches of the all-hits and first-k tests ---------------------------------------------------------------------------------------------
def every_kind_of_ray(rng, n, rec):
    """The mix the query tests draw: through the scene's bounds, from inside colliders, axis-parallel, a zero direction, ignore_body set, finite and
    infinite max_t."""
    lo, hi = bounds(rec)
    span = np.maximum(hi - lo, 1.0)
    live = np.nonzero(np.isfinite(rec["p"]).all(axis=1))[0]
    r = np.zeros(n, dtype=E.RAY)
    r["max_t"] = np.inf
    r["ignore_body"] = NONE
    r["origin"] = rng.uniform(lo - 0.2 * span, hi + 0.2 * span, size=(n, 3))
    aim = rng.uniform(lo, hi, size=(n, 3))
    d = aim - r["origin"]
    r["direction"] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.25, 4.0, size=(n, 1))
    kind = np.arange(n) % 8
    inside = kind == 1                                              # from inside a collider (its centre, a little off)
    r["origin"][inside] = rec["p"][rng.choice(live, size=int(inside.sum()))] + rng.normal(scale=0.05, size=(int(inside.sum()), 3)).astype(np.float32)
    axis = kind == 2                                                # axis-parallel: two direction components exactly zero
    d = np.zeros((int(axis.sum()), 3), dtype=np.float32)
    d[np.arange(len(d)), rng.integers(0, 3, size=len(d))] = rng.choice([-1.0, 1.0], size=len(d)) * rng.uniform(0.5, 2.0, size=len(d))
    r["direction"][axis] = d
    down = kind == 3                                                # straight down through the scene
    r["origin"][down, 1] = hi[1] + 5.0
    r["direction"][down] = (0.0, -1.0, 0.0)
    zero = kind == 4                                                # a zero direction, half of them from inside a collider
    r["direction"][zero] = 0.0
    zi = np.nonzero(zero)[0][::2]
    r["origin"][zi] = rec["p"][rng.choice(live, size=len(zi))]
    ign = kind == 5
    r["ignore_body"][ign] = rec["body"][rng.choice(live, size=int(ign.sum()))]
    r["max_t"][kind == 6] = rng.uniform(0.0, 0.5 * float(np.linalg.norm(span)), size=int((kind == 6).sum()))
    r["max_t"][kind == 7] = 0.0
    return r


def mixed(rng, n, rec, lo, hi):
    """Random rays with ignore_body set on a third, finite max_t on a third, a few from inside colliders, a few invalid and a few of zero direction."""
    r = kinds_of_rays(rng, n, lo, hi, "random")
    live = np.nonzero(np.isfinite(rec["p"]).all(axis=1))[0]
    ign = rng.random(n) < 0.3
    r["ignore_body"][ign] = rec["body"][rng.choice(live, size=int(ign.sum()))]
    fin = rng.random(n) < 0.3
    r["max_t"][fin] = rng.uniform(0.0, 0.5 * float(np.linalg.norm(np.asarray(hi, np.float64) - np.asarray(lo, np.float64))), size=int(fin.sum()))
    ins = rng.choice(n, size=n // 8, replace=False)
    r["origin"][ins] = rec["p"][rng.choice(live, size=len(ins))]
    bad = rng.choice(n, size=max(4, n // 64), replace=False)
    for j, b in enumerate(bad):
        k = j % 4
        if k == 0:
            r["origin"][b, 1] = np.nan
        elif k == 1:
            r["direction"][b, 0] = np.inf
        elif k == 2:
            r["max_t"][b] = np.nan
        else:
            r["direction"][b] = 0.0
    return r


def sphere_casts(rays, radii=RADII, invalid=True):
    """nh_SphereCast records on the rays' heads: the radii in turn, and a few invalid ones."""
    c = spheres(rays, radii[np.arange(len(rays)) % len(radii)])
    if invalid:
        c["radius"][10::97], c["radius"][11::97], c["radius"][12::97], c["radius"][13::97] = -0.5, np.nan, np.inf, -0.0
    return c


def box_casts(rng, rays, sizes=BOX_SIZES, invalid=True):
    """nh_BoxCast records on the rays' heads: the sizes in turn, every other rotation random, and a few invalid records."""
    n = len(rays)
    c = _head(rays, HC.BOX)
    c["size"] = sizes[np.arange(n) % len(sizes)]
    turn = (np.arange(n) // len(sizes)) % 2 == 1
    c["rotation"][turn] = unit_quats(rng, int(turn.sum()))
    if invalid:
        bad = rng.choice(n, size=8, replace=False)
        c["size"][bad] = (0.5, 0.5, 0.5)
        c["origin"][bad[0], 2] = np.nan
        c["direction"][bad[1], 0] = np.inf
        c["size"][bad[2], 1] = -0.25
        c["size"][bad[3], 0] = np.nan
        c["size"][bad[4], 2] = np.inf
        c["rotation"][bad[5], 3] = np.nan
        c["max_t"][bad[6]] = np.nan
        c["rotation"][bad[7]] = np.nan              # ... which a size of 0 does not read: this one is a valid ray
        c["size"][bad[7]] = 0.0
    return c


def capsule_casts(rng, rays, shapes=CAPSULES, invalid=True):
    """nh_CapsuleCast records on the rays' heads: (radius, half height) in turn, every other rotation random, and a few invalid records."""
    n = len(rays)
    c = _head(rays, HC.CAPSULE)
    s = shapes[np.arange(n) % len(shapes)]
    c["radius"], c["half_height"] = s[:, 0], s[:, 1]
    turn = (np.arange(n) // len(shapes)) % 2 == 1
    c["rotation"][turn] = unit_quats(rng, int(turn.sum()))
    if invalid:
        bad = rng.choice(n, size=8, replace=False)
        c["radius"][bad], c["half_height"][bad] = 0.5, 0.5
        c["origin"][bad[0], 1] = np.inf
        c["direction"][bad[1], 2] = np.nan
        c["radius"][bad[2]] = -0.5
        c["half_height"][bad[3]] = -1.0
        c["radius"][bad[4]] = np.nan
        c["rotation"][bad[5], 0] = np.inf
        c["max_t"][bad[6]] = np.nan
        c["rotation"][bad[7]] = np.nan              # ... which a half height of 0 does not read: this one is a valid ball
        c["half_height"][bad[7]] = 0.0
    return c


def casts_through(centre, n, rng):
    """n rays towards `centre` from 20 units away, ignoring body 0."""
    r = np.zeros(n, dtype=E.RAY)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r["origin"], r["direction"], r["max_t"], r["ignore_body"] = np.float32(centre) - 20.0 * d, d, np.inf, 0
    return r


def k_rays(rng, n, rec):
    """mixed() rays, every fourth of them turned straight down through the centre of a collider (a little off): random rays through a sparse world
    seldom pierce more than three colliders, a ray down a stack or through a compound body does.  The heads keep their max_t and ignore_body."""
    lo, hi = bounds(rec)
    r = mixed(rng, n, rec, lo, hi)
    live = np.nonzero(np.isfinite(rec["p"]).all(axis=1))[0]
    down = np.nonzero((np.arange(n) % 4 == 3) & np.isfinite(r["origin"]).all(axis=1) & np.isfinite(r["direction"]).all(axis=1) & r["direction"].any(axis=1))[0]
    r["origin"][down] = rec["p"][rng.choice(live, size=len(down))] + rng.normal(scale=0.05, size=(len(down), 3)).astype(np.float32)
    r["origin"][down, 1] = hi[1] + 5.0
    r["direction"][down] = (0.0, -1.0, 0.0)
    # ... and every fourth cut short, to a few body sizes or to a twentieth of the world, where a long cast through a pile would list many: rows
    # that hits and misses share
    span = float(np.linalg.norm(hi - lo))
    for phase, reach in ((1, 2.0), (5, 0.05 * span)):
        short = np.nonzero((np.arange(n) % 8 == phase) & ~np.isnan(r["max_t"]))[0]
        r["max_t"][short] = rng.uniform(0.0, reach, size=len(short))
    return r


def wide_casts(rng, rec):
    """{shape: casts} for the world of far_and_near_scene(): rays from all over it and rays inside the small cluster, under sizes from 0 (every
    degenerate shape) and 1e-4 to 100 units."""
    rays = np.concatenate([k_rays(rng, 768, rec), every_kind_of_ray(rng, 256, rec[np.abs(rec["p"]).max(axis=1) < 0.1])])
    sizes = np.float32([(0, 0, 0), (1e-4, 1e-4, 1e-4), (5.0, 0.4, 2.0), (100.0, 100.0, 100.0), (0.0, 30.0, 0.0), (-0.0, 0.0, -0.0)])
    shapes = np.float32([(0, 0), (1e-4, 1e-4), (5.0, 0.0), (0.0, 50.0), (100.0, 25.0), (-0.0, 0.0), (1e-4, -0.0)])
    return {"ray": rays, "sphere": sphere_casts(rays, np.float32([0.0, 1e-4, 5.0, 100.0, -0.0])),
            "box": box_casts(rng, rays, sizes=sizes), "capsule": capsule_casts(rng, rays, shapes=shapes)}


# ---- worlds -------------------------------------------------------------------------------------------------------------------------------------
def host_world(name):
    """(records, nbox) of HOST_WORLDS[name] at its initial pose."""
    scene = HOST_WORLDS[name]()
    return HC.records(scene["body_transforms"], scene), len(scene["box_tags"])


def coincident(n):
    """n equal upright boxes at one position (bodies 1 .. n; the ground slab, body 0, elsewhere)."""
    scene = S.pile(n, 0, seed=3)
    scene["body_transforms"]["position"][1:] = (0.25, 3.0, -0.5)
    scene["body_transforms"]["rotation"][1:] = IDENTITY
    scene["box_data"]["size"][1:] = scene["box_data"]["size"][1]
    return scene


def far_and_near(scene, rng):
    """`scene` with half its bodies moved within 0.05 of the origin at size 1e-3, the others anywhere within 1e4 at sizes of 25 to 30."""
    nb = len(scene["body_transforms"])
    small = rng.random(nb) < 0.5
    pos = np.where(small[:, None], rng.uniform(-0.05, 0.05, size=(nb, 3)), rng.uniform(-1e4, 1e4, size=(nb, 3))).astype(np.float32)
    scene["body_transforms"]["position"][1:] = pos[1:]
    bsmall = small[scene["box_transforms"]["body"][1:]]
    scene["box_data"]["size"][1:] = np.where(bsmall[:, None], np.float32(1e-3), np.float32(30.0))
    scene["sphere_data"]["radius"] = np.where(small[scene["sphere_transforms"]["body"]], np.float32(1e-3), np.float32(25.0))
    return scene


def far_and_near_scene():
    """A world of 1e-3 .. 1e4 units on 600 boxes and 300 spheres."""
    return far_and_near(S.pile(600, 300, seed=3), np.random.default_rng(61))


def degenerate_worlds(check_world, rng, n_one, n_halves, n_coincident, **coincident_args):
    """check_world(w, scene, rng, n, what) on the ground slab alone, on the spheres and on the boxes of a pile alone, and on 4096 boxes at one
    position (with `coincident_args` on top)."""
    scene = S.pile(4, 0, seed=3)
    w = E.World(scene, flags=FUSED)
    w.set_counts(len(scene["body_transforms"]), 1, 0)          # the ground slab alone (body 0)
    check_world(w, scene, rng, n_one, "one collider")
    w.close()

    scene = S.pile(300, 300, seed=3)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    w.set_counts(nb, 0, 300)
    check_world(w, scene, rng, n_halves, "spheres only")
    w.set_counts(nb, 301, 0)
    check_world(w, scene, rng, n_halves, "boxes only")
    w.close()

    scene = S.pile(4096, 0, seed=3)
    scene["body_transforms"]["position"][1:] = (0.25, 3.0, -0.5)        # every Morton key equal but the ground's
    w = E.World(scene, flags=FUSED)
    check_world(w, scene, rng, n_coincident, "4096 coincident boxes", **coincident_args)
    w.close()


def slide_past(p, R, h, ext, a, b, sb, off):
    """(origin, direction) of a cast that slides along axis a of the resting box (p, R, h) past its face of axis b (side sb), its shape of half
    extents `ext` along the box's axes, at the touching distance + off."""
    ol, dl = np.zeros(3), np.zeros(3)
    ol[a], ol[b], dl[a] = -(h[a] + ext[a] + 2.0), sb * (h[b] + ext[b] + off), 1.0
    return p + R @ ol, R @ dl


# ---- the GPU calls on numpy records, and the byte comparisons --------------------------------------------------------------------------------------
def closest(w, casts, any_hit=False):
    """The closest-hit call of the casts' shape on the numpy records `casts`: its nh_RayHit records, back on the host."""
    raw = getattr(w, HC.shape_of(casts).call + "_records")(upload(w, casts), any_hit=any_hit)
    return np.frombuffer(raw.cpu().numpy().tobytes(), dtype=E.RAY_HIT).copy()


def same_hits(got, ref, what):
    bad = (got.view(np.uint8).reshape(-1, 32) != ref.view(np.uint8).reshape(-1, 32)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(ref)} hit records differ, first at {int(np.argmax(bad))}"


def all_hits(w, casts, capacity):
    """(offsets, hits): one all-hits call of the casts' shape with `hits` pre-filled with the sentinel (capacity records; None = count only)."""
    return gpu_list(w, HC.shape_of(casts).call + "_all_records", casts, capacity, E.RAY_HIT)


def host_all_hits(rec, nbox, casts, capacity):
    """(offsets, hits, total) of the brute force, `hits` pre-filled with the sentinel as all_hits() has them."""
    return HC.cast_all(HC.shape_of(casts), rec, nbox, casts, capacity=capacity, hits=sentinel_hits(capacity, E.RAY_HIT))


def first_record_is_the_closest_hit(w, casts, off, hits, what):
    """The contract, against the closest-hit call on the GPU itself, for every cast of the batch."""
    best = closest(w, casts)
    cnt = np.diff(off.astype(np.int64))
    full = cnt > 0
    assert (best["shape"][~full] == NONE).all(), f"{what}: {int((best['shape'][~full] != NONE).sum())} empty segments where the closest-hit call hits"
    first = hits[off[:-1][full]]
    bad = (first.view(np.uint8).reshape(-1, 32) != best[full].view(np.uint8).reshape(-1, 32)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {int(full.sum())} first records differ from the closest hit"


def same_all_hits(w, rec, casts, what, capacity=None):
    """The count-only call, then a list call with `capacity` (None: exactly the total), against the brute force; returns (offsets, hits, total)."""
    shape = HC.shape_of(casts)
    off, hits, total = same_lists(w, shape.call + "_all_records", functools.partial(HC.cast_all, shape), rec, casts, E.RAY_HIT, what, capacity, with_hits=True)
    if total and ((0 if total >= NONE else total) if capacity is None else capacity) >= total:
        first_record_is_the_closest_hit(w, casts, off, hits, what)
    return off, hits, total


def first_k(w, casts, k, with_counts=True):
    """(counts or None, hits (n, k)) of one first-k call on buffers pre-filled with the sentinel; the guards behind both must come back untouched."""
    import torch
    n = len(casts)
    ht = torch.full((n * k + GUARD, 32), SENTINEL, dtype=torch.uint8, device=w.dev)
    ct = torch.full((n + GUARD,), -1, dtype=torch.int32, device=w.dev)
    getattr(w, HC.shape_of(casts).call + "_k_records")(upload(w, casts), k, counts=ct if with_counts else None, hits=ht)
    hits = np.frombuffer(ht.cpu().numpy().tobytes(), dtype=E.RAY_HIT).copy()
    counts = ct.cpu().numpy().view(np.uint32).copy()
    assert set(hits[n * k:].tobytes()) == {SENTINEL}, f"k {k}: bytes behind record count * k were written"
    assert (counts[n:] == NONE).all() and (with_counts or (counts == NONE).all()), f"k {k}: words outside counts[0 .. count) were written"
    return (counts[:n] if with_counts else None), hits[:n * k].reshape(n, k)


# ---- an all-hits list on the host against oracles that share no code with it --------------------------------------------------------------------
def check_against_the_single_collider_oracle(rec, nbox, casts, got, single, closest, what):
    """`got` = (offsets, hits, total) of the all-hits brute force; `single(c)` = the closest-hit oracle's records with collider c alone, `closest` =
    its closest-hit records."""
    off, hits, total = got
    n, m = len(casts), len(rec)
    assert int(off[n]) == total == len(hits) or total == 0
    only = np.stack([single(c) for c in range(m)])                     # (collider, cast) records
    hit = only["shape"] != NONE
    counts = hit.sum(axis=0)
    assert np.array_equal(np.diff(off.astype(np.int64)), counts), what
    comb = hits["collider"].astype(np.int64) + np.where(hits["shape"] == E.NH_SHAPE_BOX, 0, nbox)
    for i in range(n):
        seg = slice(int(off[i]), int(off[i + 1]))
        cs = comb[seg]
        # the set, one record per collider, and each record the single-collider call's bytes
        assert np.array_equal(np.sort(cs), np.nonzero(hit[:, i])[0]), (what, i)
        assert hits[seg].tobytes() == only[cs, i].tobytes(), (what, i)
        # the order: t non-decreasing as floats, equal t in ascending combined index
        t = hits["t"][seg]
        assert not np.isnan(t).any() and (np.diff(t) >= 0).all(), (what, i)
        tie = np.diff(t) == 0
        assert (np.diff(cs)[tie] > 0).all(), (what, i)
        # the first record is the closest hit; an empty segment is a miss there
        if len(cs):
            assert hits[seg][0].tobytes() == closest[i].tobytes(), (what, i)
        else:
            assert closest[i]["shape"] == NONE, (what, i)
    return counts


def restated(counts, records, capacity):
    """offsets, the written records and the bytes behind them, from the per-cast counts and the full list: the header's rules in plain Python."""
    total = int(sum(counts))
    off = [0]
    for k in counts:
        off.append((off[-1] + int(k)) & 0xFFFFFFFF)
    out = bytearray([SENTINEL]) * (32 * max(capacity, 1))
    if total >= 0xFFFFFFFF:
        off[-1] = NONE
        return off, bytes(out)
    for i in range(len(counts)):
        if off[i + 1] <= capacity:
            out[32 * off[i]: 32 * off[i + 1]] = records[32 * off[i]: 32 * off[i + 1]]
    return off, bytes(out)


# ---- a float64 closed form ---------------------------------------------------------------------------------------------------------------------
def ball64(o, d, c, r):
    """First t >= 0 of the ray in the ball (c, r), or inf."""
    m = o - c
    a, b, cc = d @ d, m @ d, m @ m - r * r
    disc = b * b - a * cc
    if disc < 0:
        return np.inf
    t = (-b - np.sqrt(disc)) / a
    return t if t >= 0 else np.inf


def sweep_box64(o, d, r, p, R, h):
    """(hit, t, normal, feature) of the first touch of the ball (o + t d, r) with the box, in float64: the least over the 6 faces pushed out by r, the
    12 edge cylinders and the 8 corner balls.  feature: 'start', 'face', 'edge' or 'corner'."""
    ol, dl = R.T @ (o - p), R.T @ d
    if np.sum(np.maximum(np.abs(ol) - h, 0.0) ** 2) <= r * r:
        return True, 0.0, -d / np.linalg.norm(d), "start"
    best, feat = np.inf, None
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        for s in (-1.0, 1.0):
            if dl[k] != 0.0:
                t = (s * (h[k] + r) - ol[k]) / dl[k]
                x = ol + t * dl
                if t >= 0 and abs(x[i]) <= h[i] and abs(x[j]) <= h[j] and t < best:
                    best, feat = t, "face"
        for si in (-1.0, 1.0):
            for sj in (-1.0, 1.0):
                m = np.array([ol[i] - si * h[i], ol[j] - sj * h[j]])
                dd = np.array([dl[i], dl[j]])
                a, b, cc = dd @ dd, m @ dd, m @ m - r * r
                if a > 0 and b * b - a * cc >= 0:
                    t = (-b - np.sqrt(b * b - a * cc)) / a
                    if t >= 0 and abs(ol[k] + t * dl[k]) <= h[k] and t < best:
                        best, feat = t, "edge"
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            for sz in (-1.0, 1.0):
                t = ball64(ol, dl, np.array([sx, sy, sz]) * h, r)
                if t < best:
                    best, feat = t, "corner"
    if feat is None:
        return False, 0.0, None, None
    x = ol + best * dl
    v = x - np.clip(x, -h, h)
    return True, best, R @ (v / np.linalg.norm(v)), feat
