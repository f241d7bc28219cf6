"""Distance queries on the GPU (pytest -m gpu): nh_distance (include/nudge_hip.h, "scene queries").

The oracle is a brute force over every collider on the host with the same arithmetic (nudge_amd/csrc/nh_query.h, "distance", through
tests/hostdistance_util.py) and the header's exact rules -- the overlap record, the key under the reach rule, ties -- so the tree walk's answer must
equal it in every byte of every record.  The float64 checks of that arithmetic are tests/test_cpu_distance.py's.  Queries are observers like the other
queries."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostdistance_util as D               # noqa: E402
import hostpoint_util as HP                 # noqa: E402
import hostquery_util as Q                  # noqa: E402
from query_util import OBSERVED, SMALL, bounds as _bounds, same_stepped_world as _same_stepped_world, unit_quats, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
FUSED = E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP
SHAPES = ("sphere", "box", "capsule")
# queries per kind of centre: the box / box pair function is ~150 segment tests, and the host's brute force runs it against every box of the scene
PER_KIND = {"sphere": 5461, "box": 700, "capsule": 5461}


def _centres(rng, n, rec, lo, hi, kind):
    """`kind`: near collider centres (inside piles: overlaps); uniform over the scene's bounds; 20 above the world (far from everything)."""
    live = rec["p"][np.isfinite(rec["p"]).all(axis=1)].astype(np.float64)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    span = np.maximum(hi - lo, 1.0)
    if kind == "inside":
        return live[rng.integers(0, len(live), size=n)] + rng.normal(scale=0.3, size=(n, 3))
    if kind == "uniform":
        return rng.uniform(lo - 0.2 * span, hi + 0.2 * span, size=(n, 3))
    p = rng.uniform(lo, hi, size=(n, 3))
    p[:, 1] = hi[1] + 20.0
    return p


def _body_size(rec):
    """One body size of a world: twice the median of its colliders' largest half extent."""
    h = rec["h"][np.isfinite(rec["p"]).all(axis=1)]
    return 2.0 * float(np.median(h.max(axis=1))) if len(h) else 1.0


def _shaped(rng, shape, centres, size, max_distance=np.inf, ignore_body=NONE):
    """Queries of one shape at `centres`: sizes up to half a body size, rotations random -- every fourth the identity."""
    n = len(centres)
    rot = unit_quats(rng, n)
    rot[::4] = (0, 0, 0, 1)
    half = 0.5 * size
    if shape == "sphere":
        return D.queries(centres, radii=rng.uniform(0.1, 1.0, n) * half, max_distance=max_distance, ignore_body=ignore_body)
    if shape == "box":
        return D.queries(centres, half_extents=rng.uniform(0.1, 1.0, (n, 3)) * half, rotations=rot, max_distance=max_distance, ignore_body=ignore_body)
    return D.queries(centres, radii=rng.uniform(0.1, 0.6, n) * half, half_heights=rng.uniform(0.0, 1.0, n) * half, rotations=rot, max_distance=max_distance,
                     ignore_body=ignore_body)


def _batches(rng, shape, rec, n=None):
    """The batches of one shape on one world: {what: queries}.  Centres inside piles, uniform over the bounds and 20 above the world, each with
    max_distance +inf or one body size; and a batch near the colliders that ignores a random body per query."""
    lo, hi = _bounds(rec)
    size = _body_size(rec)
    n = n or PER_KIND[shape]
    out = {}
    for kind in ("inside", "uniform", "above"):
        out[kind] = _shaped(rng, shape, _centres(rng, n, rec, lo, hi, kind), size, max_distance=rng.choice(np.float32([np.inf, size]), size=n))
    c = _centres(rng, n, rec, lo, hi, "inside")
    out["ignoring"] = _shaped(rng, shape, c, size, max_distance=rng.choice(np.float32([np.inf, size]), size=n),
                              ignore_body=rng.integers(0, int(rec["body"].max()) + 1, size=n))
    return out


def shares(queries, ref):
    """(overlap records, separated hits, misses under a finite max_distance) as shares of a batch's records."""
    hit = ref["shape"] != NONE
    unit = (ref["normal"] != 0).any(axis=1)
    return np.array([(hit & ~unit).mean(), (hit & unit).mean(), (~hit & np.isfinite(queries["max_distance"])).mean()])


def _distance(w, queries):
    raw = w.distance_records(_upload(w, queries))
    return np.frombuffer(raw.cpu().numpy().tobytes(), dtype=E.POINT_HIT).copy()


def _same_hits(got, ref, what):
    bad = (got.view(np.uint8).reshape(-1, 48) != ref.view(np.uint8).reshape(-1, 48)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(ref)} hit records differ, first at {int(np.argmax(bad))}: {got[bad][:1]} vs {ref[bad][:1]}"


def _check_world(w, scene, rng, what):
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    for shape in SHAPES:
        b = _batches(rng, shape, rec)
        q = np.concatenate(list(b.values()))
        ref = D.distance(rec, w.nbox, q)
        _same_hits(_distance(w, q), ref, f"{what} / {shape}")
        # the invariant: a unit normal iff the record is a separated one, and nothing ignored is reported
        hit = ref["shape"] != NONE
        unit = np.abs(np.linalg.norm(ref["normal"].astype(np.float64), axis=1) - 1) < 1e-5
        assert np.all(unit[hit] == (ref["distance"][hit] > 0)) and np.all(ref["normal"][~unit] == 0)
        assert not (hit & (ref["body"] == q["ignore_body"])).any()
        s = shares(q, ref)
        assert s[0] >= 0.05 and s[1] >= 0.05 and s[2] >= 0.01, (what, shape, s)


# ---- 6. bytes against the brute force ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SMALL))
def test_distances_equal_the_brute_force_before_and_after_stepping(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(900 + sorted(SMALL).index(name))
    w = E.World(scene, flags=FUSED)
    _check_world(w, scene, rng, f"{name} initial")
    w.step(50)
    _check_world(w, scene, rng, f"{name} after 50 steps")
    w.close()


def _mixed(rng, rec, n):
    """n queries of all three shapes mixed in one batch, with every kind of invalid query among them."""
    parts = [b for shape in SHAPES for b in _batches(rng, shape, rec, n=(n + 11) // 12).values()]
    q = np.concatenate(parts)[:n]
    q = q[rng.permutation(len(q))]
    bad = rng.choice(n, size=n // 16, replace=False)
    for j, i in enumerate(bad):
        k = j % 6
        if k == 0:
            q["shape"][i] = 5
        elif k == 1:
            q["center"][i, j % 3] = np.nan
        elif k == 2:
            q["size"][i, 0] = -0.5
        elif k == 3:
            q["max_distance"][i] = np.nan
        elif k == 4:
            q["max_distance"][i] = -1.0
        elif q["shape"][i] != E.NH_SHAPE_SPHERE:
            q["size"][i, 1] = np.inf
    return q


# ---- 7. tails and guards ----------------------------------------------------------------------------------------------------------------------
def test_tails_guards_and_mixed_batches():
    import torch
    scene = SMALL["pile"]()
    w = E.World(scene, flags=FUSED)
    w.step(20)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    rng = np.random.default_rng(910)
    for count in (1, 63, 65, 257, 1000):
        q = _mixed(rng, rec, count)
        assert len(q) == count
        hits = torch.full((count + 2, 48), 0xAB, dtype=torch.uint8, device=w.dev)
        w.distance_records(_upload(w, q), hits=hits)
        raw = hits.cpu().numpy()
        assert (raw[count:] == 0xAB).all(), f"count {count}: bytes behind hits[count] were written"
        ref = D.distance(rec, w.nbox, q)
        _same_hits(np.frombuffer(raw[:count].tobytes(), dtype=E.POINT_HIT), ref, f"count {count}")
        if count >= 257:
            assert np.isnan(ref["distance"]).sum() >= count // 24
    # count = 0 launches nothing
    hits = torch.full((4, 48), 0xAB, dtype=torch.uint8, device=w.dev)
    assert w.L.nh_distance(w.ctx, C.c_void_p(hits.data_ptr()), 0, C.c_void_p(hits.data_ptr()), 0) == 0
    assert w.L.nh_distance(w.ctx, None, 0, None, 0) == 0
    w.torch.cuda.synchronize()
    assert (hits.cpu().numpy() == 0xAB).all()
    w.close()


# ---- 8. identities ---------------------------------------------------------------------------------------------------------------------------
def test_identities_on_the_device():
    scene = SMALL["pile"]()
    w = E.World(scene, flags=FUSED)
    w.step(30)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(920)
    n = 8192
    c = np.concatenate([_centres(rng, n // 2, rec, lo, hi, "inside"), _centres(rng, n // 2, rec, lo, hi, "uniform")]).astype(np.float32)
    md = rng.choice(np.float32([np.inf, 0.5, 2.0]), size=n)
    ign = np.where(rng.random(n) < 0.3, rng.integers(0, 64, size=n), NONE).astype(np.uint32)
    # a sphere of radius 0 writes nh_closest's bytes wherever nh_closest reports distance > 0
    pq = np.zeros(n, dtype=E.POINT_QUERY)
    pq["point"], pq["max_distance"], pq["ignore_body"] = c, md, ign
    near = np.frombuffer(w.closest_records(_upload(w, pq)).cpu().numpy().tobytes(), dtype=E.POINT_HIT)
    got = _distance(w, D.queries(c, radii=0.0, max_distance=md, ignore_body=ign))
    pos = near["distance"] > 0
    assert pos.sum() > n // 8 and (near["distance"] < 0).sum() > n // 16
    assert got[pos].tobytes() == near[pos].tobytes()
    _same_hits(got, D.distance(rec, w.nbox, D.queries(c, radii=0.0, max_distance=md, ignore_body=ign)), "radius 0")
    assert got[pos].tobytes() == HP.closest(rec, w.nbox, pq)[pos].tobytes()
    # a capsule of half height 0 writes the sphere query's bytes, and its rotation is not read
    radii = rng.uniform(0, 0.5, size=n)
    sph = _distance(w, D.queries(c, radii=radii, max_distance=md, ignore_body=ign))
    cap = D.queries(c, radii=radii, half_heights=0.0, max_distance=md, ignore_body=ign)
    cap["rotation"] = np.nan
    assert _distance(w, cap).tobytes() == sph.tobytes()
    assert ((sph["shape"] != NONE) & (sph["distance"] > 0)).mean() > 0.1 and (sph["distance"] == 0).mean() > 0.05
    w.close()


# ---- 9. refit --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pile", "grid_tiles"])
def test_after_a_refit_the_bytes_are_those_of_a_fresh_build(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(930)
    w = E.World(scene, flags=FUSED)
    w.query_build()
    old = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    w.step(50)
    w.query_refit()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    q = _mixed(rng, rec, 3000)
    ref = D.distance(rec, w.nbox, q)
    assert ref.tobytes() != D.distance(old, w.nbox, q).tobytes()          # (the world moved)
    refit = _distance(w, q)
    _same_hits(refit, ref, f"{name} refit")
    w.query_build()
    assert _distance(w, q).tobytes() == refit.tobytes()
    w.close()


# ---- 10. observers ---------------------------------------------------------------------------------------------------------------------------
def _query(w, queries_t, hits_t):
    w.query_build()
    w.distance_records(queries_t, hits=hits_t)


_COUNTERS = ("still_steps", "still_replays", "ahead_steps", "pair_steps", "asleep_steps")


@pytest.mark.parametrize("name", sorted(OBSERVED))
def test_distance_queries_between_calls_change_nothing(name):
    scene = OBSERVED[name]()
    rng = np.random.default_rng(940)
    rec = Q.records(scene["body_transforms"], scene)
    q = _mixed(rng, rec, 1024)
    # between nh_step calls
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    qt = _upload(a, q)
    ht = a.torch.empty((len(q), 48), dtype=a.torch.uint8, device=a.dev)
    done = 0
    for k in [1, 2, 3, 5, 7, 4, 8] * 10:
        k = min(k, 300 - done)
        if k <= 0:
            break
        _query(a, qt, ht)
        a.step(k)
        b.step(k)
        done += k
    _query(a, qt, ht)
    _same_stepped_world(a, b, f"{name} nh_step")
    ca, cb = a.counts(), b.counts()
    assert [ca[k] for k in _COUNTERS] == [cb[k] for k in _COUNTERS]
    if name == "grid_tiles":
        assert ca["still_steps"] > 0, ca
    a.close(); b.close()
    # between every call of the fused step
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    qt = _upload(a, q)
    ht = a.torch.empty((len(q), 48), dtype=a.torch.uint8, device=a.dev)
    for s in range(60):
        for call in ("collide", "gravity", "read_cache", "setup", "apply", "update", "write_cache", "advance"):
            _query(a, qt, ht)
            getattr(a, call)()
            getattr(b, call)()
        a.step_done(); b.step_done()
    _query(a, qt, ht)
    _same_stepped_world(a, b, f"{name} call by call")
    a.close(); b.close()


# ---- 11. return codes ------------------------------------------------------------------------------------------------------------------------
def test_return_codes():
    import torch
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    L = w.L
    rec = Q.records(scene["body_transforms"], scene)
    q = _mixed(np.random.default_rng(950), rec, 1024)
    t = _upload(w, q)
    hits = torch.zeros((1025, 48), dtype=torch.uint8, device=w.dev)
    qp, hp = t.data_ptr(), hits.data_ptr()
    assert L.nh_distance(w.ctx, C.c_void_p(qp), 1024, C.c_void_p(hp), 0) == 1          # before any build: NH_ERR_INVALID
    assert L.nh_distance(None, C.c_void_p(qp), 1024, C.c_void_p(hp), 0) == 1
    w.query_build()
    assert L.nh_distance(w.ctx, C.c_void_p(qp), 1024, C.c_void_p(hp), 1) == 1          # flags other than 0
    assert L.nh_distance(w.ctx, C.c_void_p(qp), 1024, None, 0) == 1                    # null hits / queries
    assert L.nh_distance(w.ctx, None, 1024, C.c_void_p(hp), 0) == 1
    assert L.nh_distance(w.ctx, C.c_void_p(qp + 4), 1023, C.c_void_p(hp), 0) == 1      # misaligned queries / hits
    assert L.nh_distance(w.ctx, C.c_void_p(qp), 1024, C.c_void_p(hp + 8), 0) == 1
    assert L.nh_distance(w.ctx, C.c_void_p(qp), 1 << 30, C.c_void_p(hp), 0) == 1       # count >= 2^30
    assert L.nh_distance(w.ctx, C.c_void_p(qp), 0, C.c_void_p(hp), 0) == 0             # count 0: a no-op
    w.torch.cuda.synchronize()
    assert int(hits.sum()) == 0                                                         # nothing was written
    assert L.nh_distance(w.ctx, C.c_void_p(qp), 1024, C.c_void_p(hp), 0) == 0
    w.torch.cuda.synchronize()
    assert int(hits[1024].sum()) == 0 and int(hits[:1024].sum()) > 0
    _same_hits(np.frombuffer(hits[:1024].cpu().numpy().tobytes(), dtype=E.POINT_HIT), D.distance(rec, w.nbox, q), "after the refused calls")
    w.close()


def test_the_python_wrapper_writes_the_records_it_describes():
    scene = SMALL["grid_tiles"]()
    w = E.World(scene, flags=FUSED)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(960)
    n = 1024
    c = _centres(rng, n, rec, lo, hi, "uniform").astype(np.float32)
    md = rng.choice(np.float32([np.inf, 0.25, 1.0]), size=n)
    ign = rng.integers(0, 40, size=n)
    rot = unit_quats(rng, n)
    for kw in (dict(radii=rng.uniform(0, 0.5, n).astype(np.float32)), dict(half_extents=rng.uniform(0.1, 0.5, (n, 3)).astype(np.float32), rotations=rot),
               dict(radii=rng.uniform(0, 0.3, n).astype(np.float32), half_heights=rng.uniform(0, 0.5, n).astype(np.float32), rotations=rot)):
        out = w.distance(c, max_distance=md, ignore_body=ign, synchronize=True, **kw)
        ref = D.distance(rec, w.nbox, D.queries(c, max_distance=md, ignore_body=ign, **kw))
        _same_hits(np.frombuffer(out["raw"].cpu().numpy().tobytes(), dtype=E.POINT_HIT), ref, f"distance({sorted(kw)})")
        assert np.array_equal(out["distance"].cpu().numpy().view(np.uint32), ref["distance"].view(np.uint32))
        assert np.array_equal(out["normal"].cpu().numpy(), ref["normal"]) and np.array_equal(out["point"].cpu().numpy(), ref["point"])
        for k in ("body", "collider", "shape", "tag"):
            assert np.array_equal(out[k].cpu().numpy(), ref[k].astype(np.int64)), k
    # defaults: +inf, nothing ignored, identity rotation -- every query finds a collider
    out = w.distance(c[:16], half_extents=(0.2, 0.3, 0.4), synchronize=True)
    assert (out["shape"].cpu().numpy() != NONE).all()
    _same_hits(np.frombuffer(out["raw"].cpu().numpy().tobytes(), dtype=E.POINT_HIT), D.distance(rec, w.nbox, D.queries(c[:16], half_extents=(0.2, 0.3, 0.4))),
               "distance() defaults")
    w.close()
