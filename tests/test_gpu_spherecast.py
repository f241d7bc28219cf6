"""Sphere casts on the GPU (pytest -m gpu): nh_spherecast (include/nudge_hip.h, "scene queries").

The oracle is a brute force over every collider on the host with the same arithmetic (nudge_amd/csrc/nh_query.h through tests/hostcast_util.py) and
the header's exact rules, so the tree's answer must equal it bit for bit in every field.  Radius 0 must give nh_raycast's bytes, a start ball that
nh_overlap finds touching something must hit at t = 0, and casts are observers like the other queries."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostcast_util as CAST                 # noqa: E402
import hostquery_util as Q                   # noqa: E402
from cast_util import closest as _sweep, degenerate_worlds, far_and_near, same_hits as _same_hits, slide_past, spheres as _casts      # noqa: E402
from query_util import FUSED, NONE, OBSERVED, SMALL, bounds as _bounds, mat, rays as _rays, same_stepped_world as _same_stepped_world, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

RADII = (0.05, 0.5, 2.0)


def _check_world(w, scene, rng, n, what, radii=RADII):
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    share = []
    for kind in ("random", "axis", "down"):
        for r in radii:
            casts = _casts(_rays(rng, n, lo, hi, kind), r)
            ref = CAST.cast(CAST.SPHERE, rec, w.nbox, casts)
            _same_hits(_sweep(w, casts), ref, f"{what} / {kind} / r {r}")
            share.append(float((ref["shape"] != NONE).mean()))
    return share


@pytest.mark.parametrize("name", sorted(SMALL))
def test_sphere_casts_equal_the_brute_force_before_and_after_stepping(name):
    scene = SMALL[name]()
    rng = np.random.default_rng(200 + sorted(SMALL).index(name))
    w = E.World(scene, flags=FUSED)
    assert max(_check_world(w, scene, rng, 16384, f"{name} initial")) > 0.05
    w.step(50)
    assert max(_check_world(w, scene, rng, 16384, f"{name} after 50 steps")) > 0.05
    w.close()


def test_degenerate_worlds():
    rng = np.random.default_rng(21)
    degenerate_worlds(_check_world, rng, 4096, 8192, 8192)

    scene = S.pile(2000, 1000, seed=3)
    far_and_near(scene, rng)
    w = E.World(scene, flags=FUSED)
    _check_world(w, scene, rng, 16384, "1e-3 .. 1e4", radii=(1e-4, 0.01, 5.0, 100.0))
    rec = Q.records(w.get_bodies()["transforms"], scene)
    for r in (1e-4, 0.01, 0.05):
        casts = _casts(_rays(rng, 16384, (-0.05,) * 3, (0.05,) * 3, "random"), r)
        _same_hits(_sweep(w, casts), CAST.cast(CAST.SPHERE, rec, w.nbox, casts), f"small cluster r {r}")
    w.close()


def test_grazing_casts_beside_resting_boxes():
    """Balls that pass a face or an edge of a resting box at r + offset, offsets 0 and +-1e-8 .. 1e-2: the walk's pruning is tested where the node test
    and the predicate are closest."""
    scene = S.stacks(64, 3, seed=5)
    w = E.World(scene, flags=FUSED)
    w.step(60)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    boxes = np.nonzero(rec["body"][: w.nbox] != 0)[0][:96]
    offs = [0.0] + [s * 10.0 ** e for e in range(-8, -1) for s in (-1.0, 1.0)]
    casts = []
    for k, c in enumerate(boxes):
        p, h = rec["p"][c].astype(np.float64), rec["h"][c].astype(np.float64)
        R = mat(rec["q"][c])
        for r in (0.05, 0.3):
            for off in offs:
                a, b = k % 3, (k + 1) % 3                    # slide along axis a past the face of axis b, and across the edge (a, b) at 45 degrees
                for sb in (-1.0, 1.0):
                    casts.append((*slide_past(p, R, h, (r, r, r), a, b, sb, off), r))
                    e = np.zeros(3)
                    e[a], e[b] = h[a], sb * h[b]
                    nrm = np.zeros(3)
                    nrm[a], nrm[b] = 1.0, sb
                    nrm /= np.sqrt(2.0)
                    tan = np.zeros(3)
                    tan[a], tan[b] = -sb, 1.0
                    tan *= sb / np.sqrt(2.0)
                    ol = e + (r + off) * nrm - 3.0 * tan
                    casts.append((p + R @ ol, R @ tan, r))
    c = np.zeros(len(casts), dtype=E.SPHERE_CAST)
    c["origin"] = [o for o, _, _ in casts]
    c["direction"] = [d for _, d, _ in casts]
    c["radius"] = [r for _, _, r in casts]
    c["max_t"] = np.inf
    c["ignore_body"] = NONE
    ref = CAST.cast(CAST.SPHERE, rec, w.nbox, c)
    _same_hits(_sweep(w, c), ref, "grazing")
    assert (ref["shape"] != NONE).mean() > 0.1          # (in a stack most casts that pass one box go on to touch its neighbours)
    w.close()


@pytest.mark.parametrize("name", ["pile", "grid_tiles", "ball_pit"])
def test_radius_zero_equals_the_ray_cast(name):
    scene = SMALL[name]()
    w = E.World(scene, flags=FUSED)
    w.step(20)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(22)
    for kind in ("random", "axis", "down"):
        rays = _rays(rng, 32768, lo, hi, kind)
        rays["max_t"][::3] = 7.0
        rays["ignore_body"][::5] = rng.integers(0, 64, size=len(rays[::5]))
        ray_hits = _sweep(w, rays)
        _same_hits(_sweep(w, _casts(rays, 0.0)), ray_hits, f"{name} / {kind}: radius 0 against nh_raycast")
    w.close()


@pytest.mark.parametrize("name", ["pile", "grid_tiles"])
def test_a_start_ball_that_overlaps_hits_at_zero(name):
    scene = SMALL[name]()
    w = E.World(scene, flags=FUSED)
    w.step(30)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(23)
    n = 32768
    rays = _rays(rng, n, lo, hi, "random")
    rays["origin"] = rng.uniform(lo, hi, size=(n, 3))
    rays["ignore_body"][::4] = rng.integers(0, 64, size=len(rays[::4]))
    radii = rng.uniform(0.05, 1.5, size=n).astype(np.float32)
    casts = _casts(rays, radii)
    got = _sweep(w, casts)
    ov = w.overlap(rays["origin"], radii=radii, ignore_body=rays["ignore_body"].astype(np.int64), synchronize=True)
    touching = np.diff(ov["offsets"].cpu().numpy()) > 0
    assert touching.mean() > 0.05, touching.mean()
    assert (got["t"][touching] == 0.0).all() and (got["shape"][touching] != NONE).all()
    _same_hits(got, CAST.cast(CAST.SPHERE, rec, w.nbox, casts), f"{name} start balls")
    w.close()


@pytest.mark.parametrize("name", ["pile", "grid_tiles"])
def test_any_hit_agrees_with_closest_hit_about_hit_or_miss(name):
    scene = SMALL[name]()
    w = E.World(scene, flags=FUSED)
    w.step(30)
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(24)
    for kind in ("random", "axis", "down"):
        rays = _rays(rng, 32768, lo, hi, kind)
        rays["max_t"] = rng.choice([np.inf, 5.0, 50.0], size=len(rays))
        casts = _casts(rays, rng.choice([0.1, 0.5, 1.5], size=len(rays)))
        closest, anyh = _sweep(w, casts), _sweep(w, casts, any_hit=True)
        assert np.array_equal(closest["shape"] == NONE, anyh["shape"] == NONE), kind
        miss = anyh["shape"] == NONE
        assert anyh[miss].tobytes() == closest[miss].tobytes()
        idx = np.nonzero(~miss)[0]
        assert len(idx) > 100
        assert (anyh["t"][idx] <= casts["max_t"][idx]).all()
        for i in idx[:: max(1, len(idx) // 500)]:
            c = int(anyh["collider"][i]) + (0 if anyh["shape"][i] == E.NH_SHAPE_BOX else w.nbox)
            one = CAST.cast(CAST.SPHERE, rec, w.nbox, casts[i:i + 1], only=c)[0]
            assert one.tobytes() == anyh[i].tobytes(), (kind, i)
    w.close()


def test_abi_edge_cases():
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    L = w.L
    casts = _casts(_rays(np.random.default_rng(25), 1024, (-5, -10, -5), (5, 300, 5), "random"), 0.5)
    t = _upload(w, casts)
    import torch
    hits = torch.zeros((1025, 32), dtype=torch.uint8, device=w.dev)
    hp = hits.data_ptr()
    assert L.nh_spherecast(w.ctx, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hp), 0) == 1          # before any build: NH_ERR_INVALID
    assert L.nh_spherecast(None, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hp), 0) == 1
    w.query_build()
    assert L.nh_spherecast(w.ctx, C.c_void_p(t.data_ptr()), 0, C.c_void_p(hp), 0) == 0            # count 0: a no-op
    assert L.nh_spherecast(w.ctx, None, 0, None, 0) == 0
    assert L.nh_spherecast(w.ctx, C.c_void_p(t.data_ptr()), 1024, None, 0) == 1                    # null hits / casts
    assert L.nh_spherecast(w.ctx, None, 1024, C.c_void_p(hp), 0) == 1
    assert L.nh_spherecast(w.ctx, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hp), 2) == 1           # unknown flags
    assert L.nh_spherecast(w.ctx, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hp), 3) == 1
    assert L.nh_spherecast(w.ctx, C.c_void_p(t.data_ptr() + 4), 1023, C.c_void_p(hp), 0) == 1       # misaligned casts / hits
    assert L.nh_spherecast(w.ctx, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hp + 8), 0) == 1
    w.torch.cuda.synchronize()
    assert int(hits.sum()) == 0                                                                   # nothing was written
    assert L.nh_spherecast(w.ctx, C.c_void_p(t.data_ptr()), 1024, C.c_void_p(hp), 1) == 0
    w.close()


# ---- observers -----------------------------------------------------------------------------------------------------------------------------
def _query(w, casts_t, hits_t):
    w.query_build()
    w.spherecast_records(casts_t, hits=hits_t)
    w.spherecast_records(casts_t, any_hit=True, hits=hits_t)


@pytest.mark.parametrize("name", sorted(OBSERVED))
def test_sphere_casts_between_calls_change_nothing(name):
    scene = OBSERVED[name]()
    casts = _casts(_rays(np.random.default_rng(26), 4096, (-30, -12, -30), (30, 20, 30), "random"), 0.5)
    # between nh_step calls
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    ct = _upload(a, casts)
    ht = a.torch.empty((4096, 32), dtype=a.torch.uint8, device=a.dev)
    done = 0
    for k in [1, 2, 3, 5, 7, 4, 8] * 10:
        k = min(k, 300 - done)
        if k <= 0:
            break
        _query(a, ct, ht)
        a.step(k)
        b.step(k)
        done += k
    _query(a, ct, ht)
    _same_stepped_world(a, b, f"{name} nh_step")
    if name == "grid_tiles":
        assert a.counts()["still_steps"] > 0, a.counts()
    a.close(); b.close()
    # between every call of the fused step
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    ct = _upload(a, casts)
    ht = a.torch.empty((4096, 32), dtype=a.torch.uint8, device=a.dev)
    for s in range(300):
        for call in ("collide", "gravity", "read_cache", "setup", "apply", "update", "write_cache", "advance"):
            _query(a, ct, ht)
            getattr(a, call)()
            getattr(b, call)()
        a.step_done(); b.step_done()
    _query(a, ct, ht)
    _same_stepped_world(a, b, f"{name} call by call")
    if name == "grid_tiles":
        assert a.counts()["still_steps"] > 0, a.counts()
    a.close(); b.close()


# ---- at size -------------------------------------------------------------------------------------------------------------------------------
def test_a_million_sphere_casts_on_the_landed_config_2_world():
    scene = S.grid_tiles(124, side=90, seed=2, lattice_cols=11)
    nb = len(scene["body_transforms"])
    n_tiles = len(scene["tile_of_static"])
    w = E.World(scene, flags=FUSED, max_contacts=6 * nb)
    w.step(70)
    assert w.counts()["error"] == 0
    w.query_build()
    rec = Q.records(w.get_bodies()["transforms"], scene)
    lo, hi = _bounds(rec)
    rng = np.random.default_rng(27)
    n = 1 << 20
    nd = n // 2
    tile = rng.integers(0, n_tiles, size=nd)
    centre = scene["box_transforms"]["position"][tile].astype(np.float64)
    half = scene["box_data"]["size"][tile, 0].astype(np.float64) - 2.5          # (a ball of radius <= 1 stays inside its tile's footprint)
    down = np.zeros(nd, dtype=E.RAY)
    down["origin"][:, 0] = centre[:, 0] + rng.uniform(-1, 1, size=nd) * half
    down["origin"][:, 1] = 20.0
    down["origin"][:, 2] = centre[:, 2] + rng.uniform(-1, 1, size=nd) * half
    down["direction"] = (0.0, -1.0, 0.0)
    down["max_t"] = np.inf
    down["ignore_body"] = NONE
    rays = np.concatenate([down, _rays(rng, n // 4, lo, hi, "random"), _rays(rng, n - nd - n // 4, lo, hi, "axis")])
    casts = _casts(rays, rng.choice(np.float32([0.25, 0.5, 1.0]), size=n))
    got = _sweep(w, casts)
    g = got[:nd]
    assert (g["shape"] != NONE).all()
    slab = g["body"] == 0
    assert (g["collider"][slab] == tile[slab]).all()
    tob = scene["tile_of_body"]
    assert (tob[g["body"][~slab]] == tile[~slab]).all()
    assert (~slab).mean() > 0.2
    # 1024 casts spread over the batch, bit for bit against the brute force over all 1,004,524 colliders
    pick = np.linspace(0, n - 1, 1024).astype(np.int64)
    _same_hits(got[pick], CAST.cast(CAST.SPHERE, rec, w.nbox, casts[pick]), "config 2, 1 M sphere casts")
    w.close()
