"""Fast bodies on the GPU (pytest -m gpu): nh_sweep and nh_sweep_limit (include/nudge_hip.h, "fast bodies").

The oracle is tests/hostoracle/hostsweep.cpp through tests/hostsweep_util.py: selection and cast records by nudge_amd/csrc/nh_query.h's own arithmetic,
the hits by a brute force over every collider, the factors and the momentum by the rule in a plain loop.  Nothing of the answer depends on the tree, so
every channel must equal the oracle byte for byte; and nh_sweep's hits must equal what the GPU's own nh_boxcast / nh_capsulecast / nh_spherecast write
for the GPU's own cast records, an identity that needs no host.  Every output buffer is pre-filled with a sentinel and carries 64 guard records behind
it that must come back untouched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cast_util as CU                       # noqa: E402
import filter_util as F                      # noqa: E402
import hostsweep_util as HS                  # noqa: E402
import list_util as LU                       # noqa: E402
import parity_util as P                      # noqa: E402
import query_util as Q                       # noqa: E402
from list_util import SENTINEL               # noqa: E402
from query_util import FUSED, NONE, OBSERVED, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
DTYPES = dict(colliders=np.dtype("<u4"), casts=E.BOX_CAST, hits=E.RAY_HIT, factors=np.dtype("<f4"))
WALKS = ("q_sweep_box", "q_sweep_ball")


# ---- the calls --------------------------------------------------------------------------------------------------------------------------------
def _buffer(w, n, name):
    import torch
    return torch.full(((n + GUARD) * DTYPES[name].itemsize,), SENTINEL, dtype=torch.uint8, device=w.dev)


def _back(buf, n, name, what):
    a = np.frombuffer(buf.cpu().numpy().tobytes(), dtype=DTYPES[name]).copy()
    assert set(a[n:].tobytes()) == {SENTINEL}, f"{what}: bytes behind the {n} records of `{name}` were written"
    return a[:n]


def _sweep(w, capacity=None, channels=E.SWEEP_CHANNELS, time_step=HS.TIME_STEP, min_travel=0.5, core=0.5, what="", keep=False):
    """dict(counts, total, channel: numpy records of the capacity) of one nh_sweep call into sentinel-filled buffers; the guards behind each must come
    back untouched.  capacity None: every collider.  keep: the device list as well (`device`), for sweep_limit_records."""
    import torch
    cap = w.nbox + w.nsph if capacity is None else capacity
    bufs = {c: _buffer(w, cap, c) for c in channels} if cap else {}
    counts = torch.full((2 + GUARD,), -1, dtype=torch.int32, device=w.dev)
    lst = w.sweep_records(time_step, min_travel, core, capacity=cap, counts=counts, **bufs)
    out = {c: _back(bufs[c], cap, c, what) for c in bufs}
    cn = counts.cpu().numpy().view(np.uint32)
    assert (cn[2:] == NONE).all(), f"{what}: words behind the two counts were written"
    out["counts"], out["total"] = cn[:2].copy(), int(cn[:2].astype(np.int64).sum())
    if keep:
        out["device"] = lst
    return out


def _same(got, ref, what, n=None):
    """The first n records (None: the total, where it fits) of every channel of `got` against `ref`, the rest of `got` still the sentinel."""
    assert np.array_equal(got["counts"], ref["counts"]), (what, got["counts"], ref["counts"])
    for c in E.SWEEP_CHANNELS:
        if c not in got:
            continue
        k = (got["total"] if got["total"] <= len(got[c]) else 0) if n is None else n
        size = DTYPES[c].itemsize
        bad = (got[c][:k].view(np.uint8).reshape(-1, size) != np.ascontiguousarray(ref[c][:k]).view(np.uint8).reshape(-1, size)).any(axis=1)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {k} records of `{c}` differ, first at {int(np.argmax(bad))}"
        assert set(got[c][k:].tobytes()) <= {SENTINEL}, f"{what}: records of `{c}` behind the first {k} were written"


def _state(w, scene):
    b = w.get_bodies()
    return Q.records(w, scene), b["transforms"], b["momentum"]


def _world(name, steps=30, seed=0, scene=None, flags=FUSED, **thrown):
    """(world, scene, records, body transforms, momentum) of HOST_WORLDS[name] after `steps` steps, thrown (HS.thrown) and built."""
    scene = CU.HOST_WORLDS[name]() if scene is None else scene
    w = E.World(scene, flags=flags)
    if steps:
        w.step(steps)
    bm = HS.thrown(np.random.default_rng(seed), len(scene["body_transforms"]), **thrown)
    w.set_bodies(momentum=bm)
    w.query_build()
    rec, bt, bm2 = _state(w, scene)
    assert bm2.tobytes() == bm.tobytes()
    return w, scene, rec, bt, bm


def _oracle(w, rec, bt, bm, **kw):
    return HS.sweep(rec, w.nbox, bt, bm, **kw)


# ---- against the host, and against the GPU's own casts -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CU.HOST_WORLDS))
def test_every_channel_equals_the_oracle_and_the_gpus_own_casts(name):
    w, scene, rec, bt, bm = _world(name, seed=900 + sorted(CU.HOST_WORLDS).index(name))
    hit = 0
    for min_travel, core in HS.PARAMS:
        what = f"{name} / min_travel {min_travel} core {core}"
        got = _sweep(w, min_travel=min_travel, core=core, what=what)
        _same(got, _oracle(w, rec, bt, bm, min_travel=min_travel, core=core), what)
        n, nb = got["total"], int(got["counts"][0])
        assert 0 < nb < n
        # without the host: the GPU's own casts on the GPU's own records
        casts, hits = got["casts"][:n], got["hits"][:n]
        CU.same_hits(hits[:nb], CU.closest(w, casts[:nb]), what + " / nh_boxcast on casts")
        balls = casts[nb:].view(E.CAPSULE_CAST)
        CU.same_hits(hits[nb:], CU.closest(w, balls), what + " / nh_capsulecast on casts")
        CU.same_hits(hits[nb:], CU.closest(w, CU.as_balls(balls)), what + " / nh_spherecast on the balls")
        hit += int((hits["shape"] != NONE).sum())
    assert hit > 20
    w.close()


def _thrown_exactly(scene, boxes, spheres, rng):
    """Momentum that selects exactly `boxes` box colliders and `spheres` sphere colliders of a pile (one collider a body): 100 m/s for those, rest
    for everybody else."""
    nb = len(scene["body_transforms"])
    bm = np.zeros(nb, dtype=S.MOMENTUM)
    box_bodies = scene["box_transforms"]["body"][scene["box_transforms"]["body"] != 0]
    sph_bodies = scene["sphere_transforms"]["body"]
    fast = np.concatenate([rng.choice(box_bodies, size=boxes, replace=False), rng.choice(sph_bodies, size=spheres, replace=False)]).astype(np.int64)
    d = rng.normal(size=(len(fast), 3))
    bm["velocity"][fast] = 100.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
    return bm


@pytest.mark.parametrize("boxes,spheres", [(1, 0), (0, 1), (63, 64), (64, 65), (65, 63), (257, 0), (0, 257), (257, 257), (0, 0)])
def test_list_lengths_that_straddle_a_wave_and_a_workgroup(boxes, spheres):
    scene = S.pile(300, 300, seed=21)
    scene["body_transforms"]["position"][1:, 1] *= 0.1                               # a denser pile: more of the sweeps hit
    w = E.World(scene, flags=FUSED)
    bm = _thrown_exactly(scene, boxes, spheres, np.random.default_rng(910 + boxes + 3 * spheres))
    w.set_bodies(momentum=bm)
    w.query_build()
    rec, bt, _ = _state(w, scene)
    what = f"{boxes} boxes, {spheres} spheres"
    got = _sweep(w, what=what, keep=True)
    assert tuple(got["counts"]) == (boxes, spheres)
    ref = _oracle(w, rec, bt, bm)
    _same(got, ref, what)
    exact = _sweep(w, capacity=boxes + spheres, what=what + " / exact capacity") if boxes + spheres else got
    _same(exact, ref, what + " / exact capacity")
    # and the limit on that list
    factors = _buffer(w, boxes + spheres + 300, "factors")
    lst = dict(got["device"], capacity=boxes + spheres) if boxes + spheres else got["device"]
    w.sweep_limit_records(lst, factors=factors if boxes + spheres else None)
    want, after = HS.sweep_limit(rec, dict(counts=ref["counts"], colliders=ref["colliders"][:ref["total"]], hits=ref["hits"][:ref["total"]]), bm)
    assert _back(factors, boxes + spheres, "factors", what).tobytes() == want.tobytes()
    assert w.get_bodies()["momentum"].tobytes() == after.tobytes()
    w.close()


def test_each_channel_alone_count_only_and_the_capacity_rule():
    w, scene, rec, bt, bm = _world("pile", seed=920)
    full = _sweep(w)
    ref = _oracle(w, rec, bt, bm)
    _same(full, ref, "all channels")
    n = full["total"]
    assert 0 < n < len(rec)
    w.enable_timing(True)
    for c in E.SWEEP_CHANNELS:
        w.kernel_times()
        got = _sweep(w, channels=(c,), what=c)
        _same(got, ref, f"{c} alone")
        w.synchronize()
        launched = {k for k, v in w.kernel_times().items() if v[1] > 0}
        assert {"q_sweep_flag", "q_sweep_gather"} <= launched
        assert (set(WALKS) <= launched) == (c == "hits"), (c, launched)                # hits == NULL: nothing walks the tree
    w.enable_timing(False)
    count_only = _sweep(w, capacity=0)
    assert np.array_equal(count_only["counts"], ref["counts"])
    short = _sweep(w, capacity=n - 1, what="one short")                              # counts true, nothing else written
    _same(short, ref, "one short", n=0)
    _same(_sweep(w, capacity=n, what="exact"), ref, "exact", n=n)
    # a list that was not written limits nobody
    lst = _sweep(w, capacity=n - 1, keep=True)["device"]
    w.sweep_limit_records(lst)
    assert w.get_bodies()["momentum"].tobytes() == bm.tobytes()
    w.close()


def _check_world(w, scene, rng, n, what, **_):
    bm = HS.thrown(rng, len(scene["body_transforms"]), lo=5.0)
    w.set_bodies(momentum=bm)
    w.query_build()
    rec, bt, _ = _state(w, scene)
    for min_travel, core in HS.PARAMS:
        _same(_sweep(w, min_travel=min_travel, core=core, what=what), HS.sweep(rec, w.nbox, bt, bm, min_travel=min_travel, core=core), what)


def test_degenerate_worlds():
    CU.degenerate_worlds(_check_world, np.random.default_rng(930), 0, 0, 0)


def test_a_world_without_colliders_counts_nothing():
    scene = S.pile(4, 0, seed=3)
    w = E.World(scene, flags=FUSED)
    w.set_counts(len(scene["body_transforms"]), 0, 0)
    w.query_build()
    got = _sweep(w, capacity=8)
    assert tuple(got["counts"]) == (0, 0) and all(set(got[c].tobytes()) == {SENTINEL} for c in E.SWEEP_CHANNELS)
    w.close()


# ---- filter, refit, determinism ------------------------------------------------------------------------------------------------------------------
def test_the_filter_off_uniform_and_per_collider_equals_the_oracle_over_the_masked_world():
    w, scene, rec, bt, bm = _world("compound", seed=940, lo=20.0)
    words = F.layers(len(rec), 941)
    whole = _sweep(w, min_travel=0.0)
    w.query_set_layers(words[:w.nbox], words[w.nbox:])
    _same(_sweep(w, min_travel=0.0), whole, "layers set, filter off")
    for mask in F.MASKS:
        w.query_filter(mask)
        got = _sweep(w, min_travel=0.0)
        _same(got, _oracle(w, rec, bt, bm, min_travel=0.0, words=words, masks=mask), f"uniform mask {mask:#x}")
        if mask == 0:
            assert (got["hits"][:got["total"]]["shape"] == NONE).all()
        elif mask == 1:
            assert got["hits"].tobytes() != whole["hits"].tobytes() and (got["hits"][:got["total"]]["shape"] != NONE).any()
    masks = np.random.default_rng(942).choice(np.uint32([0, 1, 6, 0xFFFFFFFF]), size=len(rec))      # one mask per COLLIDER, by combined index
    w.query_filter(_upload(w, masks).view(w.torch.int32))
    got = _sweep(w, min_travel=0.0)
    _same(got, _oracle(w, rec, bt, bm, min_travel=0.0, words=words, masks=masks), "per-collider masks")
    n = got["total"]
    assert (got["hits"][:n][masks[got["colliders"][:n]] == 0]["shape"] == NONE).all()
    w.query_filter(None)
    _same(_sweep(w, min_travel=0.0), whole, "filter off again")
    w.close()


def test_a_refit_gives_the_builds_bytes_on_the_new_state():
    w, scene, rec, bt, bm = _world("compound", seed=950)
    before = _sweep(w)
    w.step(40)
    w.query_refit()
    rec2, bt2, bm2 = _state(w, scene)
    refit = _sweep(w)
    _same(refit, _oracle(w, rec2, bt2, bm2), "refitted after 40 steps")
    w.query_build()
    _same(_sweep(w), refit, "build against refit")
    assert refit["casts"].tobytes() != before["casts"].tobytes()                     # (the world did move)
    w.close()


def test_two_identical_calls_give_identical_bytes():
    w, scene, rec, bt, bm = _world("pile", seed=960)
    a, b = _sweep(w), _sweep(w)
    _same(a, b, "twice")
    assert a["total"] > 0
    w.close()


# ---- the limit --------------------------------------------------------------------------------------------------------------------------------
def _limit(w, got, with_factors=True):
    n = got["total"]
    factors = _buffer(w, n, "factors") if with_factors else None
    w.sweep_limit_records(dict(got["device"], capacity=n), factors=factors)
    return _back(factors, n, "factors", "limit") if with_factors else None


@pytest.mark.parametrize("name", sorted(CU.HOST_WORLDS))
def test_the_factors_and_the_momentum_equal_the_oracle(name):
    w, scene, rec, bt, bm = _world(name, seed=970 + sorted(CU.HOST_WORLDS).index(name), lo=20.0)
    got = _sweep(w, min_travel=0.0, keep=True)
    n = got["total"]
    want, after = HS.sweep_limit(rec, dict(counts=got["counts"], colliders=got["colliders"][:n], hits=got["hits"][:n]), bm)
    factors = _limit(w, got)
    assert factors.tobytes() == want.tobytes()
    now = w.get_bodies()["momentum"]
    assert now.tobytes() == after.tobytes()
    limited = np.unique(rec["body"][got["colliders"][:n]][want < 1])
    assert len(limited) > 5 and (want == 1).sum() > 5
    others = np.setdiff1d(np.arange(len(bm)), limited)
    assert now[others].tobytes() == bm[others].tobytes()                             # bodies that are not limited keep every byte
    assert now["angular_velocity"].tobytes() == bm["angular_velocity"].tobytes() and now["unused0"].tobytes() == bm["unused0"].tobytes()
    # factors == NULL: the same momentum from the same start
    w.set_bodies(momentum=bm)
    _limit(w, got, with_factors=False)
    assert w.get_bodies()["momentum"].tobytes() == after.tobytes()
    w.close()


def test_a_body_with_a_start_overlap_and_a_later_hit_takes_the_latter():
    import torch
    w, scene, rec, bt, bm = _world("compound", seed=980, lo=50.0, spoil=False)
    got = _sweep(w, min_travel=0.0, core=1.0, keep=True)
    n = got["total"]
    bodies = rec["body"][got["colliders"][:n]]
    several = [b for b in np.unique(bodies) if (bodies == b).sum() >= 3]
    hits = got["hits"][:n].copy()
    e0, e1 = np.nonzero(bodies == several[0])[0], np.nonzero(bodies == several[1])[0]
    hits["shape"][e0], hits["t"][e0[0]], hits["t"][e0[1]], hits["t"][e0[2]] = E.NH_SHAPE_BOX, 0.0, 0.75, 0.25
    hits["shape"][e1], hits["t"][e1] = E.NH_SHAPE_BOX, 0.0
    lst = dict(got["device"], capacity=n, hits=_upload(w, hits))
    factors = torch.zeros(n, dtype=torch.float32, device=w.dev)
    w.sweep_limit_records(lst, factors=factors)
    f = factors.cpu().numpy()
    want, after = HS.sweep_limit(rec, dict(counts=got["counts"], colliders=got["colliders"][:n], hits=hits), bm)
    assert f.tobytes() == want.tobytes() and (f[e0] == 0.25).all() and (f[e1] == 1.0).all()
    now = w.get_bodies()["momentum"]
    assert now.tobytes() == after.tobytes() and now[several[1]].tobytes() == bm[several[1]].tobytes()
    w.close()


@pytest.mark.parametrize("flags", [FUSED, 0], ids=["fused", "default"])
def test_stepping_with_the_limit_on_the_device_equals_stepping_with_it_on_the_host(flags):
    scene = CU.HOST_WORLDS["pile"]()
    scene["body_momentum"]["velocity"][1:, 1] = -60.0                                # half a metre a step: the lower bodies reach the ground
    a, b = E.World(scene, flags=flags), E.World(scene, flags=flags)
    dt = scene["params"]["time_step"]
    a.query_build()
    limited = 0
    for _ in range(60):
        a.step(1)
        a.query_refit()
        lst = a.sweep_records(dt, 0.5, 0.5, capacity=a.nbox + a.nsph, colliders=True, hits=True)
        a.sweep_limit_records(lst)
        b.step(1)
        rec, bt, bm = _state(b, scene)
        ref = HS.sweep(rec, b.nbox, bt, bm, time_step=dt)
        n = ref["total"]
        factors, after = HS.sweep_limit(rec, dict(counts=ref["counts"], colliders=ref["colliders"][:n], hits=ref["hits"][:n]), bm)
        limited += int((factors < 1).sum())
        b.set_bodies(momentum=after)
    assert limited > 10
    ba, bb = a.get_bodies(), b.get_bodies()
    assert P.bits_equal(ba["transforms"], bb["transforms"]) and P.bits_equal(ba["momentum"], bb["momentum"]) and np.array_equal(ba["idle"], bb["idle"])
    a.close(); b.close()


# ---- the wall ---------------------------------------------------------------------------------------------------------------------------------
def test_the_guard_stops_bullets_at_a_thin_wall():
    """Bullets of size 0.1 -- the wall and a bullet together are 0.3 deep, less than the 0.5 the slowest travels a step -- each started half a step
    off a whole number of steps from the wall, so that without the guard its samples straddle the wall at -s / 2 and +s / 2 and no step sees a contact."""
    speeds = (60.0, 120.0, 180.0, 240.0, 300.0, 360.0, 420.0, 480.0)
    start = [-(np.floor(3.0 / (v / 120.0)) + 0.5) * (v / 120.0) for v in speeds]
    bullets = [("sphere" if i % 2 == 0 else "box", 0.1, -4.0 + i, v, x) for i, (v, x) in enumerate(zip(speeds, start))] + [("sphere", 0.1, 4.0, 2.0)]
    scene, body = HS.wall_scene(bullets)
    fast, slow = body[:-1], body[-1]
    dt = scene["params"]["time_step"]
    g, u = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    g.query_build()
    top = np.full(len(fast), -np.inf)
    for _ in range(40):
        g.query_refit()
        g.sweep(time_step=dt, limit=True)
        g.step(1)
        u.step(1)
        bg, bu = g.get_bodies(), u.get_bodies()
        top = np.maximum(top, bg["transforms"]["position"][fast, 0])
        # nothing touches the slow one in 40 steps: its bytes are the same in both worlds
        assert bg["transforms"][slow].tobytes() == bu["transforms"][slow].tobytes() and bg["momentum"][slow].tobytes() == bu["momentum"][slow].tobytes()
    assert (top <= -0.05).all(), top
    assert (np.linalg.norm(bg["momentum"]["velocity"][fast], axis=1) < 1.0).all(), bg["momentum"]["velocity"][fast]
    assert (bu["transforms"]["position"][fast, 0] > 0).all(), bu["transforms"]["position"][fast, 0]      # without the guard every one tunnels
    g.close(); u.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_abi_edge_cases():
    import torch
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    L = w.L
    bm = HS.thrown(np.random.default_rng(990), len(scene["body_transforms"]), lo=20.0)
    w.set_bodies(momentum=bm)
    rec, bt, _ = _state(w, scene)
    n = len(rec)
    counts = torch.zeros(8, dtype=torch.int32, device=w.dev)
    colliders = torch.zeros(n + 8, dtype=torch.int32, device=w.dev)
    casts = torch.zeros((n + 8, 64), dtype=torch.uint8, device=w.dev)
    hits = torch.zeros((n + 8, 32), dtype=torch.uint8, device=w.dev)
    factors = torch.zeros(n + 8, dtype=torch.float32, device=w.dev)
    cp, lp, kp, hp, fp = counts.data_ptr(), colliders.data_ptr(), casts.data_ptr(), hits.data_ptr(), factors.data_ptr()
    bodies = C.byref(w.bodies)

    def lst(counts=cp, colliders=lp, casts=kp, hits=hp, capacity=n):
        return C.byref(E.SweepList(counts, colliders, casts, hits, capacity, 0))

    def par(time_step=HS.TIME_STEP, min_travel=0.5, core=0.5):
        return C.byref(E.SweepParams(time_step, min_travel, core, 0))

    assert L.nh_sweep(w.ctx, bodies, par(), lst(), 0) == 1                            # before any build: NH_ERR_INVALID
    assert L.nh_sweep_limit(w.ctx, bodies, lst(), C.c_void_p(fp), 0) == 1
    w.query_build()
    no_bodies = C.byref(E.BodyData(None, None, None, None, w.nb))
    for bad in ((None, bodies, par(), lst(), 0), (w.ctx, None, par(), lst(), 0), (w.ctx, bodies, None, lst(), 0), (w.ctx, bodies, par(), None, 0),
                (w.ctx, bodies, par(), lst(counts=None), 0), (w.ctx, no_bodies, par(), lst(), 0),
                (w.ctx, bodies, par(), lst(counts=cp + 2), 0), (w.ctx, bodies, par(), lst(colliders=lp + 1), 0),
                (w.ctx, bodies, par(), lst(casts=kp + 8), 0), (w.ctx, bodies, par(), lst(hits=hp + 4), 0),
                (w.ctx, bodies, par(), lst(), 1), (w.ctx, bodies, par(), lst(capacity=1 << 31), 0),
                (w.ctx, bodies, par(), lst(capacity=0), 0), (w.ctx, bodies, par(), lst(cp, None, None, hp, 0), 0),
                (w.ctx, bodies, par(time_step=np.nan), lst(), 0), (w.ctx, bodies, par(time_step=np.inf), lst(), 0),
                (w.ctx, bodies, par(min_travel=-1.0), lst(), 0), (w.ctx, bodies, par(min_travel=np.nan), lst(), 0),
                (w.ctx, bodies, par(core=-0.5), lst(), 0), (w.ctx, bodies, par(core=1.5), lst(), 0), (w.ctx, bodies, par(core=np.nan), lst(), 0)):
        assert L.nh_sweep(*bad) == 1, bad
    for bad in ((None, bodies, lst(), C.c_void_p(fp), 0), (w.ctx, None, lst(), C.c_void_p(fp), 0), (w.ctx, bodies, None, C.c_void_p(fp), 0),
                (w.ctx, bodies, lst(counts=None), C.c_void_p(fp), 0), (w.ctx, no_bodies, lst(), C.c_void_p(fp), 0), (w.ctx, bodies, lst(), C.c_void_p(fp), 1),
                (w.ctx, bodies, lst(), C.c_void_p(fp + 2), 0), (w.ctx, bodies, lst(hits=hp + 8), C.c_void_p(fp), 0), (w.ctx, bodies, lst(colliders=None), C.c_void_p(fp), 0),
                (w.ctx, bodies, lst(hits=None), C.c_void_p(fp), 0), (w.ctx, bodies, lst(capacity=1 << 31), C.c_void_p(fp), 0)):
        assert L.nh_sweep_limit(*bad) == 1, bad
    torch.cuda.synchronize()
    assert int(counts.abs().sum()) == 0 and int(colliders.abs().sum()) == 0 and int(casts.sum()) == 0 and int(hits.sum()) == 0 and int(factors.abs().sum()) == 0
    assert w.get_bodies()["momentum"].tobytes() == bm.tobytes()                      # nothing was written
    # counts and colliders need 4-byte alignment only: each at an odd word offset; count only with capacity 0
    assert L.nh_sweep(w.ctx, bodies, par(), lst(cp + 4, None, None, None, 0), 0) == 0
    assert L.nh_sweep(w.ctx, bodies, par(), lst(cp + 12, lp + 4, kp, hp, n), 0) == 0
    ref = HS.sweep(rec, w.nbox, bt, bm)
    k = ref["total"]
    assert 0 < k < n
    cn = counts.cpu().numpy().view(np.uint32)
    assert np.array_equal(cn[1:3], ref["counts"]) and np.array_equal(cn[3:5], ref["counts"]) and cn[0] == 0 and not cn[5:].any()
    cl = colliders.cpu().numpy().view(np.uint32)
    assert cl[0] == 0 and np.array_equal(cl[1:1 + k], ref["colliders"][:k]) and not cl[1 + k:].any()
    gc = np.frombuffer(casts.cpu().numpy().tobytes(), dtype=E.BOX_CAST)
    gh = np.frombuffer(hits.cpu().numpy().tobytes(), dtype=E.RAY_HIT)
    assert gc[:k].tobytes() == ref["casts"][:k].tobytes() and not gc[k:].view(np.uint8).any()
    assert gh[:k].tobytes() == ref["hits"][:k].tobytes() and not gh[k:].view(np.uint8).any()
    # the limit on that list, the factors at an odd word offset; capacity 0 is a no-op
    assert L.nh_sweep_limit(w.ctx, bodies, lst(cp + 4, None, None, None, 0), None, 0) == 0
    assert L.nh_sweep_limit(w.ctx, bodies, lst(cp + 12, lp + 4, kp, hp, n), C.c_void_p(fp + 4), 0) == 0
    want, after = HS.sweep_limit(rec, dict(counts=ref["counts"], colliders=ref["colliders"][:k], hits=ref["hits"][:k]), bm)
    gf = factors.cpu().numpy()
    assert gf[0] == 0 and gf[1:1 + k].tobytes() == want.tobytes() and not gf[1 + k:].any()
    assert w.get_bodies()["momentum"].tobytes() == after.tobytes()
    w.close()


# ---- observers -----------------------------------------------------------------------------------------------------------------------------
def _observer_batch(a, scene):
    import torch
    a.query_build()
    n = a.nbox + a.nsph
    return (torch.zeros(2, dtype=torch.int32, device=a.dev), torch.empty(n, dtype=torch.int32, device=a.dev), torch.empty((n, 64), dtype=torch.uint8, device=a.dev),
            torch.empty((n, 32), dtype=torch.uint8, device=a.dev))


def _query(w, counts, colliders, casts, hits):
    w.query_refit()
    w.sweep_records(w.params["time_step"], 0.0, 0.5, capacity=w.nbox + w.nsph, counts=counts, colliders=colliders, casts=casts, hits=hits)


def test_sweeps_between_nh_step_calls_change_nothing():
    counts = LU.queries_between_nh_step_calls_change_nothing(OBSERVED["grid_tiles"], _observer_batch, _query, "grid_tiles", still=True)[0]
    assert int(counts.sum()) >= 0


def test_sweeps_between_every_call_of_the_fused_step_change_nothing():
    counts = LU.queries_between_every_call_of_the_fused_step_change_nothing(OBSERVED["pile"], _observer_batch, _query, "pile", steps=120)[0]
    assert int(counts.sum()) > 0                                                     # (something did move, and was swept)


# ---- the rate tool ----------------------------------------------------------------------------------------------------------------------------
def test_the_rate_tool_runs_on_a_rehearsal_world(tmp_path):
    """tools/fast_bodies.py end to end in a child process on 2 tiles of side 12, 2 blocks of 2 calls, the log in tmp_path: its own checks -- the hits
    against nh_boxcast's bytes, 258 entries against the oracle -- must pass, and profiles/ stays as it is."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "sweep_rates.log"
    listing = sorted(os.listdir(os.path.join(root, "profiles")))
    child = subprocess.run([sys.executable, os.path.join(root, "tools", "fast_bodies.py"), "--tiles", "2", "--side", "12", "--reps", "2", "--inner", "2",
                            "--thrown", "64", "--out", str(out)], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert child.returncode == 0, f"status {child.returncode}\n{child.stdout[-2000:]}\n{child.stderr[-4000:]}"
    assert out.read_text() == child.stdout
    last = json.loads(child.stdout.rstrip("\n").split("\n")[-1])
    cases = list(last["cases"].values())
    assert len(cases) == 3 and cases[1]["selected"] == 64 and cases[2]["selected"] == last["colliders"] - 2
    assert sorted(os.listdir(os.path.join(root, "profiles"))) == listing


# ---- Python -----------------------------------------------------------------------------------------------------------------------------------
def test_the_python_wrapper():
    import torch
    w, scene, rec, bt, bm = _world("pile", seed=995, lo=20.0)
    n = w.nbox + w.nsph
    out = w.sweep(time_step=HS.TIME_STEP, synchronize=True)
    assert out["counts"].shape == (2,) and out["counts"].dtype == torch.int64 and out["colliders"].shape == (n,) and out["colliders"].dtype == torch.int64
    assert out["casts"].shape == (n, 16) and out["casts"].dtype == torch.float32 and out["t"].shape == (n,) and out["normal"].shape == (n, 3)
    assert out["raw"].shape == (n, 32) and out["body"].dtype == torch.int64 and "factors" not in out
    ref = HS.sweep(rec, w.nbox, bt, bm)
    k = ref["total"]
    assert int(out["counts"].sum()) == k and np.array_equal(out["colliders"][:k].cpu().numpy(), ref["colliders"][:k])
    assert out["raw"][:k].cpu().numpy().tobytes() == ref["hits"][:k].tobytes() and out["t"][:k].cpu().numpy().tobytes() == ref["hits"]["t"][:k].tobytes()
    assert w.get_bodies()["momentum"].tobytes() == bm.tobytes()                      # limit=False: an observer
    lim = w.sweep(time_step=HS.TIME_STEP, limit=True, synchronize=True)
    want, after = HS.sweep_limit(rec, dict(counts=ref["counts"], colliders=ref["colliders"][:k], hits=ref["hits"][:k]), bm)
    assert lim["factors"].shape == (n,) and lim["factors"][:k].cpu().numpy().tobytes() == want.tobytes() and (want < 1).any()
    assert w.get_bodies()["momentum"].tobytes() == after.tobytes()                   # ... as the records call changes it
    assert int(w.sweep(capacity=0)["counts"].sum()) >= 0 and set(w.sweep(capacity=0)) == {"counts"}
    w.close()
