"""Body impulses on the GPU (pytest -m gpu): nh_impulse_sums / nh_body_impulses / nh_blast_impulses / nh_touch_impulses (include/nudge_hip.h, "body
impulses").

The oracle is tests/hostimpulse_util.py's C++ one (the per-item functions of nudge_amd/csrc/nh_impulse.h on the host around a serial stable sort;
tests/test_cpu_impulses.py holds it against an independent numpy implementation and asserts that the batches of tests/impulse_batches.py hold what they
are for).  Counts, records, momentum and idle counters must equal the oracle's byte for byte, and so must every byte behind a written prefix: a 0xA5
sentinel there stays the sentinel."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostimpulse_util as HI                # noqa: E402
import impulse_batches as B                  # noqa: E402
import query_util as Q                       # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu
_stopped = []          # why no further test of this module starts anything on the GPU


@pytest.fixture(autouse=True)
def _not_stopped():
    assert not _stopped, f"not started: {_stopped[0]}"


SENTINEL = 0xA5
SLACK = 2          # sentinel records kept behind every output's capacity
NH_ERR_INVALID = 1


@pytest.fixture(scope="module")
def w():
    """A context to call through; the sums and the generators read the body arrays they are given, not its world's."""
    world = E.World(S.pile(8, 0, seed=1), flags=Q.FUSED)
    yield world
    world.close()


def sentinel(n, dtype=E.IMPULSE_SUM):
    return np.frombuffer(bytes([SENTINEL]) * dtype.itemsize * n, dtype=dtype).copy()


def word(w, value):
    import torch
    return torch.tensor([value], dtype=torch.int64, device=w.dev).to(torch.int32)


def up(w, a):
    import torch
    return Q.upload(w, a) if len(a) else torch.zeros(64, dtype=torch.uint8, device=w.dev)


def body_data(tdev, count):
    """An nh_BodyData of transforms alone (what nh_impulse_sums and nh_blast_impulses read)."""
    return E.BodyData(tdev.data_ptr(), 0, 0, 0, count)


def dev_out(w, capacity):
    """An output list (count, sums, capacity): the count word and capacity + SLACK records of the sentinel; capacity None: count only."""
    import torch
    ct = torch.full((1,), -0x5A5A5A5B, dtype=torch.int32, device=w.dev)          # 0xA5A5A5A5
    if capacity is None:
        return ct, None, 0
    return ct, torch.full((capacity + SLACK, 32), SENTINEL, dtype=torch.uint8, device=w.dev), capacity


def read(out):
    ct, st, _ = out
    n = int(ct.cpu().numpy().view(np.uint32)[0])
    return n, (None if st is None else np.frombuffer(st.cpu().numpy().tobytes(), dtype=E.IMPULSE_SUM).copy())


def same(got, want, what):
    assert got[0] == want[0], f"{what}: count {got[0]}, the oracle's {want[0]}"
    if got[1] is not None:
        a, b = got[1].view(np.uint8).reshape(-1, 32), want[1].view(np.uint8).reshape(-1, 32)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {int((a != b).any(axis=1).sum())} of {len(a)} record slots differ"


def gpu_sums(w, bodies, ldev, n, capacity, count=None):
    out = dev_out(w, capacity)
    w.impulse_sums_records(ldev if n else None, count=None if count is None else word(w, count), capacity=n, out=out, bodies=bodies)
    return read(out)


def check_sums(w, t, lst, what, tdev=None):
    """Count only, then a list of exactly the count, against the oracle.  Returns the count."""
    tdev = up(w, t) if tdev is None else tdev
    bodies, ldev = body_data(tdev, len(t)), up(w, lst)
    total = HI.count_sums(t, lst)
    same(gpu_sums(w, bodies, ldev, len(lst), None), (total, None), f"{what}, count only")
    same(gpu_sums(w, bodies, ldev, len(lst), total), HI.sums(t, lst, capacity=total, out=sentinel(total + SLACK)), what)
    return total


# ---- nh_impulse_sums ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", B.SIZES)
def test_lists_of_every_size(w, n):
    """count == NULL: the capacity is the count.  70,001 records: more than one tile per block of the 512-block sort, a scan over several blocks."""
    for mode in B.MODES:
        t, lst = B.sized(n, mode)
        total = check_sums(w, t, lst, f"{mode} {n}")
        assert total == {"one_body": min(n, 1), "distinct": n}.get(mode, total)


def test_every_rule_and_every_key_width(w):
    import torch
    bodies = B.feature_bodies()
    lst = B.features(bodies)
    B.check_features(bodies, lst)
    check_sums(w, bodies["transforms"], lst, "features")
    cases = B.key_widths()
    B.check_key_widths(cases)
    for count, used, t, lst, passes in cases:
        tdev = torch.zeros((count, 32), dtype=torch.uint8, device=w.dev)          # (the unused bodies' transforms are zeros on both sides)
        tdev[torch.from_numpy(used.astype(np.int64)).to(w.dev)] = Q.upload(w, t).reshape(-1, 32)
        assert check_sums(w, B.dense(count, used, t), lst, f"{passes} key bytes", tdev=tdev) == len(used)
        del tdev


def test_capacity_one_short_exact_and_with_room_to_spare(w):
    for t, lst in ((B.feature_bodies()["transforms"], B.features()), B.sized(257, "mixed")):
        tdev = up(w, t)
        bodies, ldev, n = body_data(tdev, len(t)), up(w, lst), len(lst)
        total = HI.count_sums(t, lst)
        assert total > 1
        same(gpu_sums(w, bodies, ldev, n, None), (total, None), "count only")
        same(gpu_sums(w, bodies, ldev, n, total - 1), (total, sentinel(total - 1 + SLACK)), "one short: the count, and every record byte the sentinel")
        same(gpu_sums(w, bodies, ldev, n, total), HI.sums(t, lst, capacity=total, out=sentinel(total + SLACK)), "exact")
        same(gpu_sums(w, bodies, ldev, n, total + 7), HI.sums(t, lst, capacity=total + 7, out=sentinel(total + 7 + SLACK)), "room to spare")


def test_a_device_count_below_and_above_the_capacity(w):
    """The tail is NaNs on bodies that exist; the result is that of the truncated list.  A count above the capacity is clamped to it."""
    t, lst = B.sized(513, "mixed")
    tdev = up(w, t)
    bodies = body_data(tdev, len(t))
    for keep in (300, 1, 0):
        tail = lst.copy()
        tail["point"][keep:], tail["impulse"][keep:], tail["body"][keep:], tail["flags"][keep:] = np.nan, np.nan, 1, 0
        total = HI.count_sums(t, lst[:keep])
        want = HI.sums(t, lst[:keep], capacity=total, out=sentinel(total + SLACK))
        same(gpu_sums(w, bodies, up(w, tail), len(tail), total, count=keep), want, f"count {keep} of 513")
    total = HI.count_sums(t, lst)
    same(gpu_sums(w, bodies, up(w, lst), len(lst), total, count=100000), HI.sums(t, lst, capacity=total, out=sentinel(total + SLACK)), "count above the capacity")


# ---- nh_body_impulses ---------------------------------------------------------------------------------------------------------------------------
def crafted_world(bodies):
    """S.pile(8, 0, seed=1) with the poses, properties, momentum and idle counters of `bodies`; never stepped."""
    scene = dict(S.pile(8, 0, seed=1))
    assert len(scene["body_transforms"]) == B.FEATURE_BODIES
    scene.update(body_transforms=bodies["transforms"], body_properties=bodies["properties"], body_momentum=bodies["momentum"], idle_counters=bodies["idle"])
    return E.World(scene, flags=Q.FUSED)


@pytest.mark.parametrize("wake", [False, True])
def test_body_impulses_on_a_small_pile(wake):
    bodies = B.feature_bodies()
    lst = B.features(bodies)
    B.check_features(bodies, lst)
    wd = crafted_world(bodies)
    wd.body_impulses_records(up(wd, lst), capacity=len(lst), wake=wake)
    got = wd.get_bodies()
    m, idle = HI.apply(bodies, lst, wake=wake)
    assert got["momentum"].tobytes() == m.tobytes(), "momentum (unused0 / unused1 included) differs from the oracle's"
    assert got["idle"].tobytes() == idle.tobytes() and got["transforms"].tobytes() == bodies["transforms"].tobytes()
    assert m.tobytes() != bodies["momentum"].tobytes() and (idle.tobytes() != bodies["idle"].tobytes()) == wake
    for b in (0, 8):          # no valid record names them
        assert got["momentum"][b].tobytes() == bodies["momentum"][b].tobytes() and got["idle"][b] == bodies["idle"][b]
    # a device count: the first 4 records only; capacity 0: nothing at all
    before = wd.get_bodies()
    wd.body_impulses_records(up(wd, lst), count=word(wd, 4), capacity=len(lst), wake=wake)
    now = dict(bodies, momentum=before["momentum"], idle=before["idle"])
    m, idle = HI.apply(now, lst, count=4, wake=wake)
    got = wd.get_bodies()
    assert got["momentum"].tobytes() == m.tobytes() and got["idle"].tobytes() == idle.tobytes()
    wd.body_impulses_records(None, capacity=0, wake=wake)
    again = wd.get_bodies()
    assert again["momentum"].tobytes() == m.tobytes() and again["idle"].tobytes() == idle.tobytes()
    wd.close()


def test_the_convenience_call_builds_the_records_of_its_arguments():
    bodies = B.feature_bodies()
    rng = np.random.default_rng(3)
    body = np.array([3, 3, 1, 5, 3, 0, 9], dtype=np.uint32)          # (the last two: nobody's)
    impulse = rng.normal(size=(len(body), 3)).astype(np.float32)
    point = bodies["transforms"]["position"][np.minimum(body, 8)] + rng.normal(size=(len(body), 3)).astype(np.float32)
    for points, wake in ((point, True), (None, False)):
        wd = crafted_world(bodies)
        wd.body_impulses(body.astype(np.int64), impulse, points=points, wake=wake)
        got = wd.get_bodies()
        m, idle = HI.apply(bodies, HI.records(body, impulse, point=points), wake=wake)
        assert got["momentum"].tobytes() == m.tobytes() and got["idle"].tobytes() == idle.tobytes(), (points is None, wake)
        assert m.tobytes() != bodies["momentum"].tobytes()
        wd.close()


# ---- the generators -----------------------------------------------------------------------------------------------------------------------------
def test_blast_records_of_every_crafted_case(w):
    cases = B.blast_cases()
    B.check_blast_cases(cases)
    for name, (t, blasts, offsets, hits) in cases.items():
        tdev, n = up(w, t), len(blasts)
        for cap in (len(hits), max(len(hits) - 2, 0)):
            fill = sentinel(len(hits) + SLACK, E.BODY_IMPULSE)
            out = Q.upload(w, fill)
            odev, hdev, bdev = up(w, offsets), up(w, hits), up(w, blasts)
            lst = E.HitList(odev.data_ptr(), hdev.data_ptr(), cap, 0)
            rc = w.L.nh_blast_impulses(w.ctx, C.byref(body_data(tdev, len(t))), bdev.data_ptr(), n, C.byref(lst), out.data_ptr(), 0)
            assert rc == 0
            want = HI.blast(t, blasts, offsets, hits, capacity=cap, out=fill.copy())
            assert out.cpu().numpy().tobytes() == want.tobytes(), f"{name}, capacity {cap}"
            assert want[cap:].tobytes() == fill[cap:].tobytes()


def test_touch_records_of_the_crafted_case(w):
    case = B.touch_case()
    B.check_touch_case(case)
    pushes, k, counts, touches = case
    n = len(pushes)
    fill = sentinel(n * k + SLACK, E.BODY_IMPULSE)
    out = Q.upload(w, fill)
    w.touch_impulses_records(up(w, pushes), n, k, up(w, counts), up(w, touches), out=out)
    want = HI.touch(*case, out=fill.copy())
    assert out.cpu().numpy().tobytes() == want.tobytes()
    assert want[n * k:].tobytes() == fill[n * k:].tobytes() and (want["body"][:n * k] != HI.NO_BODY).sum() >= 5


def _tiles():
    return S.grid_tiles(1, side=12, seed=2)


def test_the_blast_chain_equals_the_host_chain_on_the_downloaded_lists():
    import torch
    scene = _tiles()
    wd = E.World(scene, flags=Q.FUSED)
    wd.step(60)
    wd.synchronize()
    wd.query_build()
    t = wd.get_bodies()["transforms"]
    mid = t["position"][1:].astype(np.float64).mean(axis=0)
    blasts = np.zeros(2, dtype=E.BLAST)
    blasts["centre"], blasts["radius"], blasts["strength"], blasts["falloff"] = [mid, mid + (4, 0, -3)], [5.0, 3.0], [6.0, 2.0], [1.0, 0.25]
    q = np.zeros(2, dtype=E.OVERLAP_QUERY)
    q["center"], q["shape"], q["rotation"], q["ignore_body"] = blasts["centre"], E.NH_SHAPE_SPHERE, (0, 0, 0, 1), Q.NONE
    q["size"][:, 0] = blasts["radius"]
    cap = wd.nbox + wd.nsph
    hits, per_body = (torch.full((2 * cap, 16), SENTINEL, dtype=torch.uint8, device=wd.dev) for _ in range(2))
    offsets, _ = wd.overlap_wide_records(Q.upload(wd, q), hits=hits, capacity=2 * cap)
    body_offsets, _ = wd.overlap_bodies_records(2, (offsets, hits, 2 * cap), hits=per_body, capacity=2 * cap)
    rec = wd.blast_impulses_records(Q.upload(wd, blasts), 2, (body_offsets, per_body, 2 * cap))
    out = dev_out(wd, wd.nb)
    wd.impulse_sums_records(rec, capacity=2 * cap, out=out)
    got = read(out)
    # the host chain on the downloaded lists
    off = body_offsets.cpu().numpy().view(np.uint32)
    h = np.frombuffer(per_body.cpu().numpy().tobytes(), dtype=E.OVERLAP_HIT)
    total = int(off[2])
    assert 0 < total <= 2 * cap
    want_rec = np.zeros(2 * cap, dtype=E.BODY_IMPULSE)
    want_rec["body"] = HI.NO_BODY
    HI.blast(t, blasts, off, h[:total], out=want_rec)
    assert rec.cpu().numpy().tobytes() == want_rec.tobytes(), "the blast records differ from the oracle's"
    same(got, HI.sums(t, want_rec, capacity=wd.nb, out=sentinel(wd.nb + SLACK)), "the sums of the blast")
    assert got[0] >= 1, "nobody was hit"
    # the one-call form gives the same records
    again = wd.blast(blasts["centre"], blasts["radius"], blasts["strength"], falloff=blasts["falloff"], wake=False)
    assert again.cpu().numpy().tobytes()[:32 * total] == want_rec[:total].tobytes()
    wd.close()


# ---- end to end against the existing path -------------------------------------------------------------------------------------------------------
def _same_bodies(worlds, what):
    ref = worlds[0].get_bodies()
    for k, wd in enumerate(worlds[1:], 1):
        got = wd.get_bodies()
        for key in ("transforms", "momentum", "idle"):
            assert got[key].tobytes() == ref[key].tobytes(), f"{what}: {key} of world {k} differ from world 0's"
    return ref


def _kick(scene, nb):
    """The kick's records: hops at the centre (leaning sideways: a body that lands where it stood would not show) and shoves at a corner, two records on
    some bodies, by each body's own mass."""
    pr = scene["body_properties"]
    hop, shove = np.arange(5, nb, 17), np.arange(11, nb, 23)
    body = np.concatenate([hop, shove, hop[:3]]).astype(np.uint32)
    dv = np.concatenate([np.tile([0.75, 4.0, 0.0], (len(hop), 1)), np.tile([1.5, 0.0, 0.5], (len(shove), 1)), np.tile([0.0, 0.5, 0.0], (3, 1))])
    return body, (dv / pr["mass_inverse"][body][:, None]).astype(np.float32), np.unique(body)


def test_a_kick_on_the_device_is_the_kick_through_the_momentum_array():
    """A: nh_body_impulses on the device.  B: the oracle's momentum through set_bodies, the existing path.  C: A's call in a world that never speculates.
    D: nobody kicked."""
    scene = _tiles()
    a, b, c, d = (E.World(scene, flags=Q.FUSED) for _ in range(4))
    c.set_option("no_still", 1)
    worlds = (a, b, c)
    landed = False
    for _ in range(40):          # (a world in free fall takes still steps too: wait for still steps of the LANDED world)
        before = a.counts()["still_steps"]
        for wd in worlds + (d,):
            wd.step(20)
        ca = a.counts()
        if ca["contacts"] >= a.nb - 1 and ca["still_steps"] > before:
            landed = True
            break
    assert landed and c.counts()["still_steps"] == 0
    a.step(3); b.step(3); c.step(3); d.step(3)          # (the step after counts() is a full one: be in the still regime again)
    c0 = a.counts()
    body, impulse, kicked = _kick(scene, a.nb)
    state = _same_bodies(worlds, "before the kick")
    at = state["transforms"]["position"][body] + np.float32([0.4, 0.4, 0.4])
    lst = HI.records(body, impulse, point=at)
    lst["flags"][:len(body) // 2] = E.NH_IMPULSE_AT_CENTRE
    m, idle = HI.apply(dict(state, properties=scene["body_properties"]), lst)
    assert idle.tobytes() == state["idle"].tobytes() and m.tobytes() != state["momentum"].tobytes()
    for wd in (a, c):
        wd.body_impulses_records(Q.upload(wd, lst), capacity=len(lst))
    b.set_bodies(momentum=m)
    _same_bodies(worlds, "right after the kick")
    done = 0
    for cp in (100, 250):
        for wd in worlds + (d,):
            wd.step(cp - done)
        done = cp
        _same_bodies(worlds, f"{cp} steps after the kick")
    c1 = a.counts()
    assert c1["still_replays"] > c0["still_replays"], (c0, c1)
    assert c1["error"] == 0 and b.counts()["error"] == 0 and c.counts()["still_steps"] == 0
    moved = np.abs(a.get_bodies()["transforms"]["position"][kicked].astype(np.float64) - d.get_bodies()["transforms"]["position"][kicked]).max(axis=1)
    assert (moved > 0.01).all(), f"kicked bodies that did not move: {kicked[moved <= 0.01]}"
    for wd in worlds + (d,):
        wd.close()


def test_a_kick_with_the_wake_flag_wakes_a_sleeping_tile():
    scene = _tiles()
    a, b, c, d = (E.World(scene, flags=Q.FUSED) for _ in range(4))
    c.set_option("no_still", 1)
    worlds = (a, b, c)
    for _ in range(8):
        for wd in worlds + (d,):
            wd.step(100)
        if a.counts()["active_bodies"] == 0:
            break
    for wd in worlds + (d,):
        wd.step(20)
    assert all(wd.counts()["active_bodies"] == 0 for wd in worlds + (d,)), "the tile was meant to be asleep"
    body, impulse, kicked = _kick(scene, a.nb)
    state = _same_bodies(worlds, "asleep")
    lst = HI.records(body, impulse, point=state["transforms"]["position"][body] + np.float32([0.4, 0.4, 0.4]))
    lst["flags"][:len(body) // 2] = E.NH_IMPULSE_AT_CENTRE
    m, idle = HI.apply(dict(state, properties=scene["body_properties"]), lst, wake=True)
    assert (idle[kicked] == 0).all() and (state["idle"][kicked] != 0).all()
    for wd in (a, c):
        wd.body_impulses_records(Q.upload(wd, lst), capacity=len(lst), wake=True)
    b.set_bodies(momentum=m, idle=idle)
    _same_bodies(worlds, "right after the kick")
    done = 0
    for cp in (1, 100, 250):
        for wd in worlds + (d,):
            wd.step(cp - done)          # (NH_ERR_STALE_HINT would raise here)
        done = cp
        _same_bodies(worlds, f"{cp} steps after the kick")
        counts = [wd.counts() for wd in worlds]
        assert all(cn["error"] == 0 for cn in counts), counts
        if cp == 1:
            assert all(cn["active_bodies"] > 0 for cn in counts) and d.counts()["active_bodies"] == 0, "the active count rises from 0"
    moved = np.abs(a.get_bodies()["transforms"]["position"][kicked].astype(np.float64) - d.get_bodies()["transforms"]["position"][kicked]).max(axis=1)
    assert (moved > 0.01).all(), f"kicked bodies that did not move: {kicked[moved <= 0.01]}"
    for wd in worlds + (d,):
        wd.close()


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_return_before_any_launch():
    import torch
    bodies = B.feature_bodies()
    lst = B.features(bodies)
    wd = crafted_world(bodies)
    L, ctx, ref = wd.L, wd.ctx, C.byref
    ldev = up(wd, lst)
    outs = []

    def ilist(**kw):
        f = dict(records=ldev.data_ptr(), count=0, capacity=len(lst))
        f.update(kw)
        return E.ImpulseList(f["records"], f["count"], f["capacity"], 0)

    def slist(**kw):
        o = dev_out(wd, 8)          # (eight records, whatever capacity the struct then claims: nothing may be written)
        outs.append(o)
        f = dict(count=o[0].data_ptr(), sums=o[1].data_ptr(), capacity=8)
        f.update(kw)
        return E.ImpulseSumList(f["count"], f["sums"], f["capacity"], 0)

    def bdata(**kw):
        f = dict(transforms=wd.bodies.transforms, properties=wd.bodies.properties, momentum=wd.bodies.momentum, idle_counters=wd.bodies.idle_counters, count=wd.nb)
        f.update(kw)
        return E.BodyData(f["transforms"], f["properties"], f["momentum"], f["idle_counters"], f["count"])

    ok_b, ok_in = ref(wd.bodies), ref(ilist())
    bad_lists = [dict(records=0), dict(records=ldev.data_ptr() + 8), dict(count=ldev.data_ptr() + 2), dict(capacity=1 << 31), dict(capacity=0xFFFFFFFF)]
    bad_sums = [dict(sums=0), dict(count=0), dict(capacity=1 << 31), dict(capacity=0xFFFFFFFF)]
    calls = [
        lambda: L.nh_impulse_sums(None, ok_b, ok_in, ref(slist()), 0),
        lambda: L.nh_impulse_sums(ctx, None, ok_in, ref(slist()), 0),
        lambda: L.nh_impulse_sums(ctx, ok_b, None, ref(slist()), 0),
        lambda: L.nh_impulse_sums(ctx, ok_b, ok_in, None, 0),
        lambda: L.nh_impulse_sums(ctx, ok_b, ok_in, ref(slist()), 1),
        lambda: L.nh_impulse_sums(ctx, ref(bdata(transforms=0)), ok_in, ref(slist()), 0),
        lambda: L.nh_body_impulses(None, ok_b, ok_in, 0),
        lambda: L.nh_body_impulses(ctx, None, ok_in, 0),
        lambda: L.nh_body_impulses(ctx, ok_b, None, 0),
        lambda: L.nh_body_impulses(ctx, ok_b, ok_in, 2),
        lambda: L.nh_body_impulses(ctx, ok_b, ok_in, 0x80000001),
    ]
    calls += [lambda k=k: L.nh_body_impulses(ctx, ref(bdata(**{k: 0})), ok_in, 0) for k in ("transforms", "properties", "momentum", "idle_counters")]
    for bad in bad_lists:
        calls += [lambda bad=bad: L.nh_impulse_sums(ctx, ok_b, ref(ilist(**bad)), ref(slist()), 0),
                  lambda bad=bad: L.nh_body_impulses(ctx, ok_b, ref(ilist(**bad)), E.NH_IMPULSE_WAKE)]
    calls += [lambda bad=bad: L.nh_impulse_sums(ctx, ok_b, ok_in, ref(slist(**bad)), 0) for bad in bad_sums]
    calls += [lambda: L.nh_impulse_sums(ctx, ok_b, ok_in, ref(slist(sums=outs[0][1].data_ptr() + 8)), 0),
              lambda: L.nh_impulse_sums(ctx, ok_b, ok_in, ref(slist(count=outs[0][1].data_ptr() + 2)), 0)]
    # the generators: flags, NULL arrays with something to do, misaligned outputs
    gen = torch.full((64, 32), SENTINEL, dtype=torch.uint8, device=wd.dev)
    t, blasts, offsets, hits = B.blast_cases()["one record"]
    bl, of, hi = up(wd, blasts), up(wd, offsets), up(wd, hits)
    hl = lambda **kw: ref(E.HitList(kw.get("offsets", of.data_ptr()), kw.get("hits", hi.data_ptr()), kw.get("capacity", len(hits)), 0))
    pushes, k, counts, touches = B.touch_case()
    pu, cn, to = up(wd, pushes), up(wd, counts), up(wd, touches)
    calls += [
        lambda: L.nh_blast_impulses(ctx, ok_b, bl.data_ptr(), 1, hl(), gen.data_ptr(), 1),
        lambda: L.nh_blast_impulses(None, ok_b, bl.data_ptr(), 1, hl(), gen.data_ptr(), 0),
        lambda: L.nh_blast_impulses(ctx, None, bl.data_ptr(), 1, hl(), gen.data_ptr(), 0),
        lambda: L.nh_blast_impulses(ctx, ok_b, None, 1, hl(), gen.data_ptr(), 0),
        lambda: L.nh_blast_impulses(ctx, ok_b, bl.data_ptr(), 1, None, gen.data_ptr(), 0),
        lambda: L.nh_blast_impulses(ctx, ok_b, bl.data_ptr(), 1, hl(), None, 0),
        lambda: L.nh_blast_impulses(ctx, ok_b, bl.data_ptr(), 1, hl(offsets=0), gen.data_ptr(), 0),
        lambda: L.nh_blast_impulses(ctx, ok_b, bl.data_ptr(), 1, hl(hits=0), gen.data_ptr(), 0),
        lambda: L.nh_blast_impulses(ctx, ok_b, bl.data_ptr(), 1, hl(capacity=1 << 31), gen.data_ptr(), 0),
        lambda: L.nh_blast_impulses(ctx, ok_b, bl.data_ptr(), 1, hl(), gen.data_ptr() + 8, 0),
        lambda: L.nh_blast_impulses(ctx, ref(bdata(transforms=0)), bl.data_ptr(), 1, hl(), gen.data_ptr(), 0),
        lambda: L.nh_touch_impulses(ctx, pu.data_ptr(), len(pushes), k, cn.data_ptr(), to.data_ptr(), gen.data_ptr(), 1),
        lambda: L.nh_touch_impulses(None, pu.data_ptr(), len(pushes), k, cn.data_ptr(), to.data_ptr(), gen.data_ptr(), 0),
        lambda: L.nh_touch_impulses(ctx, None, len(pushes), k, cn.data_ptr(), to.data_ptr(), gen.data_ptr(), 0),
        lambda: L.nh_touch_impulses(ctx, pu.data_ptr(), len(pushes), k, None, to.data_ptr(), gen.data_ptr(), 0),
        lambda: L.nh_touch_impulses(ctx, pu.data_ptr(), len(pushes), k, cn.data_ptr(), None, gen.data_ptr(), 0),
        lambda: L.nh_touch_impulses(ctx, pu.data_ptr(), len(pushes), k, cn.data_ptr(), to.data_ptr(), None, 0),
        lambda: L.nh_touch_impulses(ctx, pu.data_ptr(), len(pushes), k, cn.data_ptr(), to.data_ptr(), gen.data_ptr() + 8, 0),
        lambda: L.nh_touch_impulses(ctx, pu.data_ptr(), 1 << 30, 2, cn.data_ptr(), to.data_ptr(), gen.data_ptr(), 0),
    ]
    for k_, call in enumerate(calls):
        assert call() == NH_ERR_INVALID, f"call {k_} did not return NH_ERR_INVALID"
    torch.cuda.synchronize()
    for o in outs:
        n, rec = read(o)
        assert n == 0xA5A5A5A5 and rec.tobytes() == sentinel(len(rec)).tobytes(), "an output was written by a call that returned NH_ERR_INVALID"
    assert gen.cpu().numpy().tobytes() == bytes([SENTINEL]) * 64 * 32
    got = wd.get_bodies()
    assert got["momentum"].tobytes() == bodies["momentum"].tobytes() and got["idle"].tobytes() == bodies["idle"].tobytes()
    # capacity 0 with NULL records: the empty list -- *count = 0 and nothing else
    out = dev_out(wd, 4)
    wd.impulse_sums_records(None, capacity=0, out=out)
    same(read(out), (0, sentinel(4 + SLACK)), "capacity 0, records NULL")
    wd.close()


# ---- the measurement program ----------------------------------------------------------------------------------------------------------------------
LIMIT = 60          # seconds for the child: a few seconds on an MI355X, most of it start-up; the rest is for a cold file cache
FATAL = (124, 134, 137, 139)


def _profiles():
    d = os.path.join(ROOT, "profiles")
    return {f: (os.stat(os.path.join(d, f)).st_mtime_ns, os.stat(os.path.join(d, f)).st_size) for f in sorted(os.listdir(d))}


def test_the_measurement_program_rehearsal(tmp_path):
    """tools/body_impulses.py on 2 tiles of side 12 in a fresh child process.  A child that ends by a signal or at its limit stops the module."""
    out = tmp_path / "body_impulses.log"
    env = {k: v for k, v in os.environ.items() if k != "NUDGE_HIP_LIBRARY"}
    before = _profiles()
    cmd = [sys.executable, os.path.join(ROOT, "tools", "body_impulses.py"), "--tiles", "2", "--side", "12", "--reps", "2", "--inner", "2", "--out", str(out)]
    try:
        child = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=LIMIT, cwd=str(tmp_path))
    except subprocess.TimeoutExpired:
        _stopped.append(f"tools/body_impulses.py was still running after {LIMIT} s")
        raise
    if child.returncode < 0 or child.returncode in FATAL:
        _stopped.append(f"tools/body_impulses.py ended with status {child.returncode}")
    assert child.returncode == 0, f"status {child.returncode}\n{child.stdout[-2000:]}\n{child.stderr[-4000:]}"
    assert out.read_text() == child.stdout
    last = json.loads(child.stdout.rstrip("\n").split("\n")[-1])
    assert isinstance(last, dict) and last and last["blast_bodies_pushed"] > 0 and all(v > 0 for k, v in last.items() if k.startswith("checked"))
    assert _profiles() == before
