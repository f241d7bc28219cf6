"""Sensors on the GPU (pytest -m gpu): nh_sense and nh_sense_rays (include/nudge_hip.h, "sensors").

The oracle is tests/hostoracle/hostsense.cpp through tests/hostsense_util.py: the ray of every (sensor, beam) by nudge_amd/csrc/nh_query.h's own
arithmetic, and a brute force over every collider on each such ray.  The answer is defined without the tree, so every channel must equal the oracle
byte for byte; and nh_sense's records must equal what the GPU's own nh_raycast writes for the GPU's own nh_sense_rays records, an identity that needs
no host.  Every output buffer is pre-filled with a sentinel and carries 64 guard records behind it that must come back untouched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cast_util as CU                       # noqa: E402
import filter_util as F                      # noqa: E402
import hostcast_util as HC                   # noqa: E402
import hostsense_util as HS                  # noqa: E402
import list_util as LU                       # noqa: E402
import query_util as Q                       # noqa: E402
from list_util import SENTINEL               # noqa: E402
from query_util import FUSED, NONE, OBSERVED, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
GRID_WAVES = 65536 * 4                       # NH_Q_SENSE_GRID workgroups of four waves: the wave items of one pass
DTYPES = dict(t=np.dtype("<f4"), body=np.dtype("<u4"), tag=np.dtype("<u4"), hits=E.RAY_HIT, rays=E.RAY)
BEAMS, COUNTS = (1, 63, 64, 65, 200), (1, 5, 300)


# ---- the calls --------------------------------------------------------------------------------------------------------------------------------
def _buffer(w, n, name):
    import torch
    return torch.full(((n + GUARD) * DTYPES[name].itemsize,), SENTINEL, dtype=torch.uint8, device=w.dev)


def _back(buf, n, name, what):
    a = np.frombuffer(buf.cpu().numpy().tobytes(), dtype=DTYPES[name]).copy()
    assert set(a[n:].tobytes()) == {SENTINEL}, f"{what}: bytes behind the {n} records of `{name}` were written"
    return a[:n]


def _sense(w, sensors, beams, channels=E.SENSE_CHANNELS, any_hit=False, mounted=True, what=""):
    """dict(channel: numpy records) of one nh_sense call into sentinel-filled buffers; the guards behind each must come back untouched."""
    n = len(sensors) * len(beams)
    bufs = {c: _buffer(w, n, c) for c in channels}
    w.sense_records(_upload(w, sensors), _upload(w, beams), any_hit=any_hit, mounted=mounted, **bufs)
    return {c: _back(bufs[c], n, c, what) for c in channels}


def _rays(w, sensors, beams, mounted=True, what=""):
    n = len(sensors) * len(beams)
    buf = _buffer(w, n, "rays")
    w.sense_rays_records(_upload(w, sensors), _upload(w, beams), rays=buf, mounted=mounted)
    return _back(buf, n, "rays", what)


def _same(got, ref, what):
    for c in got:
        size = DTYPES[c].itemsize
        bad = (got[c].view(np.uint8).reshape(-1, size) != np.ascontiguousarray(ref[c]).view(np.uint8).reshape(-1, size)).any(axis=1)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {len(bad)} records of `{c}` differ, first at {int(np.argmax(bad))}"


def _world(name, steps=30):
    """(world, scene, records, body transforms, dynamic bodies) of HOST_WORLDS[name] after `steps` steps and a build."""
    scene = CU.HOST_WORLDS[name]()
    w = E.World(scene, flags=FUSED)
    if steps:
        w.step(steps)
    w.query_build()
    return (w, scene) + _state(w, scene)


def _state(w, scene):
    bt = w.get_bodies()["transforms"]
    rec = Q.records(w, scene)
    return rec, bt, np.unique(rec["body"][rec["body"] != 0])


def _batches(rng, rec, bt, dynamic, spoil=False):
    """(sensors, beams) for every beam count of BEAMS -- the tail lanes, one and several waves a sensor -- times every count of COUNTS -- one and
    several workgroups: world-frame and mounted sensors mixed, mounts on body 0, on dynamic bodies and out of range."""
    for m in BEAMS:
        for count in COUNTS:
            yield HS.sensors(rng, count, rec, nbodies=len(bt), dynamic=dynamic, spoil=spoil), HS.pattern(rng, m)


# ---- rays and answers against the host ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CU.HOST_WORLDS))
def test_the_rays_equal_the_oracle(name):
    w, scene, rec, bt, dynamic = _world(name)
    rng = np.random.default_rng(800 + sorted(CU.HOST_WORLDS).index(name))
    for sensors, beams in _batches(rng, rec, bt, dynamic):
        what = f"{name} / {len(sensors)} x {len(beams)}"
        _same(dict(rays=_rays(w, sensors, beams, what=what)), dict(rays=HS.sense_rays(sensors, beams, bt)), what)
        _same(dict(rays=_rays(w, sensors, beams, mounted=False, what=what)), dict(rays=HS.sense_rays(sensors, beams, None)), what + " / no bodies")
    w.close()


@pytest.mark.parametrize("name", sorted(CU.HOST_WORLDS))
def test_all_four_channels_equal_the_oracle_and_the_gpus_own_raycast(name):
    w, scene, rec, bt, dynamic = _world(name)
    rng = np.random.default_rng(810 + sorted(CU.HOST_WORLDS).index(name))
    hit = []
    for sensors, beams in _batches(rng, rec, bt, dynamic, spoil=True):
        what = f"{name} / {len(sensors)} x {len(beams)}"
        got = _sense(w, sensors, beams, what=what)
        _same(got, HS.sense(rec, w.nbox, sensors, beams, bt), what)
        # without the host: nh_raycast on the rays nh_sense_rays wrote
        cast = CU.closest(w, _rays(w, sensors, beams, what=what))
        CU.same_hits(got["hits"], cast, what + " / nh_raycast on nh_sense_rays")
        assert got["t"].tobytes() == cast["t"].tobytes() and got["body"].tobytes() == cast["body"].tobytes() and got["tag"].tobytes() == cast["tag"].tobytes()
        hit.append(float((cast["shape"] != NONE).mean()))
    _same(_sense(w, sensors, beams, mounted=False), HS.sense(rec, w.nbox, sensors, beams, None), f"{name} / no bodies")
    assert max(hit) > 0.2 and min(hit) < 1.0, hit
    w.close()


def test_each_single_channel_call_writes_that_channels_bytes():
    w, scene, rec, bt, dynamic = _world("pile")
    rng = np.random.default_rng(820)
    sensors, beams = HS.sensors(rng, 37, rec, nbodies=len(bt), dynamic=dynamic, spoil=True), HS.pattern(rng, 65)
    full = _sense(w, sensors, beams)
    for c in E.SENSE_CHANNELS:
        _same(_sense(w, sensors, beams, channels=(c,), what=c), {c: full[c]}, f"{c} alone")
    _same(_sense(w, sensors, beams, channels=("t", "body")), dict(t=full["t"], body=full["body"]), "t and body")
    w.close()


def test_a_batch_whose_wave_items_stride_the_grid():
    w, scene, rec, bt, dynamic = _world("pile", steps=0)
    rng = np.random.default_rng(830)
    count = GRID_WAVES // 2 + 150                                         # 65 beams are two wave items a sensor: more items than one pass of the grid
    sensors, beams = HS.sensors(rng, count, rec, nbodies=len(bt), dynamic=dynamic), HS.pattern(rng, 65)
    assert count * 2 > GRID_WAVES
    got = _sense(w, sensors, beams, channels=("t", "body"))
    _same(got, HS.sense(rec, w.nbox, sensors, beams, bt, channels=("t", "body")), f"{count} x 65")
    # the rays of the last sensors, which the waves' second pass writes
    tail = _rays(w, sensors, beams)[-300 * 65:]
    _same(dict(rays=tail), dict(rays=HS.sense_rays(sensors[-300:], beams, bt)), f"{count} x 65 rays")
    w.close()


def _check_world(w, scene, rng, n, what):
    w.query_build()
    rec, bt, dynamic = _state(w, scene)
    sensors, beams = HS.sensors(rng, n, rec, nbodies=len(bt), dynamic=dynamic), HS.pattern(rng, 65)
    _same(_sense(w, sensors, beams, what=what), HS.sense(rec, w.nbox, sensors, beams, bt), what)


def test_degenerate_worlds():
    CU.degenerate_worlds(_check_world, np.random.default_rng(840), 64, 64, 16)


# ---- flags, filter, refit ---------------------------------------------------------------------------------------------------------------------
def test_any_hit_reports_real_hits_and_the_same_hit_or_miss():
    w, scene, rec, bt, dynamic = _world("compound")
    rng = np.random.default_rng(850)
    sensors, beams = HS.sensors(rng, 40, rec, nbodies=len(bt), dynamic=dynamic, spoil=True), HS.pattern(rng, 65)
    best = _sense(w, sensors, beams)
    got = _sense(w, sensors, beams, any_hit=True)
    hit = got["hits"]["shape"] != NONE
    assert np.array_equal(hit, best["hits"]["shape"] != NONE) and 0.05 < hit.mean() < 1.0
    assert got["hits"][~hit].tobytes() == best["hits"][~hit].tobytes()
    assert np.array_equal(got["t"].view(np.uint32), got["hits"]["t"].view(np.uint32)) and np.array_equal(got["body"], got["hits"]["body"]) and np.array_equal(got["tag"], got["hits"]["tag"])
    rays = HS.sense_rays(sensors, beams, bt)
    assert (got["t"][hit] <= rays["max_t"][hit]).all() and (got["t"][hit] >= 0).all()
    # each reported record is the single-collider oracle's for that ray and that collider
    comb = got["hits"]["collider"].astype(np.int64) + np.where(got["hits"]["shape"] == E.NH_SHAPE_BOX, 0, w.nbox)
    for c in np.unique(comb[hit]):
        sel = hit & (comb == c)
        assert got["hits"][sel].tobytes() == HC.cast(HC.RAY, rec, w.nbox, rays[sel], only=int(c)).tobytes(), int(c)
    w.close()


def test_the_filter_off_uniform_and_per_sensor_equals_the_oracle_over_the_masked_world():
    w, scene, rec, bt, dynamic = _world("pile")
    rng = np.random.default_rng(860)
    sensors, beams = HS.sensors(rng, 60, rec, nbodies=len(bt), dynamic=dynamic), HS.pattern(rng, 65)
    words = F.layers(len(rec), 861)
    whole = _sense(w, sensors, beams)
    w.query_set_layers(words[:w.nbox], words[w.nbox:])
    _same(_sense(w, sensors, beams), whole, "layers set, filter off")
    for mask in F.MASKS:
        w.query_filter(mask)
        got = _sense(w, sensors, beams)
        _same(got, HS.sense(rec, w.nbox, sensors, beams, bt, words=words, masks=mask), f"uniform mask {mask:#x}")
        if mask == 0:
            assert (got["hits"]["shape"] == NONE).all() and (got["body"] == NONE).all()           # mask 0 gives all misses
            rays = HS.sense_rays(sensors, beams, bt)
            valid = np.isfinite(rays["origin"]).all(axis=1)                                      # (a mount that does not exist: t = NaN)
            assert got["t"][valid].tobytes() == rays["max_t"][valid].tobytes() and np.isnan(got["t"][~valid]).all() and (~valid).any()
        elif mask == 1:
            assert got["hits"].tobytes() != whole["hits"].tobytes() and (got["hits"]["shape"] != NONE).any()
    masks = rng.choice(np.uint32([0, 1, 6, 0xFFFFFFFF]), size=len(sensors))                        # one mask per SENSOR
    w.query_filter(_upload(w, masks).view(w.torch.int32))
    got = _sense(w, sensors, beams)
    _same(got, HS.sense(rec, w.nbox, sensors, beams, bt, words=words, masks=masks), "per-sensor masks")
    assert (got["hits"].reshape(len(sensors), -1)[masks == 0]["shape"] == NONE).all()
    w.query_filter(None)
    _same(_sense(w, sensors, beams), whole, "filter off again")
    w.close()


def test_a_refit_gives_the_builds_bytes_on_the_new_transforms():
    w, scene, rec, bt, dynamic = _world("compound")
    rng = np.random.default_rng(870)
    sensors, beams = HS.sensors(rng, 50, rec, nbodies=len(bt), dynamic=dynamic), HS.pattern(rng, 65)
    before = _sense(w, sensors, beams)
    w.step(40)
    w.query_refit()
    rec2, bt2, _ = _state(w, scene)
    refit, refit_rays = _sense(w, sensors, beams), _rays(w, sensors, beams)
    _same(refit, HS.sense(rec2, w.nbox, sensors, beams, bt2), "refitted after 40 steps")
    _same(dict(rays=refit_rays), dict(rays=HS.sense_rays(sensors, beams, bt2)), "rays after 40 steps")
    w.query_build()
    _same(_sense(w, sensors, beams), refit, "build against refit")
    assert refit["hits"].tobytes() != before["hits"].tobytes()                                    # (the world did move)
    w.close()


def test_two_identical_calls_give_identical_bytes():
    w, scene, rec, bt, dynamic = _world("pile")
    rng = np.random.default_rng(880)
    sensors, beams = HS.sensors(rng, 300, rec, nbodies=len(bt), dynamic=dynamic, spoil=True), HS.pattern(rng, 200)
    _same(_sense(w, sensors, beams), _sense(w, sensors, beams), "twice")
    assert _rays(w, sensors, beams).tobytes() == _rays(w, sensors, beams).tobytes()
    w.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_abi_edge_cases():
    import torch
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    L = w.L
    rec, bt, dynamic = _state(w, scene)
    rng = np.random.default_rng(890)
    sensors, beams = HS.sensors(rng, 8, rec, nbodies=len(bt), dynamic=dynamic), HS.pattern(rng, 20)
    ns, nb, n = len(sensors), len(beams), len(sensors) * len(beams)
    st, bm = _upload(w, sensors), _upload(w, beams)
    words = torch.zeros(3 * (n + 8), dtype=torch.int32, device=w.dev)
    hits = torch.zeros((n + 8, 32), dtype=torch.uint8, device=w.dev)
    rays = torch.zeros((n + 8, 32), dtype=torch.uint8, device=w.dev)
    sp, bp, rp = C.c_void_p(st.data_ptr()), C.c_void_p(bm.data_ptr()), C.c_void_p(rays.data_ptr())
    tp, yp, gp, hp = words.data_ptr(), words.data_ptr() + 4 * (n + 8), words.data_ptr() + 8 * (n + 8), hits.data_ptr()
    bodies = C.byref(w.bodies)

    def out(t=tp, body=yp, tag=gp, hits=hp):
        return C.byref(E.SenseOut(t, body, tag, hits))

    assert L.nh_sense(w.ctx, bodies, sp, ns, bp, nb, out(), 0) == 1                # before any build: NH_ERR_INVALID
    assert L.nh_sense_rays(w.ctx, bodies, sp, ns, bp, nb, rp, 0) == 1
    assert L.nh_sense(None, bodies, sp, ns, bp, nb, out(), 0) == 1
    assert L.nh_sense_rays(None, bodies, sp, ns, bp, nb, rp, 0) == 1
    w.query_build()
    assert L.nh_sense(w.ctx, bodies, sp, ns, bp, nb, out(), 2) == 1                # flags
    assert L.nh_sense(w.ctx, bodies, sp, ns, bp, nb, out(), 3) == 1
    assert L.nh_sense_rays(w.ctx, bodies, sp, ns, bp, nb, rp, 1) == 1              # (NH_RAY_ANY_HIT has no meaning there)
    for call, last in ((L.nh_sense, out()), (L.nh_sense_rays, rp)):
        assert call(w.ctx, bodies, None, ns, bp, nb, last, 0) == 1                 # null / unaligned sensors and beams
        assert call(w.ctx, bodies, sp, ns, None, nb, last, 0) == 1
        assert call(w.ctx, bodies, C.c_void_p(st.data_ptr() + 4), ns - 1, bp, nb, last, 0) == 1
        assert call(w.ctx, bodies, sp, ns, C.c_void_p(bm.data_ptr() + 8), nb - 1, last, 0) == 1
        assert call(w.ctx, C.byref(E.BodyData(None, None, None, None, w.nb)), sp, ns, bp, nb, last, 0) == 1      # bodies without transforms
        assert call(w.ctx, bodies, sp, 1 << 16, bp, 1 << 15, last, 0) == 1         # count * beam_count >= 2^31: refused on the host
        assert call(w.ctx, bodies, sp, 0xFFFFFFFF, bp, 0xFFFFFFFF, last, 0) == 1
        assert call(w.ctx, bodies, sp, 0, bp, nb, last, 0) == 0                    # count 0, beam_count 0: no-ops, nothing read
        assert call(w.ctx, bodies, sp, ns, bp, 0, last, 0) == 0
        assert call(w.ctx, None, None, 0, None, 0, None, 0) == 0
        assert call(w.ctx, bodies, None, ns, None, 0, None, 0) == 0
    assert L.nh_sense_rays(w.ctx, bodies, sp, ns, bp, nb, None, 0) == 1            # null / unaligned rays
    assert L.nh_sense_rays(w.ctx, bodies, sp, ns, bp, nb, C.c_void_p(rays.data_ptr() + 8), 0) == 1
    assert L.nh_sense(w.ctx, bodies, sp, ns, bp, nb, None, 0) == 1                 # no out, no channel
    assert L.nh_sense(w.ctx, bodies, sp, ns, bp, nb, out(None, None, None, None), 0) == 1
    assert L.nh_sense(w.ctx, bodies, sp, ns, bp, nb, out(hits=hp + 8), 0) == 1     # unaligned hits; t, body, tag off a word boundary
    assert L.nh_sense(w.ctx, bodies, sp, ns, bp, nb, out(t=tp + 2), 0) == 1
    assert L.nh_sense(w.ctx, bodies, sp, ns, bp, nb, out(body=yp + 1), 0) == 1
    assert L.nh_sense(w.ctx, bodies, sp, ns, bp, nb, out(tag=gp + 3), 0) == 1
    assert L.nh_sense(w.ctx, bodies, sp, ns, bp, nb, out(None, None, gp + 2, None), 0) == 1
    torch.cuda.synchronize()
    assert int(words.abs().sum()) == 0 and int(hits.sum()) == 0 and int(rays.sum()) == 0         # nothing was written
    # t, body and tag need 4-byte alignment only: each at an odd word offset
    assert L.nh_sense(w.ctx, bodies, sp, ns, bp, nb, out(tp + 4, yp + 12, gp + 20, hp), 0) == 0
    assert L.nh_sense_rays(w.ctx, bodies, sp, ns, bp, nb, rp, 0) == 0
    ref = HS.sense(rec, w.nbox, sensors, beams, bt)
    assert 0 < (ref["hits"]["shape"] != NONE).sum() < n
    wd = words.cpu().numpy().view(np.uint32).reshape(3, n + 8)
    for k, (c, off) in enumerate((("t", 1), ("body", 3), ("tag", 5))):
        assert wd[k, off:off + n].tobytes() == ref[c].tobytes(), c
        assert not wd[k, :off].any() and not wd[k, off + n:].any(), c              # and no word beside them
    got = np.frombuffer(hits.cpu().numpy().tobytes(), dtype=E.RAY_HIT)
    assert got[:n].tobytes() == ref["hits"].tobytes() and not got[n:].view(np.uint8).any()
    gr = np.frombuffer(rays.cpu().numpy().tobytes(), dtype=E.RAY)
    assert gr[:n].tobytes() == HS.sense_rays(sensors, beams, bt).tobytes() and not gr[n:].view(np.uint8).any()
    w.close()


# ---- observers -----------------------------------------------------------------------------------------------------------------------------
def _observer_batch(a, scene):
    import torch
    a.query_build()
    rec, bt, dynamic = _state(a, scene)
    sensors = HS.sensors(np.random.default_rng(900), 64, rec, nbodies=len(bt), dynamic=dynamic)
    n = 64 * 65
    return (_upload(a, sensors), _upload(a, HS.pattern(np.random.default_rng(901), 65)), torch.empty(n, dtype=torch.float32, device=a.dev),
            torch.empty(n, dtype=torch.int32, device=a.dev), torch.empty((n, 32), dtype=torch.uint8, device=a.dev))


def _query(w, st, bm, t, body, rays):
    w.query_refit()
    w.sense_records(st, bm, t=t, body=body)
    w.sense_rays_records(st, bm, rays=rays)


def test_sensors_between_nh_step_calls_change_nothing():
    LU.queries_between_nh_step_calls_change_nothing(OBSERVED["grid_tiles"], _observer_batch, _query, "grid_tiles", still=True)


def test_sensors_between_every_call_of_the_fused_step_change_nothing():
    LU.queries_between_every_call_of_the_fused_step_change_nothing(OBSERVED["pile"], _observer_batch, _query, "pile", steps=120)


# ---- Python -----------------------------------------------------------------------------------------------------------------------------------
def test_the_python_wrapper():
    import torch
    w, scene, rec, bt, dynamic = _world("pile")
    rng = np.random.default_rng(910)
    tiled, back = E.pinhole_beams(24, 16, np.radians(70.0), 60.0)
    row, _ = E.pinhole_beams(24, 16, np.radians(70.0), 60.0, tile=1)
    s = HS.sensors(rng, 6, rec)
    s["position"][:, 1] = np.abs(s["position"][:, 1]) + 2.0
    a = w.sense(s["position"], s["rotation"], tiled, channels=("t", "body", "tag", "hits"), synchronize=True)
    b = w.sense(s["position"], s["rotation"], row, synchronize=True)
    assert a["t"].shape == (6, 384) and a["t"].dtype == torch.float32 and a["body"].dtype == torch.int64 and a["raw"].shape == (6, 384, 32)
    assert a["normal"].shape == (6, 384, 3) and set(b) == {"t", "body"}
    # the tiled pattern's image, un-permuted to row-major, is the row-major pattern's image
    t_img = a["t"].cpu().numpy()[:, back]
    assert t_img.tobytes() == b["t"].cpu().numpy().tobytes() and np.array_equal(a["body"].cpu().numpy()[:, back], b["body"].cpu().numpy())
    assert 0 < int((b["body"] != NONE).sum()) < 6 * 384
    ref = HS.sense(rec, w.nbox, s, row)
    assert b["t"].cpu().numpy().tobytes() == ref["t"].tobytes() and np.array_equal(b["body"].cpu().numpy().reshape(-1), ref["body"])
    # mounted, ignoring the carrier, a lidar pattern
    lid = E.lidar_beams(np.linspace(0.0, 2 * np.pi, 70, endpoint=False), np.radians([-10.0, 0.0]), 40.0)
    carrier = dynamic[:5].astype(np.int64)
    m = w.sense(np.zeros((5, 3)), np.tile(np.float32([0, 0, 0, 1]), (5, 1)), lid, bodies=carrier, ignore_body=carrier, channels=("t", "body"), synchronize=True)
    sm = np.zeros(5, dtype=E.SENSOR)
    sm["rotation"], sm["body"], sm["ignore_body"] = (0, 0, 0, 1), carrier, carrier
    ref = HS.sense(rec, w.nbox, sm, lid, bt)
    assert m["t"].cpu().numpy().tobytes() == ref["t"].tobytes() and np.array_equal(m["body"].cpu().numpy().reshape(-1), ref["body"])
    assert not (m["body"].cpu().numpy() == carrier[:, None]).any()
    with pytest.raises(ValueError):
        w.sense(s["position"], s["rotation"], row, channels=("depth",))
    w.close()
