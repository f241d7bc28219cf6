"""Sensors on the host (no GPU): the rays of nh_sense_rays and the answers of nh_sense (include/nudge_hip.h, "sensors") through the oracle of
tests/hostoracle/hostsense.cpp, which runs nudge_amd/csrc/nh_query.h's own arithmetic -- the bits the device computes.

The ray of (sensor, beam) is checked against a float64 restatement that shares no code with it, the answers against the ray oracle the cast tests use
(tests/hostcast_util.py) on those very rays: nh_sense is nh_raycast on the rays nh_sense_rays would write, channel by channel."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cast_util as CU                       # noqa: E402
import hostcast_util as HC                   # noqa: E402
import hostsense_util as HS                  # noqa: E402
from hostsense_util import NONE, QNAN        # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


def test_the_library_exports_the_sensor_calls():
    so = os.path.join(ROOT, "nudge_amd", "libnudge_hip.so")
    if not os.path.exists(so):
        E.build()
    lib = ctypes.CDLL(so)
    assert hasattr(lib, "nh_sense") and hasattr(lib, "nh_sense_rays")
    assert {"nh_sense", "nh_sense_rays"} <= set(E.EXPORTS)
    assert callable(E.World.sense) and callable(E.World.sense_records) and callable(E.World.sense_rays_records)
    assert E.BEAM.itemsize == 16 and E.SENSOR.itemsize == 48 and ctypes.sizeof(E.SenseOut) == 4 * ctypes.sizeof(ctypes.c_void_p)


def _bodies(rng, n):
    bt = np.zeros(n, dtype=S.TRANSFORM)
    bt["position"] = rng.uniform(-50.0, 50.0, size=(n, 3))
    bt["rotation"] = HS.unit_quats(rng, n)
    bt["rotation"][0] = (0.0, 0.0, 0.0, 1.0)
    bt["position"][0] = 0.0
    return bt


@pytest.mark.parametrize("name", sorted(CU.HOST_WORLDS))
def test_the_rays_follow_the_contract_in_float64(name):
    """Each direction component is a dozen rounded operations on magnitudes of at most 2 |r| (the two cross products of nh_rotate and its sums), hence
    a bound near 24 x 2^-24 |r|; the rest of 32 x 2^-24 |r| is margin for the rounding of the quaternion itself.  The origin of a mounted sensor is the
    same rotation applied to its local position plus the body's: the bound scales with |local position| + |body position|.  max_t and ignore_body are
    copies."""
    rec, _ = CU.host_world(name)
    rng = np.random.default_rng(700 + sorted(CU.HOST_WORLDS).index(name))
    bt = _bodies(rng, 40)
    sensors = HS.sensors(rng, 60, rec, nbodies=len(bt), dynamic=np.arange(1, len(bt)))
    sensors = sensors[(sensors["body"] == NONE) | (sensors["body"] < len(bt))]       # (mounts that do not exist: the test of the invalid sensors)
    assert (sensors["body"] == NONE).sum() > 10 and (sensors["body"] == 0).sum() > 5 and ((sensors["body"] != NONE) & (sensors["body"] > 0)).sum() > 5
    beams = HS.pattern(rng, 65)
    for bodies in (bt, None):
        rays = HS.sense_rays(sensors, beams, bodies).reshape(len(sensors), len(beams))
        o64, d64 = HS.rays64(sensors, beams, bodies)
        rlen = np.linalg.norm(beams["direction"].astype(np.float64), axis=1)
        err = np.abs(rays["direction"].astype(np.float64) - d64).max(axis=2)
        assert (err <= 32 * EPS * rlen[None, :]).all(), float((err / np.maximum(rlen[None, :], 1e-30)).max() / EPS)
        mounted = np.zeros(len(sensors), dtype=bool) if bodies is None else sensors["body"] != NONE
        scale = np.linalg.norm(sensors["position"].astype(np.float64), axis=1)
        if bodies is not None:
            scale = scale + np.where(mounted, np.linalg.norm(bt["position"][np.where(mounted, sensors["body"], 0)].astype(np.float64), axis=1), 0.0)
        oerr = np.abs(rays["origin"].astype(np.float64) - o64).max(axis=2)
        assert (oerr[mounted] <= 32 * EPS * scale[mounted, None]).all()
        # a world-frame sensor's origin is its position, to the bit
        assert rays["origin"][~mounted].tobytes() == np.repeat(sensors["position"][~mounted][:, None, :], len(beams), axis=1).tobytes()
        assert rays["max_t"].tobytes() == np.tile(beams["range"], len(sensors)).tobytes()
        assert np.array_equal(rays["ignore_body"], np.repeat(sensors["ignore_body"][:, None], len(beams), axis=1))
        assert (rays["direction"][:, len(beams) // 2] == 0).all()                    # the zero beam stays zero


@pytest.mark.parametrize("name", sorted(CU.HOST_WORLDS))
def test_the_answers_are_the_ray_oracles_on_the_generated_rays(name):
    rec, nbox = CU.host_world(name)
    scene = CU.HOST_WORLDS[name]()
    bt = scene["body_transforms"]
    rng = np.random.default_rng(710 + sorted(CU.HOST_WORLDS).index(name))
    dynamic = np.unique(rec["body"][rec["body"] != 0])
    sensors = HS.sensors(rng, 48, rec, nbodies=len(bt), dynamic=dynamic, spoil=True)
    beams = HS.pattern(rng, 65)
    for bodies in (bt, None):
        rays = HS.sense_rays(sensors, beams, bodies)
        ref = HC.cast(HC.RAY, rec, nbox, rays)
        got = HS.sense(rec, nbox, sensors, beams, bodies)
        assert got["hits"].tobytes() == ref.tobytes()
        assert got["t"].tobytes() == ref["t"].tobytes() and got["body"].tobytes() == ref["body"].tobytes() and got["tag"].tobytes() == ref["tag"].tobytes()
        hit = (ref["shape"] != NONE).reshape(len(sensors), len(beams))
        kind = np.arange(len(sensors)) % 3                                           # inside the bounds, outside them, inside a collider
        valid = (np.isfinite(rays["origin"]).all(axis=1) & np.isfinite(rays["direction"]).all(axis=1)).reshape(len(sensors), len(beams)).all(axis=1)
        valid &= sensors["body"] == NONE                                             # (a mounted sensor's position is local: it is where its body is)
        assert hit[(kind == 0) & valid].any() and hit[(kind == 1) & valid].any() and not hit[(kind == 1) & valid].all()
        # from inside a collider every beam hits at t = 0, unless that collider's body is ignored
        t = ref["t"].reshape(len(sensors), len(beams))
        assert (t[(kind == 2) & valid & (sensors["ignore_body"] == NONE)] == 0).mean() > 0.9


def test_invalid_sensors_miss_with_nan_and_leave_their_neighbours_alone():
    rec, nbox = CU.host_world("pile")
    bt = CU.HOST_WORLDS["pile"]()["body_transforms"]
    rng = np.random.default_rng(720)
    good = HS.sensors(rng, 12, rec)
    good["body"] = 0
    beams = HS.pattern(rng, 20)
    bad = good.copy()
    bad["body"][1] = len(bt)                                                         # the mount index == count
    bad["body"][4] = 0xFFFFFFFE
    bad["rotation"][7, 1] = np.nan
    bad["position"][10, 2] = np.inf
    spoiled = np.zeros(len(good), dtype=bool)
    spoiled[[1, 4, 7, 10]] = True
    rays = HS.sense_rays(bad, beams, bt).reshape(len(bad), len(beams))
    # a mount that does not exist: all six words the quiet NaN, max_t and ignore_body as for any other ray
    for s in (1, 4):
        assert (rays["origin"][s].view(np.uint32) == QNAN).all() and (rays["direction"][s].view(np.uint32) == QNAN).all()
        assert rays["max_t"][s].tobytes() == beams["range"].tobytes() and (rays["ignore_body"][s] == bad["ignore_body"][s]).all()
    a, b = HS.sense(rec, nbox, good, beams, bt), HS.sense(rec, nbox, bad, beams, bt)
    for k in ("t", "body", "tag", "hits"):
        x, y = a[k].reshape(len(good), len(beams)), b[k].reshape(len(good), len(beams))
        assert x[~spoiled].tobytes() == y[~spoiled].tobytes(), k
    t = b["t"].reshape(len(good), len(beams))
    assert (t[spoiled].view(np.uint32) == QNAN).all()
    assert (b["body"].reshape(len(good), -1)[spoiled] == NONE).all() and (b["tag"].reshape(len(good), -1)[spoiled] == NONE).all()
    h = b["hits"].reshape(len(good), len(beams))[spoiled]
    assert (h["shape"] == NONE).all() and (h["collider"] == NONE).all() and not h["normal"].any()
    # without bodies the mount word is not read: those two are ordinary world-frame sensors
    c = HS.sense(rec, nbox, bad, beams, None)["t"].reshape(len(good), len(beams))
    assert not np.isnan(c[[1, 4]]).any()


def test_zero_directions_and_ranges_follow_the_ray_rules():
    rec, nbox = CU.host_world("pile")
    rng = np.random.default_rng(730)
    live = np.nonzero(np.isfinite(rec["p"]).all(axis=1))[0]
    s = np.zeros(2, dtype=E.SENSOR)
    s["rotation"], s["body"], s["ignore_body"] = HS.unit_quats(rng, 2), NONE, NONE
    s["position"][0] = rec["p"][live[3]]                                             # inside a collider
    s["position"][1] = rec["p"][live].max(axis=0) + (0.0, 30.0, 0.0)                 # above the scene
    beams = np.zeros(8, dtype=E.BEAM)
    beams["direction"] = [(0, 0, 0), (0, 0, 0), (0, -1, 0), (0, -1, 0), (0, -1, 0), (0, -1, 0), (0, -1, 0), (1, 2, 3)]
    beams["range"] = [np.inf, 5.0, 0.0, np.nan, np.inf, 1e-3, -1.0, np.inf]
    s["rotation"][1] = (0.0, 0.0, 0.0, 1.0)
    got = HS.sense(rec, nbox, s, beams)
    ref = HC.cast(HC.RAY, rec, nbox, HS.sense_rays(s, beams))
    assert got["hits"].tobytes() == ref.tobytes()
    h = got["hits"].reshape(2, 8)
    # a zero direction from inside a collider hits it at t = 0 (its normal is 0 / 0); from outside it misses with t = max_t
    assert h["t"][0, 0] == 0 and h["shape"][0, 0] != NONE and h["shape"][1, 0] == NONE and h["t"][1, 0] == np.inf and h["t"][1, 1] == 5.0
    # range 0 from inside: the hit at t = 0 counts; from above: a miss with t = 0
    assert h["shape"][0, 2] != NONE and h["t"][0, 2] == 0 and h["shape"][1, 2] == NONE and h["t"][1, 2] == 0
    # a NaN range never hits and is written back; +inf reaches the pile from above; a negative range never hits
    assert h["shape"][0, 3] == NONE and np.isnan(h["t"][0, 3]) and h["shape"][1, 3] == NONE and np.isnan(h["t"][1, 3])
    assert h["shape"][1, 4] != NONE and 0 < h["t"][1, 4] < np.inf
    assert h["shape"][1, 5] == NONE and h["t"][1, 5] == np.float32(1e-3)
    assert h["shape"][0, 6] == NONE and h["t"][0, 6] == -1.0


def test_masks_are_per_sensor_and_see_the_masked_world():
    import filter_util as F
    rec, nbox = CU.host_world("compound")
    rng = np.random.default_rng(740)
    sensors, beams = HS.sensors(rng, 24, rec), HS.pattern(rng, 33)
    words = F.layers(len(rec), 741)
    off = HS.sense(rec, nbox, sensors, beams)
    masks = rng.choice(np.uint32([0, 1, 6, NONE]), size=len(sensors))
    got = HS.sense(rec, nbox, sensors, beams, words=words, masks=masks)["hits"].reshape(len(sensors), len(beams))
    for v in (0, 1, 6, NONE):
        ref = HC.cast(HC.RAY, F.masked(rec, words, v), nbox, HS.sense_rays(sensors, beams)).reshape(len(sensors), len(beams))
        assert got[masks == v].tobytes() == ref[masks == v].tobytes(), v
        uni = HS.sense(rec, nbox, sensors, beams, words=words, masks=int(v))["hits"]
        assert uni.tobytes() == ref.tobytes(), v
    assert (got[masks == 0]["shape"] == NONE).all()
    assert HS.sense(rec, nbox, sensors, beams, words=None, masks=5)["hits"].tobytes() == off["hits"].tobytes()      # no layers set: all ones
    assert HS.sense(rec, nbox, sensors, beams, words=None, masks=0)["hits"]["shape"].max() == NONE and (HS.sense(rec, nbox, sensors, beams, masks=0)["body"] == NONE).all()


def test_the_pattern_helpers():
    beams, back = E.pinhole_beams(24, 16, np.radians(60.0), 50.0)
    row, _ = E.pinhole_beams(24, 16, np.radians(60.0), 50.0, tile=1)
    assert beams.dtype == E.BEAM and len(beams) == 24 * 16 and sorted(back) == list(range(24 * 16))
    assert beams[back].tobytes() == row.tobytes()                                     # un-permuted, the tiled pattern is the row-major one
    # a wave's 64 beams are an 8 x 8 patch: the first 64 cover columns 0 .. 7 of rows 0 .. 7
    img = np.zeros(24 * 16, dtype=np.int64)
    img[:] = np.arange(24 * 16)[back] // 64
    img = img.reshape(16, 24)
    assert (img[:8, :8] == 0).all() and (img[:8, 8:16] == 1).all() and (img[8:, :8] == 3).all()
    d = row["direction"].reshape(16, 24, 3)
    assert (d[..., 2] == -1).all() and d[0, 0, 0] < 0 < d[0, -1, 0] and d[0, 0, 1] > 0 > d[-1, 0, 1]
    assert np.isclose(d[0, :, 1].max(), np.tan(np.radians(30.0)) * (1 - 1 / 16)) and (row["range"] == 50.0).all()
    ragged, rback = E.pinhole_beams(13, 9, 1.0, 5.0)
    assert ragged[rback].tobytes() == E.pinhole_beams(13, 9, 1.0, 5.0, tile=1)[0].tobytes()
    lid = E.lidar_beams(np.linspace(0, 2 * np.pi, 128, endpoint=False), np.radians([-15.0, 0.0, 15.0]), 100.0)
    assert len(lid) == 3 * 128 and np.allclose(np.linalg.norm(lid["direction"], axis=1), 1.0, atol=1e-6)
    assert np.allclose(lid["direction"][128], (0.0, 0.0, -1.0), atol=1e-7) and np.allclose(lid["direction"][128 + 32], (1.0, 0.0, 0.0), atol=1e-6)
    assert lid["direction"][0, 1] < 0 < lid["direction"][256, 1]
