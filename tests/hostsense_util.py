"""ctypes access to the sensor oracle of tests/hostoracle/hostsense.cpp (built by tests/hostlib.py), and what the sensor tests share
(tests/test_cpu_sense.py, tests/test_gpu_sense.py): hs_sense_rays -- the ray of every (sensor, beam) by the arithmetic of nudge_amd/csrc/nh_query.h with
the device's bits -- and hs_sense -- the brute-force closest hit of each such ray, under layer words and one mask per sensor --, the sensor and beam
batches, and a float64 restatement of the ray that shares no code with either."""
import ctypes as C

import numpy as np

import hostlib as H
from nudge_amd import engine as E
from nudge_amd import scenes as S

NONE = 0xFFFFFFFF
QNAN = 0x7FC00000

lib = H.oracle({
    "hs_sense_rays": ([C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32], None),
    "hs_sense": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                  C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32], None),
})


def _bodies(body_transforms):
    if body_transforms is None:
        return None, None, 0
    bt = np.ascontiguousarray(body_transforms, dtype=S.TRANSFORM)
    return bt, H.p(bt), len(bt)


def sense_rays(sensors, beams, body_transforms=None, threads=None):
    """The nh_Ray records (E.RAY, count * beam_count) of nh_sense_rays; body_transforms None: the call without bodies."""
    sensors, beams = np.ascontiguousarray(sensors, dtype=E.SENSOR), np.ascontiguousarray(beams, dtype=E.BEAM)
    rays = np.zeros(len(sensors) * len(beams), dtype=E.RAY)
    _, bp, nb = _bodies(body_transforms)
    lib().hs_sense_rays(H.p(sensors), len(sensors), H.p(beams), len(beams), bp, nb, H.p(rays), H.threads(threads))
    return rays


def sense(rec, nbox, sensors, beams, body_transforms=None, words=None, masks=None, threads=None, channels=E.SENSE_CHANNELS):
    """dict(t, body, tag, hits) of nh_sense by brute force over `rec` (hostlib.REC), or those of `channels`.  masks None: the filter is off; an int:
    every sensor uses it; an array: sensor s uses masks[s].  words: the colliders' layer words (None: all ones)."""
    sensors, beams = np.ascontiguousarray(sensors, dtype=E.SENSOR), np.ascontiguousarray(beams, dtype=E.BEAM)
    rec = np.ascontiguousarray(rec, dtype=H.REC)
    n = len(sensors) * len(beams)
    dtypes = dict(t=np.float32, body=np.uint32, tag=np.uint32, hits=E.RAY_HIT)
    out = {c: np.zeros(n, dtype=dtypes[c]) for c in channels}
    _, bp, nb = _bodies(body_transforms)
    wp = None if words is None else np.ascontiguousarray(words, dtype=np.uint32)
    per = None if masks is None or np.isscalar(masks) else np.ascontiguousarray(masks, dtype=np.uint32)
    assert per is None or len(per) == len(sensors)
    lib().hs_sense(H.p(rec), len(rec), nbox, H.p(sensors), len(sensors), H.p(beams), len(beams), bp, nb, 0 if masks is None else 1,
                   None if wp is None else H.p(wp), None if per is None else H.p(per), int(masks) & NONE if np.isscalar(masks) else 0,
                   *[H.p(out[c]) if c in out else None for c in E.SENSE_CHANNELS], H.threads(threads))
    return out


# ---- batches ------------------------------------------------------------------------------------------------------------------------------------
def unit_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def pattern(rng, m):
    """m beams: random unit directions scaled by 0.25 .. 4, a zero direction and an axis-parallel one among them (from m = 3 on), ranges infinite, a
    few scene sizes, and zero."""
    d = rng.normal(size=(m, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.25, 4.0, size=(m, 1))
    b = np.zeros(m, dtype=E.BEAM)
    b["direction"] = d
    b["range"] = rng.choice(np.float32([np.inf, np.inf, 100.0, 10.0, 2.0]), size=m)
    if m >= 3:
        b["direction"][m // 2] = 0.0
        b["direction"][m - 1] = (0.0, -1.5, 0.0)
        b["range"][m - 1] = np.inf
    if m >= 8:
        b["range"][3] = 0.0
    return b


def sensors(rng, n, rec, nbodies=0, dynamic=(), spoil=False):
    """n sensors around the colliders of `rec`: inside the scene's bounds, outside them and at a collider's centre in turn; one in four ignores a body.
    nbodies > 0: they are mounted in turn on nothing (world frame), body 0, a body of `dynamic` (local poses near the body) and -- two of a batch of
    eight or more -- bodies that do not exist (nbodies itself and 0xfffffffe).  spoil: a NaN rotation and an infinite position as well."""
    live = np.nonzero(np.isfinite(rec["p"]).all(axis=1))[0]
    lo, hi = rec["p"][live].min(axis=0) - 1.0, rec["p"][live].max(axis=0) + 1.0
    span = hi - lo
    s = np.zeros(n, dtype=E.SENSOR)
    s["reserved"] = rng.integers(0, 1 << 32, size=(n, 3), dtype=np.uint64).astype(np.uint32)           # never read
    s["body"] = NONE
    s["ignore_body"] = NONE
    s["rotation"] = unit_quats(rng, n)
    kind = np.arange(n) % 3
    s["position"] = rng.uniform(lo, hi, size=(n, 3))
    out = kind == 1
    s["position"][out] = (rng.uniform(lo, hi, size=(n, 3)) + rng.choice([-1.0, 1.0], size=(n, 3)) * span)[out]
    ins = kind == 2
    s["position"][ins] = rec["p"][rng.choice(live, size=int(ins.sum()))] + rng.normal(scale=0.02, size=(int(ins.sum()), 3)).astype(np.float32)
    ign = rng.random(n) < 0.25
    s["ignore_body"][ign] = rec["body"][rng.choice(live, size=int(ign.sum()))]
    if nbodies:
        mount = (np.arange(n) // 3) % 3
        s["body"][mount == 1] = 0
        dyn = np.nonzero(mount == 2)[0]
        if len(dynamic):
            s["body"][dyn] = rng.choice(np.asarray(dynamic, dtype=np.uint32), size=len(dyn))
            s["position"][dyn] = rng.normal(scale=1.5, size=(len(dyn), 3))
        if n >= 8:
            s["body"][n - 2], s["body"][n - 3] = nbodies, 0xFFFFFFFE
    if spoil and n >= 8:
        s["rotation"][1, 2] = np.nan
        s["position"][4, 0] = np.inf
    return s


# ---- the contract in float64 ----------------------------------------------------------------------------------------------------------------------
def _matrix64(q):
    q = np.asarray(q, dtype=np.float64)
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rays64(sensors, beams, body_transforms=None):
    """(origins, directions) in float64, (count, beam_count, 3) each, of valid sensors: the rotation matrix of the normalised quaternion applied to the
    beam, the pose composed with the mount's where there is one."""
    o = np.zeros((len(sensors), len(beams), 3))
    d = np.zeros((len(sensors), len(beams), 3))
    for i, s in enumerate(sensors):
        R, p = _matrix64(s["rotation"]), s["position"].astype(np.float64)
        if body_transforms is not None and s["body"] != NONE:
            b = body_transforms[int(s["body"])]
            Rb = _matrix64(b["rotation"])
            R, p = Rb @ R, Rb @ p + b["position"].astype(np.float64)
        o[i] = p
        d[i] = beams["direction"].astype(np.float64) @ R.T
    return o, d
