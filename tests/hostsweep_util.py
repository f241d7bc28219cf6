"""ctypes access to the fast-body oracle of tests/hostoracle/hostsweep.cpp (built by tests/hostlib.py), and what the sweep tests share
(tests/test_cpu_sweep.py, tests/test_gpu_sweep.py): hs_sweep -- selection, cast records and hits of nh_sweep by the arithmetic of
nudge_amd/csrc/nh_query.h with the device's bits and a brute force over all colliders -- and hs_sweep_limit -- the factors and the new momentum of
nh_sweep_limit --, the momentum the tests throw the bodies with, float64 restatements of the travel, the selection rule and the limit rule that share
no code with either, and the wall scene of the issue."""
import ctypes as C

import numpy as np

import hostlib as H
from nudge_amd import engine as E
from nudge_amd import scenes as S

NONE = 0xFFFFFFFF
PARAMS = ((0.5, 0.5), (0.0, 1.0), (1e-3, 0.0))            # (min_travel, core)
# of speeds log-uniform from 1e-3 to 600 m/s a fifth carries a unit-sized collider further than half its half extent in 1 / 60 s, a third in 1 / 20 s: the
# tests want between a quarter and three quarters selected at (0.5, 0.5)
TIME_STEP = 1.0 / 20.0

lib = H.oracle({
    "hs_sweep": ([C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p,
                  C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32, C.c_uint32], None),
    "hs_sweep_limit": ([C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p], None),
})


def sweep(rec, nbox, transforms, momentum, time_step=TIME_STEP, min_travel=0.5, core=0.5, capacity=None, words=None, masks=None, channels=E.SWEEP_CHANNELS,
          fill=None, threads=None):
    """dict(counts, colliders, casts, hits, total) of nh_sweep by brute force over `rec` (hostlib.REC).  capacity None: room for every collider.
    masks None: the filter is off; an int: every collider uses it; an array: collider c uses masks[c].  words: the layer words (None: all ones).
    `fill`: the byte the channels hold before the call (None: zeros); records the call does not write keep it.  The channels come back `capacity` long."""
    rec = np.ascontiguousarray(rec, dtype=H.REC)
    bt, bm = np.ascontiguousarray(transforms, dtype=S.TRANSFORM), np.ascontiguousarray(momentum, dtype=S.MOMENTUM)
    assert len(bt) == len(bm)
    cap = len(rec) if capacity is None else int(capacity)
    dtypes = dict(colliders=np.uint32, casts=E.BOX_CAST, hits=E.RAY_HIT)
    out = {c: np.zeros(cap, dtype=dtypes[c]) for c in channels}
    if fill is not None:
        for c in out:
            out[c].view(np.uint8)[:] = fill
    counts = np.zeros(2, dtype=np.uint32)
    wp = None if words is None else np.ascontiguousarray(words, dtype=np.uint32)
    per = None if masks is None or np.isscalar(masks) else np.ascontiguousarray(masks, dtype=np.uint32)
    assert per is None or len(per) == len(rec)
    lib().hs_sweep(H.p(rec), len(rec), nbox, H.p(bt), H.p(bm), len(bt), time_step, min_travel, core, 0 if masks is None else 1,
                   None if wp is None else H.p(wp), None if per is None else H.p(per), int(masks) & NONE if np.isscalar(masks) else 0,
                   H.p(counts), *[H.p(out[c]) if c in out and cap else None for c in E.SWEEP_CHANNELS], cap, H.threads(threads))
    out["counts"], out["total"] = counts, int(counts.sum())
    return out


def sweep_limit(rec, lst, momentum, capacity=None):
    """(factors, new momentum) of nh_sweep_limit on the list `lst` (sweep()'s dict, or counts / colliders / hits arrays); factors: one per entry."""
    rec = np.ascontiguousarray(rec, dtype=H.REC)
    bm = np.ascontiguousarray(momentum, dtype=S.MOMENTUM).copy()
    counts = np.ascontiguousarray(lst["counts"], dtype=np.uint32)
    colliders, hits = np.ascontiguousarray(lst["colliders"], dtype=np.uint32), np.ascontiguousarray(lst["hits"], dtype=E.RAY_HIT)
    cap = len(colliders) if capacity is None else int(capacity)
    factors = np.ones(max(cap, 1), dtype=np.float32)
    lib().hs_sweep_limit(H.p(rec), len(rec), H.p(counts), H.p(colliders), H.p(hits), cap, H.p(bm), len(bm), H.p(factors))
    return factors[:int(counts.sum())] if int(counts.sum()) <= cap else factors[:0], bm


# ---- momentum -------------------------------------------------------------------------------------------------------------------------------------
def thrown(rng, n, lo=1e-3, hi=600.0, spoil=True):
    """S.MOMENTUM for n bodies: speeds log-uniform from `lo` to `hi` m/s in random directions, spins of a few rad/s, the unused words random bits;
    with `spoil` a few NaN and infinite words and a few bodies exactly at rest (from 16 bodies on).  Body 0 gets a velocity too: it is never swept."""
    m = np.zeros(n, dtype=S.MOMENTUM)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    m["velocity"] = d * np.exp(rng.uniform(np.log(lo), np.log(hi), size=(n, 1)))
    m["angular_velocity"] = rng.normal(size=(n, 3)) * rng.uniform(0.0, 5.0, size=(n, 1))
    m["unused0"] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    m["unused1"] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    if spoil and n >= 16:
        bad = rng.choice(np.arange(1, n), size=8, replace=False)
        m["velocity"][bad[0], 1] = np.nan
        m["velocity"][bad[1], 0] = np.inf
        m["angular_velocity"][bad[2], 2] = np.nan
        m["angular_velocity"][bad[3], 0] = -np.inf
        m["velocity"][bad[4:]] = 0.0
        m["angular_velocity"][bad[4:]] = 0.0
    return m


# ---- the contract in float64 ------------------------------------------------------------------------------------------------------------------------
def travel64(rec, transforms, momentum, time_step):
    """(d, scale) in float64 for every collider whose body exists: d = (v + w x (p_c - p_b)) * time_step, and the magnitude the rounding bound scales
    with, (|v_k| + 2 |w| |p_c - p_b|) * |time_step| per component (largest components of w and of the arm).  Rows of colliders without a body are NaN."""
    n = len(rec)
    b = rec["body"].astype(np.int64)
    ok = b < len(transforms)
    bb = np.where(ok, b, 0)
    pc, pb = rec["p"].astype(np.float64), transforms["position"][bb].astype(np.float64)
    v, w = momentum["velocity"][bb].astype(np.float64), momentum["angular_velocity"][bb].astype(np.float64)
    with np.errstate(all="ignore"):
        d = (v + np.cross(w, pc - pb)) * time_step
        scale = (np.abs(v) + 2.0 * np.abs(w).max(axis=1, keepdims=True) * np.abs(pc - pb).max(axis=1, keepdims=True)) * abs(time_step)
    d[~ok] = np.nan
    return d.reshape(n, 3), scale.reshape(n, 3)


def smallest_half(rec, nbox):
    """m of the rule: the smallest half extent of a box, the radius of a sphere (float64)."""
    h = rec["h"].astype(np.float64)
    return np.where(np.arange(len(rec)) < nbox, h.min(axis=1), h[:, 0])


def limit64(bodies_of_entries, hits):
    """{body: factor} by the rule in plain Python: the least t over the body's entries with a real hit and t > 0, else 1."""
    f = {}
    for b, h in zip(bodies_of_entries, hits):
        f.setdefault(int(b), np.float32(1.0))
        if h["shape"] != NONE and h["t"] > 0 and h["t"] < f[int(b)]:
            f[int(b)] = h["t"]
    return f


# ---- the wall scene -----------------------------------------------------------------------------------------------------------------------------------
def wall_scene(bullets):
    """A static wall of half extents (0.05, 5, 5) at the origin (body 0) and one body per bullet, each (shape, size, z, speed) or (shape, size, z, speed, x): a
    sphere of radius `size` or a box of half extent `size` at (x, 0, z), x = -3 unless given, fired at +x with `speed` m/s.  No gravity, no damping, time_step 1 / 120.  Returns
    (scene, body of each bullet): the bodies of the boxes come first (nudge_amd/scenes.py)."""
    f = np.float32
    wall = S._identity_transforms(1)
    of = {"box": [i for i, b in enumerate(bullets) if b[0] == "box"], "sphere": [i for i, b in enumerate(bullets) if b[0] == "sphere"]}

    def bodies(idx):
        t = S._identity_transforms(len(idx))
        t["position"] = [(bullets[i][4] if len(bullets[i]) > 4 else -3.0, 0.0, bullets[i][2]) for i in idx] if idx else np.zeros((0, 3))
        return t, np.array([bullets[i][1] for i in idx], dtype=f)

    bt, bs = bodies(of["box"])
    st, sr = bodies(of["sphere"])
    scene = S._assemble((wall, np.array([[0.05, 5.0, 5.0]], dtype=f)), (bt, np.stack([bs, bs, bs], axis=1).reshape(-1, 3), S._box_properties(bs, bs, bs)),
                        (st, sr, S._sphere_properties(sr)), dict(time_step=1.0 / 120.0, gravity=0.0, damping_rate=0.0, iterations=8), name="wall")
    body = np.zeros(len(bullets), dtype=np.int64)
    body[of["box"]] = 1 + np.arange(len(of["box"]))
    body[of["sphere"]] = 1 + len(of["box"]) + np.arange(len(of["sphere"]))
    scene["body_momentum"]["velocity"][body, 0] = [b[3] for b in bullets]
    return scene, body
