"""What the scene-query tests share: the small scenes, the bounds of a world's colliders, random unit quaternions, rays around a scene, the upload of
numpy records, a world's collider records, and the comparison of two worlds that must have stepped alike (queries are observers)."""
import numpy as np

import hostlib
import parity_util as P
from nudge_amd import engine as E
from nudge_amd import scenes as S

NONE = 0xFFFFFFFF
FUSED = E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP

SMALL = {
    "pile": lambda: S.pile(256, 64, seed=1),
    "compound": lambda: S.compound(150, seed=6),
    "stacks": lambda: S.stacks(64, 3, seed=5),
    "grid_tiles": lambda: S.grid_tiles(4, side=16, sphere_fraction=0.5, seed=2),
    "ball_pit": lambda: S.ball_pit(6, 6, 6, seed=4),
}
# the worlds of the observer tests: queries between their steps must change nothing
OBSERVED = {"pile": lambda: S.pile(256, 0, seed=1), "grid_tiles": lambda: S.grid_tiles(2, side=20, seed=2)}


def bounds(rec):
    """(lowest, highest) centre of the colliders with a finite pose (float64)."""
    p = rec["p"][np.isfinite(rec["p"]).all(axis=1)].astype(np.float64)
    return p.min(axis=0), p.max(axis=0)


def unit_quats(rng, n):
    """n unit quaternions (float32): one rng.normal(size=(n, 4)) draw, normalised in float64."""
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def mat(q):
    """The rotation matrix of the quaternion q = (x, y, z, s), in float64."""
    x, y, z, s = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y)],
                     [2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)],
                     [2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)]])


def rays(rng, n, lo, hi, kind, max_t=np.inf):
    """`kind`: random origins / directions around the scene; axis-aligned (one or two direction components exactly zero); a downward grid."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    span = np.maximum(hi - lo, 1.0)
    r = np.zeros(n, dtype=E.RAY)
    r["max_t"] = max_t
    r["ignore_body"] = NONE
    if kind == "random":
        r["origin"] = rng.uniform(lo - 0.2 * span, hi + 0.2 * span, size=(n, 3))
        aim = rng.uniform(lo, hi, size=(n, 3))
        d = aim - r["origin"]
        r["direction"] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.25, 4.0, size=(n, 1))
    elif kind == "axis":
        r["origin"] = rng.uniform(lo - 0.1 * span, hi + 0.1 * span, size=(n, 3))
        d = np.zeros((n, 3))
        ax = rng.integers(0, 3, size=n)
        d[np.arange(n), ax] = rng.choice([-1.0, 1.0], size=n) * rng.uniform(0.5, 2.0, size=n)
        two = rng.random(n) < 0.3          # (a third of them with one zero component only)
        ax2 = (ax + 1) % 3
        d[two, ax2[two]] = rng.uniform(-1.0, 1.0, size=int(two.sum()))
        r["direction"] = d
    else:
        side = int(np.sqrt(n))
        gx, gz = np.meshgrid(np.linspace(lo[0], hi[0], side), np.linspace(lo[2], hi[2], n // side + 1))
        r["origin"][:, 0] = gx.reshape(-1)[:n]
        r["origin"][:, 1] = hi[1] + 5.0
        r["origin"][:, 2] = gz.reshape(-1)[:n]
        r["direction"] = (0.0, -1.0, 0.0)
    return r


def upload(w, records):
    """The numpy records as bytes on the device of the world `w`."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).copy()).to(w.dev)


def records(w, scene):
    """The collider records of the world `w` as its bodies stand now."""
    return hostlib.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)


# what nh_read_counts reports of a context's history, not of its last step: tallies over its whole life, and the large colliders of the broadphase's last grid --
# built whenever this context last had to (a context that rebuilt eight steps in a row searches directly for a while: same pairs, another grid)
BY_HISTORY = ("large_colliders", "broadphase_rebuilds", "sort_reuses", "broadphase_inserts", "still_steps", "still_replays", "still_diff_key", "still_diff_count", "still_diff_feature",
           "still_diff_escape", "asleep_steps", "ahead_steps", "fused_steps", "pair_steps", "pair_diag_roles", "pair_diag_record", "pair_diag_scale", "pair_diag_owned")


def same_stepped_world(a, b, what, history=True):
    """history=False: for two contexts of different age, which can only agree about the last step."""
    ba, bb = a.get_bodies(), b.get_bodies()
    assert P.bits_equal(ba["transforms"], bb["transforms"]) and P.bits_equal(ba["momentum"], bb["momentum"]) and np.array_equal(ba["idle"], bb["idle"]), what
    a.export_views(E.NH_VIEW_ALL)
    b.export_views(E.NH_VIEW_ALL)
    ka, kb = a.get_contacts(), b.get_contacts()
    assert ka["count"] == kb["count"] and ka["data"].tobytes() == kb["data"].tobytes() and np.array_equal(ka["tags"], kb["tags"]), what
    assert np.array_equal(ka["features"], kb["features"]) and np.array_equal(ka["bodies"], kb["bodies"]) and np.array_equal(ka["sleeping_pairs"], kb["sleeping_pairs"]), what
    ca, cb = a.get_cache(), b.get_cache()
    assert ca["count"] == cb["count"] and ca["data"].tobytes() == cb["data"].tobytes() and np.array_equal(ca["tags"], cb["tags"]), what
    assert np.array_equal(a.get_active(), b.get_active()), what
    na, nb = a.counts(), b.counts()
    if not history:
        na, nb = ({k: v for k, v in n.items() if k not in BY_HISTORY} for n in (na, nb))
    assert na == nb, (what, na, nb)
