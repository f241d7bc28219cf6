"""Fast bodies on the host (no GPU): the selection, the cast records and the hits of nh_sweep and the factors of nh_sweep_limit (include/nudge_hip.h,
"fast bodies") through the oracle of tests/hostoracle/hostsweep.cpp, which runs nudge_amd/csrc/nh_query.h's own arithmetic -- the bits the device
computes.

The travel of a collider is checked against a float64 restatement that shares no code with it, the selection against the restated rule wherever the
float64 margin is clear of the threshold, the hits against the cast oracles the cast tests use (tests/hostcast_util.py) on the oracle's own records:
nh_sweep is nh_boxcast / nh_spherecast on the records it writes.  With the reference library present the wall scene of the issue is stepped with and
without the guard."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cast_util as CU                       # noqa: E402
import hostcast_util as HC                   # noqa: E402
import hostsweep_util as HS                  # noqa: E402
from hostsweep_util import NONE              # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402
from oracle import refworld                  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
needs_ref = pytest.mark.skipif(not refworld.available("exact"), reason="oracle/_ref not built (needs /root/reference: make -C oracle)")


def test_the_library_exports_the_sweep_calls(tmp_path):
    so = os.path.join(ROOT, "nudge_amd", "libnudge_hip.so")
    if not os.path.exists(so):
        E.build()
    lib = ctypes.CDLL(so)
    assert hasattr(lib, "nh_sweep") and hasattr(lib, "nh_sweep_limit")
    assert {"nh_sweep", "nh_sweep_limit"} <= set(E.EXPORTS)
    assert callable(E.World.sweep) and callable(E.World.sweep_records) and callable(E.World.sweep_limit_records)
    # the mirrors against what a C compiler makes of the header: nh_SweepParams is four words; nh_SweepList four pointers and two words -- 40 bytes on
    # LP64 (the issue's text says 48, which is not what the struct it defines measures)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nudge_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(nh_SweepParams), sizeof(nh_SweepList), offsetof(nh_SweepList, hits), offsetof(nh_SweepList, capacity));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert sizes == [ctypes.sizeof(E.SweepParams), ctypes.sizeof(E.SweepList), E.SweepList.hits.offset, E.SweepList.capacity.offset]
    assert sizes[0] == 16
    if ctypes.sizeof(ctypes.c_void_p) == 8:
        assert sizes[1] == 40


def _world(name, seed):
    """(records, nbox, body transforms, thrown momentum) of a HOST_WORLD, a collider of a body that does not exist among them."""
    rec, nbox = CU.host_world(name)
    scene = CU.HOST_WORLDS[name]()
    bt = scene["body_transforms"]
    rng = np.random.default_rng(seed)
    bm = HS.thrown(rng, len(bt))
    return rec, nbox, bt, bm, rng


@pytest.mark.parametrize("name", sorted(CU.HOST_WORLDS))
def test_travel_selection_and_records_follow_the_contract_in_float64(name):
    """A component of d is one subtraction (r), two products and their difference (the cross product), one sum (with v) and one product (with
    time_step): five roundings on the path, each relative to a magnitude of at most |v_k| + 2 |w| |r| (the subtraction of two floats is off by at most
    2^-24 of its own result), and the rounding of r carried through two products -- 8 x 2^-24 of (|v_k| + 2 |w| |r|) |time_step| bounds them.  |d|^2 then carries 2 x 8 + 3 roundings of the same scale squared
    and s^2 three: the rule is compared where the float64 margin exceeds 32 x 2^-24 of (scale^2 + s^2).  Every other word of a record is a copy or one
    product."""
    rec, nbox, bt, bm, rng = _world(name, 800 + sorted(CU.HOST_WORLDS).index(name))
    dyn = rec["body"] != 0
    for min_travel, core in HS.PARAMS:
        # capacity: every collider, so that the records of ALL colliders can be looked at through min_travel = -1 below; the call itself first
        got = HS.sweep(rec, nbox, bt, bm, min_travel=min_travel, core=core)
        sel = np.zeros(len(rec), dtype=bool)
        sel[got["colliders"][:got["total"]]] = True
        assert got["counts"][0] == sel[:nbox].sum() and got["counts"][1] == sel[nbox:].sum()
        assert (np.diff(got["colliders"][:got["total"]].astype(np.int64)) > 0).all()
        d64, scale = HS.travel64(rec, bt, bm, HS.TIME_STEP)
        casts = got["casts"][:got["total"]]
        c = got["colliders"][:got["total"]]
        fin = np.isfinite(d64[c]).all(axis=1)
        err = np.abs(casts["direction"][fin].astype(np.float64) - d64[c][fin])
        assert (err <= 8 * EPS * scale[c][fin]).all(), float((err / scale[c][fin]).max() / EPS)
        # the rule, where float64 is clear of the threshold
        with np.errstate(all="ignore"):
            d2, s2, sc2 = (d64 ** 2).sum(axis=1), (min_travel * HS.smallest_half(rec, nbox)) ** 2, (scale ** 2).sum(axis=1)
            clear = np.abs(d2 - s2) > 32 * EPS * (sc2 + s2)
            want = dyn & (d2 > s2)
        finite = np.isfinite(d2)
        assert clear[finite & dyn].mean() > 0.9
        assert np.array_equal(sel[clear & finite], want[clear & finite])
        # a NaN anywhere selects nobody, nor does body 0; an INFINITE travel is larger than any threshold by the rule as written -- its cast is
        # invalid and its hit a miss with t = NaN, which limits nothing
        assert np.isnan(d2[dyn]).any() and not sel[np.isnan(d2)].any() and not sel[~dyn].any()
        wild = sel & ~finite
        assert (d2[wild] == np.inf).all()
        lost = got["hits"][:got["total"]][~fin]
        assert (lost["shape"] == NONE).all() and np.isnan(lost["t"]).all()
        # bodies at rest are selected by nothing but min_travel = 0 ... and not by that either: 0 > 0 is false
        rest = dyn & (d2 == 0)
        assert rest.any() and not sel[rest].any()
        # the other words
        assert casts["origin"].tobytes() == rec["p"][c].tobytes() and (casts["max_t"] == 1.0).all() and np.array_equal(casts["ignore_body"], rec["body"][c])
        box = c < nbox
        assert casts["rotation"][box].tobytes() == rec["q"][c[box]].tobytes()
        assert casts["size"][box].tobytes() == (rec["h"][c[box]] * np.float32(core)).astype(np.float32).tobytes() and (casts["reserved"] == 0).all()
        balls = casts[~box].view(E.CAPSULE_CAST)
        assert (balls["rotation"] == np.float32(CU.IDENTITY)).all() and (balls["half_height"] == 0).all() and (balls["reserved"] == 0).all()
        assert balls["radius"].tobytes() == (rec["h"][c[~box], 0] * np.float32(core)).astype(np.float32).tobytes()
        if (min_travel, core) == (0.5, 0.5):
            share = sel[dyn & finite].mean()
            assert 0.25 <= share <= 0.75, share


@pytest.mark.parametrize("name", sorted(CU.HOST_WORLDS))
def test_the_hits_are_the_cast_oracles_on_the_oracles_own_records(name):
    rec, nbox, bt, bm, rng = _world(name, 810 + sorted(CU.HOST_WORLDS).index(name))
    some = 0
    for min_travel, core in HS.PARAMS:
        got = HS.sweep(rec, nbox, bt, bm, min_travel=min_travel, core=core)
        n, nb = got["total"], int(got["counts"][0])
        casts, hits = got["casts"][:n], got["hits"][:n]
        assert hits[:nb].tobytes() == HC.cast(HC.BOX, rec, nbox, casts[:nb]).tobytes()
        balls = casts[nb:].view(E.CAPSULE_CAST)
        assert hits[nb:].tobytes() == HC.cast(HC.CAPSULE, rec, nbox, balls).tobytes()
        assert hits[nb:].tobytes() == HC.cast(HC.SPHERE, rec, nbox, CU.as_balls(balls)).tobytes()
        assert (hits["body"] != casts["ignore_body"]).all()                          # nobody hits itself
        some += int((hits["shape"] != NONE).sum())
        if core == 0.0:
            assert n and nb and n > nb
    assert some > 20


def test_colliders_without_a_body_and_bodies_beyond_the_count_are_never_selected():
    rec, nbox, bt, bm, rng = _world("compound", 820)
    bm = HS.thrown(rng, len(bt), lo=100.0, spoil=False)                              # everybody is fast
    full = HS.sweep(rec, nbox, bt, bm)
    assert full["total"] == int((rec["body"] != 0).sum())
    cut = len(bt) - 7                                                                # the call names fewer bodies than the colliders do
    got = HS.sweep(rec, nbox, bt[:cut], bm[:cut])
    assert got["total"] == int(((rec["body"] != 0) & (rec["body"] < cut)).sum()) and (rec["body"][got["colliders"][:got["total"]]] < cut).all()
    lost = rec.copy()                                                                # a NaN pose: the record of a collider whose body does not exist
    gone = np.nonzero(rec["body"] != 0)[0][::5]
    lost["p"][gone] = np.nan
    got = HS.sweep(lost, nbox, bt, bm)
    assert got["total"] == full["total"] - len(gone) and not np.isin(gone, got["colliders"][:got["total"]]).any()


def _limited(rec, nbox, bt, bm, **kw):
    lst = HS.sweep(rec, nbox, bt, bm, **kw)
    n = lst["total"]
    lst = dict(counts=lst["counts"], colliders=lst["colliders"][:n], hits=lst["hits"][:n])
    factors, after = HS.sweep_limit(rec, lst, bm)
    return lst, factors, after


@pytest.mark.parametrize("name", sorted(CU.HOST_WORLDS))
def test_the_factors_and_the_momentum_follow_the_restated_rule(name):
    rec, nbox, bt, bm, rng = _world(name, 830 + sorted(CU.HOST_WORLDS).index(name))
    bm = HS.thrown(rng, len(bt), lo=20.0)                                           # fast enough for many hits
    bm["velocity"][:, 1] = -np.abs(bm["velocity"][:, 1])                             # towards the ground
    lst, factors, after = _limited(rec, nbox, bt, bm, min_travel=0.0, core=0.5)
    hits, bodies = lst["hits"], rec["body"][lst["colliders"]]
    # doctor a few records so that every clause of the rule is met: t == 0 entries beside t > 0 ones on one body
    want = HS.limit64(bodies, hits)
    assert factors.tobytes() == np.float32([want[int(b)] for b in bodies]).tobytes()
    assert sum(1 for f in want.values() if f < 1) > 5 and sum(1 for f in want.values() if f == 1) > 5
    expect = bm.copy()
    for b, f in want.items():
        if f < 1:
            expect["velocity"][b] = expect["velocity"][b] * np.float32(f)            # three products
    assert after.tobytes() == expect.tobytes()                                       # ... and every other byte as it was
    assert after["angular_velocity"].tobytes() == bm["angular_velocity"].tobytes() and after["unused0"].tobytes() == bm["unused0"].tobytes()


def test_start_overlaps_limit_nothing_and_compound_bodies_take_their_earliest_hit():
    rec, nbox, bt, bm, rng = _world("compound", 840)
    bm = HS.thrown(rng, len(bt), lo=50.0, spoil=False)
    bm["velocity"][:, 1] = -np.abs(bm["velocity"][:, 1])
    lst, _, _ = _limited(rec, nbox, bt, bm, min_travel=0.0, core=1.0)
    bodies = rec["body"][lst["colliders"]]
    several = [b for b in np.unique(bodies) if (bodies == b).sum() >= 3]
    assert len(several) > 10
    hits = lst["hits"].copy()
    b0, b1, b2 = several[0], several[1], several[2]
    e0, e1, e2 = np.nonzero(bodies == b0)[0], np.nonzero(bodies == b1)[0], np.nonzero(bodies == b2)[0]
    hits["shape"][e0], hits["t"][e0[0]], hits["t"][e0[1]], hits["t"][e0[2]] = E.NH_SHAPE_BOX, 0.0, 0.75, 0.25          # t == 0 ignored, the least of the rest
    hits["shape"][e1], hits["t"][e1] = E.NH_SHAPE_BOX, 0.0                                                            # only start overlaps: not limited
    hits["shape"][e2], hits["t"][e2] = NONE, 0.5                                                                      # misses limit nothing, whatever their t
    hits["t"][e2[1]], hits["shape"][e2[1]] = 1.0, E.NH_SHAPE_SPHERE                                                   # a hit at the very end: factor 1
    doctored = dict(counts=lst["counts"], colliders=lst["colliders"], hits=hits)
    factors, after = HS.sweep_limit(rec, doctored, bm)
    assert (factors[e0] == 0.25).all() and (factors[e1] == 1.0).all() and (factors[e2] == 1.0).all()
    assert after["velocity"][b0].tobytes() == (bm["velocity"][b0] * np.float32(0.25)).tobytes()
    assert after[b1].tobytes() == bm[b1].tobytes() and after[b2].tobytes() == bm[b2].tobytes()
    assert factors.tobytes() == np.float32([HS.limit64(bodies, hits)[int(b)] for b in bodies]).tobytes()


def test_capacity_is_all_or_none_and_the_counts_are_true_either_way():
    rec, nbox, bt, bm, rng = _world("pile", 850)
    full = HS.sweep(rec, nbox, bt, bm, fill=0xA5)
    n = full["total"]
    assert 0 < n < len(rec)
    for cap in (n - 1, 0):
        short = HS.sweep(rec, nbox, bt, bm, capacity=cap, fill=0xA5)
        assert np.array_equal(short["counts"], full["counts"])
        assert all(set(short[c].tobytes()) <= {0xA5} for c in E.SWEEP_CHANNELS)
        assert HS.sweep_limit(rec, dict(counts=short["counts"], colliders=short["colliders"], hits=short["hits"]), bm, capacity=cap)[1].tobytes() == bm.tobytes()
    exact = HS.sweep(rec, nbox, bt, bm, capacity=n, fill=0xA5)
    for c in E.SWEEP_CHANNELS:
        assert exact[c].tobytes() == full[c][:n].tobytes() and set(full[c][n:].tobytes()) == {0xA5}
    only = HS.sweep(rec, nbox, bt, bm, channels=("hits",))
    assert only["hits"].tobytes() == HS.sweep(rec, nbox, bt, bm)["hits"].tobytes() and "casts" not in only


def test_masks_are_per_collider_and_see_the_masked_world():
    import filter_util as F
    rec, nbox, bt, bm, rng = _world("compound", 860)
    bm = HS.thrown(rng, len(bt), lo=20.0)
    words = F.layers(len(rec), 861)
    off = HS.sweep(rec, nbox, bt, bm, min_travel=0.0)
    n, nb = off["total"], int(off["counts"][0])
    c = off["colliders"][:n]
    masks = rng.choice(np.uint32([0, 1, 6, NONE]), size=len(rec))
    got = HS.sweep(rec, nbox, bt, bm, min_travel=0.0, words=words, masks=masks)
    assert got["colliders"].tobytes() == off["colliders"].tobytes() and got["casts"].tobytes() == off["casts"].tobytes()     # the filter selects nobody
    differ = 0
    for v in (0, 1, 6, NONE):
        world = F.masked(rec, words, v)
        ref = np.concatenate([HC.cast(HC.BOX, world, nbox, off["casts"][:nb]), HC.cast(HC.CAPSULE, world, nbox, off["casts"][nb:n].view(E.CAPSULE_CAST))])
        mine = masks[c] == v
        assert mine.any() and got["hits"][:n][mine].tobytes() == ref[mine].tobytes(), v
        assert HS.sweep(rec, nbox, bt, bm, min_travel=0.0, words=words, masks=int(v))["hits"][:n].tobytes() == ref.tobytes(), v
        differ += int((ref["collider"] != off["hits"][:n]["collider"]).sum())
    assert differ > 0 and (got["hits"][:n][masks[c] == 0]["shape"] == NONE).all()
    assert HS.sweep(rec, nbox, bt, bm, min_travel=0.0, words=None, masks=5)["hits"].tobytes() == off["hits"].tobytes()          # no layers set: all ones


# ---- the wall scene: a thin wall, bullets at 240 m/s and 120 Hz -----------------------------------------------------------------------------------
def _fire(bullet, guard):
    """Steps the wall scene with one bullet 40 times in the reference; with `guard` the oracle's sweep and limit go before every step.  Returns the
    bullet's x after each step, whether a contact ever appeared, and its final speed."""
    scene, body = HS.wall_scene([bullet])
    w = refworld.RefWorld(scene)
    nbox = len(scene["box_tags"])
    xs, contact = [], False
    for _ in range(40):
        if guard:
            b = w.bodies()
            rec = HC.records(b["transforms"], scene)
            lst = HS.sweep(rec, nbox, b["transforms"], b["momentum"], time_step=scene["params"]["time_step"], min_travel=0.5, core=0.5)
            n = lst["total"]
            _, after = HS.sweep_limit(rec, dict(counts=lst["counts"], colliders=lst["colliders"][:n], hits=lst["hits"][:n]), b["momentum"])
            w.set_bodies(momentum=after)
        w.step(1)
        contact = contact or w.contacts()["count"] > 0
        xs.append(float(w.bodies()["transforms"]["position"][body[0], 0]))
    return np.array(xs), contact, float(np.linalg.norm(w.bodies()["momentum"]["velocity"][body[0]]))


@needs_ref
@pytest.mark.parametrize("bullet", [("sphere", 0.25, 0.0, 240.0), ("box", 0.2, 0.0, 240.0)], ids=["sphere", "box"])
def test_the_guard_stops_a_bullet_the_reference_lets_through(bullet):
    xs, contact, speed = _fire(bullet, guard=False)
    assert xs[-1] > 0 and not contact and xs[0] == -1.0 and xs[1] == 1.0             # it tunnels: -1, +1, +3, ...
    xs, contact, speed = _fire(bullet, guard=True)
    assert xs.max() <= -0.05, xs.max()                                               # the centre never reaches the wall's face
    assert contact and speed < 1.0, (contact, speed)
