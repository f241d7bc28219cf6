"""The pure parts of tools/rates.py (no GPU): the statistics, the log, the spot-check indices, the workloads more than one rate tool times, and what
landed() derives from the scene."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rates                                 # noqa: E402
import hostquery_util as Q                   # noqa: E402
import walk_batches as WB                    # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

N = 64
LO, HI = np.array([-3.0, -1.0, -5.0]), np.array([7.0, 2.0, 4.0])          # a hand-made bounds box
LIVE = np.array([[0.0, 0.5, 0.0], [1.5, 0.75, -2.0], [-2.0, 1.0, 3.0], [6.0, 0.5, -4.0], [3.0, 1.5, 1.0]])          # a handful of positions inside it


def unit(v):
    return np.abs(np.linalg.norm(np.asarray(v, dtype=np.float64), axis=-1) - 1.0).max() <= 1e-6


def inside(p, lo, hi):
    p = np.asarray(p, dtype=np.float64)
    return bool((p >= lo - 1e-5).all() and (p <= hi + 1e-5).all())


@pytest.fixture(scope="module")
def small():
    """grid_tiles(2, side=12): the scene, and its collider records where it starts (the CPU stands in for the landed world)."""
    scene = S.grid_tiles(2, side=12, seed=2, lattice_cols=11)
    return scene, Q.records(scene["body_transforms"], scene)


def test_spread_is_median_min_max_as_plain_floats():
    s = rates.spread(np.array([3.0, 1.0, 10.0, 2.0], dtype=np.float32))
    assert s == dict(ms=2.5, min=1.0, max=10.0)
    assert all(type(v) is float for v in s.values())
    assert rates.spreads({"a": [1.0, 2.0, 4.0]}) == {"a": dict(ms=2.0, min=1.0, max=4.0)}
    assert rates.best_median([3.0, 1.0, 2.0]) == (1.0, 2.0)
    assert rates.fmt(s) == "2.500 (1.000 .. 10.000)" and rates.fmt_best(s) == "1.000 best, 2.500 (1.000 .. 10.000)"


def test_log_round_trips_through_a_file(tmp_path, capsys):
    log = rates.Log()
    log.say("first")
    log.say()
    log.say("\nwith a break")
    path = tmp_path / "deeper" / "x.log"
    log.write(str(path))
    assert path.read_text() == "first\n\n\nwith a break\n" == capsys.readouterr().out == log.text()


def test_spot_is_258_sorted_distinct_indices_and_everything_below_that():
    pick = rates.spot(1 << 20)
    assert len(pick) == 258 and (np.diff(pick) > 0).all() and 0 <= pick[0] and pick[-1] < (1 << 20)
    assert np.array_equal(pick, np.sort(np.random.default_rng(3).choice(1 << 20, size=258, replace=False)))          # the indices the tools have always drawn
    assert np.array_equal(rates.spot(1 << 20), pick)
    # fewer records than the spot check wants: every record is checked, once
    assert np.array_equal(rates.spot(100), np.arange(100))
    assert np.array_equal(rates.spot(258), np.arange(258))
    assert len(rates.spot(0)) == 0


def test_world_arguments_and_names():
    a = rates.parser("some_rates").parse_args([])
    assert (a.steps, a.tiles, a.world_side) == (70, 124, 90) and a.out == os.path.join(ROOT, "profiles", "some_rates.log")
    assert rates.world_name(a.tiles, a.world_side) == "config-2"
    a = rates.parser("some_rates").parse_args(["--tiles", "2", "--side", "12", "--steps", "5"])
    assert rates.world_flags(a) == ["--steps", "5", "--tiles", "2", "--side", "12"] and rates.world_name(2, 12) == "2-tile side-12"
    ap = rates.parser("sense_rates", side_flag="--world-side")          # a tool whose --side is its own
    ap.add_argument("--side", type=int, default=64)
    a = ap.parse_args(["--side", "8"])
    assert (a.side, a.world_side) == (8, 90) and ap.parse_args(["--world-side", "12"]).world_side == 12


def test_ray_sets():
    inc, coh = rates.ray_sets(np.random.default_rng(1), N, LO, HI)
    again = rates.ray_sets(np.random.default_rng(1), N, LO, HI)
    assert inc.tobytes() == again[0].tobytes() and coh.tobytes() == again[1].tobytes()
    assert inc.tobytes() != rates.ray_sets(np.random.default_rng(2), N, LO, HI)[0].tobytes()
    for r in (inc, coh):
        assert r.dtype == E.RAY and r.shape == (N,)
        assert np.isinf(r["max_t"]).all() and (r["ignore_body"] == rates.NONE).all()
        assert unit(r["direction"])
    assert inside(inc["origin"], LO, HI + np.array([0.0, 60.0, 0.0]))
    assert (coh["direction"] == np.array([0.0, -1.0, 0.0], dtype=np.float32)).all() and (coh["origin"][:, 1] == 30.0).all()
    assert inside(coh["origin"][:, [0, 2]], LO[[0, 2]], HI[[0, 2]])
    assert len(np.unique(coh["origin"][:, 0])) == N          # below 1,024 rays the grid is one row


def test_cast_records_and_rotations():
    inc, _ = rates.ray_sets(np.random.default_rng(1), N, LO, HI)
    rot = rates.random_rotations(N)
    assert rot.dtype == np.float32 and rot.shape == (N, 4) and unit(rot) and rot.tobytes() == rates.random_rotations(N).tobytes()
    ball = rates.cast_records(inc, E.SPHERE_CAST, radius=0.75)
    box = rates.cast_records(inc, E.BOX_CAST, size=0.75)
    cap = rates.cast_records(inc, E.CAPSULE_CAST, rotation=rot, radius=0.5, half_height=2.0)
    for c, dtype in ((ball, E.SPHERE_CAST), (box, E.BOX_CAST), (cap, E.CAPSULE_CAST)):
        assert c.dtype == dtype and c.shape == (N,)
        for k in rates.RAY_FIELDS:
            assert c[k].tobytes() == inc[k].tobytes()
    assert (ball["radius"] == 0.75).all() and (box["size"] == 0.75).all() and (cap["radius"] == 0.5).all() and (cap["half_height"] == 2.0).all()
    assert (box["rotation"] == np.array([0, 0, 0, 1], dtype=np.float32)).all() and cap["rotation"].tobytes() == rot.tobytes()


def test_point_sets_and_queries():
    sets = rates.point_sets(np.random.default_rng(5), N, LIVE, LO, HI)
    again = rates.point_sets(np.random.default_rng(5), N, LIVE, LO, HI)
    assert [s[0] for s in sets] == ["near bodies, max 2", "uniform in bounds, inf", "20 m above the pile, inf"] and [s[2] for s in sets] == [2.0, np.inf, np.inf]
    for (_, p, _), (_, p2, _) in zip(sets, again):
        assert p.dtype == np.float64 and p.shape == (N, 3) and p.tobytes() == p2.tobytes()
    near, uniform, above = (s[1] for s in sets)
    assert (np.linalg.norm(near[:, None, :] - LIVE[None], axis=2).min(axis=1) < 4.0).all()          # 0.5 a standard deviation around a body
    assert inside(uniform, LO, HI)
    assert inside(above[:, [0, 2]], LO[[0, 2]], HI[[0, 2]]) and (above[:, 1] == LIVE[:, 1].max() + 20.0).all()
    # tools/distance_rates.py's order of draws: the same three kinds of set, other bytes
    first = rates.point_sets(np.random.default_rng(5), N, LIVE, LO, HI, above_first=True)
    assert [s[0] for s in first] == [s[0] for s in sets]
    assert np.array_equal(first[2][1][:, [0, 2]], np.random.default_rng(5).uniform(LO, HI, size=(N, 3))[:, [0, 2]])          # the generator's first draw
    assert first[2][1].tobytes() != above.tobytes() and inside(first[1][1], LO, HI) and (first[2][1][:, 1] == LIVE[:, 1].max() + 20.0).all()
    q = rates.point_queries(uniform, np.inf)
    assert q.dtype == E.POINT_QUERY and q.shape == (N,) and np.isinf(q["max_distance"]).all() and (q["ignore_body"] == rates.NONE).all()
    assert q["point"].tobytes() == uniform.astype(np.float32).tobytes()


def test_overlap_queries_and_spheres_on_bodies():
    q = rates.spheres_on_bodies(np.random.default_rng(1), N, LIVE)
    assert q.tobytes() == rates.spheres_on_bodies(np.random.default_rng(1), N, LIVE).tobytes()
    assert q.dtype == E.OVERLAP_QUERY and q.shape == (N,) and (q["shape"] == E.NH_SHAPE_SPHERE).all() and (q["size"] == np.array([1, 0, 0], dtype=np.float32)).all()
    assert unit(q["rotation"]) and (q["ignore_body"] == rates.NONE).all()
    assert (np.linalg.norm(q["center"].astype(np.float64)[:, None, :] - LIVE[None], axis=2).min(axis=1) < 2.0).all()
    b = rates.overlap_queries(LIVE, np.full((len(LIVE), 3), 0.5), E.NH_SHAPE_BOX, ignore_body=0)
    assert b.shape == (len(LIVE),) and (b["size"] == 0.5).all() and (b["ignore_body"] == 0).all() and b["center"].tobytes() == LIVE.astype(np.float32).tobytes()


def test_box_planes_keep_what_is_inside():
    planes = rates.box_planes(LO, HI)
    assert planes.dtype == np.float32 and planes.shape == (1, 6, 4) and unit(planes[..., :3])
    for p, keep in ((0.5 * (LO + HI), True), (LO, True), (HI + 0.1, False), (LO - np.array([0.0, 0.1, 0.0]), False)):
        assert bool((planes[0, :, :3] @ p + planes[0, :, 3] >= 0).all()) is keep
    assert rates.box_planes(np.stack([LO, LO - 1]), np.stack([HI, HI + 1])).shape == (2, 6, 4)


def test_move_batch():
    o, d = rates.move_batch(np.random.default_rng(1), N, LIVE)
    o2, d2 = rates.move_batch(np.random.default_rng(1), N, LIVE)
    assert o.tobytes() == o2.tobytes() and d.tobytes() == d2.tobytes() and o.shape == d.shape == (N, 3) and o.dtype == d.dtype == np.float64
    rel = o[:, None, :] - LIVE[None]
    assert ((np.abs(rel[..., 0]) <= 0.5) & (np.abs(rel[..., 2]) <= 0.5) & (rel[..., 1] >= 2.2) & (rel[..., 1] <= 3.0)).any(axis=1).all()
    length = np.linalg.norm(d, axis=1)
    assert (length >= 0.75 - 1e-9).all() and (length <= 3.0 + 1e-9).all() and (d[:, 1] < 0).all()          # they lean downwards


def test_walk_batch_stands_on_the_slab_or_on_a_body(small):
    scene, rec = small
    tops = WB._tops(rec, len(scene["box_tags"]))
    x, top, z, d = rates.walk_batch(np.random.default_rng(2), N, rec, tops)
    again = rates.walk_batch(np.random.default_rng(2), N, rec, tops)
    assert all(u.tobytes() == v.tobytes() for u, v in zip((x, top, z, d), again))
    assert x.shape == top.shape == z.shape == (N,) and d.shape == (N, 3)
    slab_top = float(np.median(tops[rec["body"] == 0]))
    on_slab = top == slab_top
    assert 0 < on_slab.sum() < N and np.isin(top[~on_slab], tops[rec["body"] != 0]).all()
    length = np.linalg.norm(d, axis=1)
    assert (d[:, 1] == 0).all() and (length >= 0.5 - 1e-9).all() and (length <= 2.0 + 1e-9).all()


def test_reach_bounds_and_tile_size(small):
    scene, rec = small
    lo, hi = rates.reach_bounds(rec)
    assert (lo <= (rec["p"] - rec["h"]).min(axis=0) - 1.0 + 1e-6).all() and (hi >= (rec["p"] + rec["h"]).max(axis=0) + 1.0 - 1e-6).all()
    pos = scene["body_transforms"]["position"]
    tile0 = pos[np.asarray(scene["tile_of_body"]) == 0].astype(np.float64)
    assert rates.tile_size(scene, pos) == float(max(np.ptp(tile0[:, 0]), np.ptp(tile0[:, 2]))) > 0


def test_landed_derives_from_the_scene_without_a_world(small):
    scene, _ = small
    a = rates.parser("some_rates").parse_args(["--tiles", "2", "--side", "12"])
    land = rates.scene_of(a)
    assert land.world is None and (land.slabs, land.bodies - 1, land.colliders, land.steps, land.name) == (2, 288, 290, 70, "2-tile side-12")
    assert len(land.scene["box_tags"]) == 290 and len(land.scene["sphere_tags"]) == 0
    for k in ("box_transforms", "box_data", "body_transforms"):
        assert land.scene[k].tobytes() == scene[k].tobytes()
    # the slabs are body 0's boxes, the first two; their bounds straight from the scene arrays
    assert (scene["box_transforms"]["body"][:2] == 0).all() and (scene["box_transforms"]["body"][2:] != 0).all()
    p, h = scene["box_transforms"]["position"][:2].astype(np.float64), scene["box_data"]["size"][:2].astype(np.float64)
    assert np.array_equal(land.lo, (p - h).min(axis=0)) and np.array_equal(land.hi, (p + h).max(axis=0)) and (land.lo < land.hi).all()
