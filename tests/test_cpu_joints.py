"""Joints without a GPU (include/nudge_hip.h, "joints"): the serial oracle of tests/hostoracle/hostjoint.cpp -- the per-item functions of
nudge_amd/csrc/nh_joint.h that the device's lanes run, in the caller's list order -- against closed forms in which every fp32 operation is exact, its
schedule against an independent numpy implementation of the level rule on every crafted list (tests/joint_batches.py), and its drift against a float64
model of the same algorithm on a pendulum and a damped rope."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostjoint_util as HJ                  # noqa: E402
import joint_batches as B                    # noqa: E402
from nudge_amd import engine as E           # noqa: E402


def exact_bodies(positions, mass_inverse=0.5, inertia_inverse=2.0):
    """Body 0 and one body per position: identity rotations, power-of-two inverse mass and inertia."""
    scene = HJ.world(positions)
    bd = HJ.bodies_of(scene)
    bd["properties"]["mass_inverse"][1:] = mass_inverse
    bd["properties"]["inertia_inverse"][1:] = inertia_inverse
    bd["momentum"]["unused0"], bd["momentum"]["unused1"] = 7.0, -9.0          # (must keep their bits)
    return bd


def solve(bd, jnt, sweeps=1, impulses=None, **kw):
    host = HJ.Host(jnt)
    if impulses is not None:
        host.impulses["row"][:] = impulses
    active = np.arange(1, len(bd["transforms"]), dtype=np.uint32)
    host.setup(bd, active, **kw)
    host.apply(bd, sweeps)
    return host


# ---- closed forms: the analytic answer is the expected bit pattern ---------------------------------------------------------------------------------------
def test_ball_between_two_equal_bodies_leaves_both_at_the_mean():
    bd = exact_bodies([(0, 4, 0), (0, 4, 0)])
    bd["momentum"]["velocity"][1], bd["momentum"]["velocity"][2] = (1, 0.5, -2), (3, -1.5, 0.25)
    bd["momentum"]["angular_velocity"][1] = (0.5, 0.25, -1)
    before = bd["momentum"].copy()
    host = solve(bd, HJ.ball(1, 2), baumgarte=0.0)
    mean = np.array([2, -0.5, -0.875], dtype=np.float32)
    assert bd["momentum"]["velocity"][1].tobytes() == mean.tobytes() == bd["momentum"]["velocity"][2].tobytes()
    assert np.array_equal(bd["momentum"]["velocity"][1] + bd["momentum"]["velocity"][2], before["velocity"][1] + before["velocity"][2])
    assert np.array_equal(bd["momentum"]["angular_velocity"], before["angular_velocity"])          # no arm, no torque
    assert bd["momentum"]["unused0"].tobytes() == before["unused0"].tobytes() and bd["momentum"]["unused1"].tobytes() == before["unused1"].tobytes()
    assert bd["momentum"][0].tobytes() == before[0].tobytes()
    assert np.array_equal(host.impulses["row"][0], np.array([-2, 2, -2.25, 0, 0, 0], dtype=np.float32))          # lambda = -(v_b - v_a) / (mi_a + mi_b)


def test_pendulum_moving_across_its_rod_gets_no_impulse():
    bd = exact_bodies([(0, 8, 0)])
    bd["momentum"]["velocity"][1] = (3, 0, 0)
    before = bd["momentum"].copy()
    host = solve(bd, HJ.distance(0, 1, 2.0, 2.0, anchor_a=(0, 10, 0)))
    assert bd["momentum"].tobytes() == before.tobytes()
    assert not host.impulses["row"].any()


def test_slack_rope_is_a_dead_row_and_forgets_its_impulse():
    bd = exact_bodies([(0, 8, 0)])
    bd["momentum"]["velocity"][1] = (3, -5, 1)
    before = bd["momentum"].copy()
    host = solve(bd, HJ.distance(0, 1, 0.0, 5.0, anchor_a=(0, 10, 0)), impulses=(3.0, 0, 0, 0, 0, 0), warm=1.0)
    assert bd["momentum"].tobytes() == before.tobytes()
    assert host.impulses.tobytes() == bytes(32)          # +0, every bit


def test_taut_rope_closing_faster_than_the_bias_is_held_at_zero_by_the_clamp():
    jnt = HJ.distance(0, 1, 0.0, 1.0, anchor_a=(0, 10, 0))          # length 2, one too long: C = 1, bias = (0.25 / 0.125) * 1 = 2
    bd = exact_bodies([(0, 8, 0)])
    bd["momentum"]["velocity"][1] = (0, 4, 0)                        # n = (0, -1, 0): jv = -4, jv + bias < 0, lambda > 0, clamped to 0
    before = bd["momentum"].copy()
    host = solve(bd, jnt, baumgarte=0.25, time_step=0.125)
    assert bd["momentum"].tobytes() == before.tobytes() and host.impulses.tobytes() == bytes(32)
    bd["momentum"]["velocity"][1] = (0, 1, 0)                        # closing too slowly: jv + bias = 1, m = 2, lambda = -2, v_b += n * (-2 * 0.5)
    host = solve(bd, jnt, baumgarte=0.25, time_step=0.125)
    assert bd["momentum"]["velocity"][1].tobytes() == np.array([0, 2, 0], dtype=np.float32).tobytes()
    assert host.impulses["row"][0, 0] == -2.0


def test_hinge_with_aligned_axes_keeps_the_spin_about_its_axis():
    jnt = HJ.hinge(0, 1, anchor_a=(0, 4, 0), axis_a=(0, 0, 1), axis_b=(0, 0, 1))
    bd = exact_bodies([(0, 4, 0)])
    bd["momentum"]["angular_velocity"][1] = (0, 0, 8)
    before = bd["momentum"].copy()
    host = solve(bd, jnt)
    assert bd["momentum"].tobytes() == before.tobytes() and not host.impulses["row"].any()
    bd["momentum"]["angular_velocity"][1] = (2, 0, 8)                # the part across the axis goes: t2 = (-1, 0, 0), k = 2, lambda = 1
    host = solve(bd, jnt)
    assert np.array_equal(bd["momentum"]["angular_velocity"][1], np.array([0, 0, 8], dtype=np.float32))
    assert np.array_equal(bd["momentum"]["velocity"][1], np.zeros(3, dtype=np.float32))


def test_a_joint_whose_bodies_are_not_active_writes_nothing():
    bd = exact_bodies([(0, 4, 0), (0, 4, 0), (0, 4, 0)])
    bd["momentum"]["velocity"][1:] = ((1, 0, 0), (3, 0, 0), (5, 0, 0))
    before = bd["momentum"].copy()
    host = HJ.Host(np.concatenate([HJ.ball(1, 2), HJ.ball(0, 3)]))
    host.impulses["row"][:] = 0.5
    host.setup(bd, np.array([3], dtype=np.uint32), baumgarte=0.0)
    host.apply(bd, 1)
    assert bd["momentum"][1:3].tobytes() == before[1:3].tobytes() and np.all(host.impulses["row"][0] == 0.5)
    assert np.array_equal(bd["momentum"]["velocity"][3], np.zeros(3, dtype=np.float32))


# ---- the schedule: hj_prepare against numpy written from the header's text ---------------------------------------------------------------------------------
CASES = B.schedule_cases()
EXPECT = {
    "chain in order": (0, 12, 12, 1), "chain even then odd": (0, 12, 2, 1), "star": (0, 9, 9, 1), "body 0 only": (0, 14, 1, 1), "invalid kinds": (0, 2, 2, 1),
    "empty": (0, 0, 0, 0), "1025 without offsets": (E.NH_JOINT_ERR_ASSEMBLY_SIZE, 1025, 0, 0), "1025 in one assembly": (E.NH_JOINT_ERR_ASSEMBLY_SIZE, 1030, 0, 0),
    "two bins": (0, 512, 256, 2), "shared across two bins": (E.NH_JOINT_ERR_SHARED_BODY, 512, 0, 0), "offsets descend": (E.NH_JOINT_ERR_OFFSETS, 20, 0, 0),
    "offsets start late": (E.NH_JOINT_ERR_OFFSETS, 20, 0, 0), "offsets end early": (E.NH_JOINT_ERR_OFFSETS, 20, 0, 0),
    "offsets end late": (E.NH_JOINT_ERR_OFFSETS, 20, 0, 0), "no assembly": (E.NH_JOINT_ERR_OFFSETS, 20, 0, 0),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_schedule_oracle_is_the_level_rule(name):
    jnt, offsets, body_count = CASES[name]
    status, levels, order = HJ.prepare(jnt, body_count, offsets)
    nstatus, nlevels, norder = HJ.np_prepare(jnt, body_count, offsets)
    assert status.tolist() == nstatus.tolist(), name
    assert np.array_equal(levels, nlevels) and np.array_equal(order, norder)
    if name in EXPECT:
        assert tuple(status.tolist()) == EXPECT[name]
    if status[0] == 0 and len(jnt):
        # joints of one level share no dynamic body, and the order is a permutation inside every span
        assert sorted(order.tolist()) == list(range(len(jnt)))
        off = np.array([0, len(jnt)]) if offsets is None else offsets.astype(np.int64)
        bins = np.repeat(off[:-1] // E.NH_JOINT_BIN, np.diff(off))
        for w in np.unique(bins):
            for lv in range(1, int(levels[bins == w].max()) + 1):
                names = np.concatenate([jnt["a"][(bins == w) & (levels == lv)], jnt["b"][(bins == w) & (levels == lv)]])
                names = names[names != 0]
                assert len(names) == len(set(names.tolist())), (name, w, lv)


def test_windows_case_straddles_the_bins_and_the_shared_body_inside_a_bin_is_no_error():
    jnt, offsets, body_count = CASES["windows"]
    status, levels, _ = HJ.prepare(jnt, body_count, offsets)
    assert status[0] == 0 and status[3] == 7          # spans start at 0, 256, 512, 769 (bin 3), 1793 (bin 7, three assemblies), 2496, 3096
    assert np.diff(offsets).max() == E.NH_JOINT_ASSEMBLY_MAX
    jnt, offsets, body_count = CASES["shared inside one bin"]
    status, levels, _ = HJ.prepare(jnt, body_count, offsets)
    assert status[0] == 0 and levels[3] == 4 and levels[15] == 5 and levels[16] == 6          # body 4's last earlier joint is link (4, 5) of the first assembly


def test_connections_are_the_valid_pairs():
    jnt = B.invalid_kinds(5)
    con = HJ.connections(jnt, 5)
    assert con[[0, 11]].tolist() == [[1, 2], [1, 4]] and not con[1:11].any()


# ---- drift: the fp32 oracle beside a float64 model of the same algorithm -------------------------------------------------------------------------------------
def _drift(scene, jnt, steps=600, sweeps=8):
    bd = HJ.bodies_of(scene)
    model = HJ.Model(bd, jnt, scene["params"])
    host = HJ.Host(jnt)
    worst = [0.0, 0.0]

    def look(_):
        model.step(sweeps)
        worst[0] = max(worst[0], HJ.anchor_errors(bd["transforms"], jnt).max())
        worst[1] = max(worst[1], HJ.anchor_errors(model.transforms(), jnt).max())

    HJ.host_steps(bd, host, steps, sweeps, scene["params"], on_step=look)
    assert np.isfinite(bd["transforms"]["position"]).all()
    return worst


def test_pendulum_and_rope_drift_like_the_float64_model():
    """600 sub-steps of gravity, setup, 8 sweeps and advance.  The fp32 oracle's worst anchor error stays within twice the float64 model's own: the error is
    the algorithm's (Baumgarte, a finite number of sweeps), far above fp32 resolution.  Figures: DESIGN.md 10.28."""
    pend_scene = HJ.world([(2, 10, 0)], spheres=True)
    pend = HJ.distance(0, 1, 2.0, 2.0, anchor_a=(0, 10, 0))
    n = 8
    rope_scene = HJ.world([(0.25 + 0.5 * k, 10, 0) for k in range(n)], half=0.2, spheres=True)
    rope = np.concatenate([HJ.ball(k, k + 1, anchor_a=(0, 10, 0) if k == 0 else (0.25, 0, 0), anchor_b=(-0.25, 0, 0)) for k in range(n)])
    for name, scene, jnt in (("pendulum", pend_scene, pend), ("rope", rope_scene, rope)):
        f32, f64 = _drift(scene, jnt)
        print(f"{name}: worst anchor error fp32 oracle {f32:.6e}, float64 model {f64:.6e}, ratio {f32 / f64:.4f}")
        assert f64 > 1e-5          # far above fp32 resolution at these magnitudes
        assert f32 <= 2.0 * f64
