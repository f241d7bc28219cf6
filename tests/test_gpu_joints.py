"""Joints on the GPU (pytest -m gpu): nh_joints_prepare, nh_joints_setup, nh_joints_apply and nh_joint_connections (include/nudge_hip.h, "joints").

The oracle is tests/hostoracle/hostjoint.cpp through tests/hostjoint_util.py: nudge_amd/csrc/nh_joint.h's own arithmetic in the plain serial loop "for each
joint in list order, for each row in row order", which is the specification -- so the device's level-parallel replay must give its bytes: levels, order
and status of every crafted list (tests/joint_batches.py), every byte of momentum (the unused words included) and of the accumulated impulses after
setup and sweeps, and the body state of a jointed world after 240 sub-steps.  Where contacts and joints meet no oracle exists: those worlds are held to
themselves (two runs, the same bytes) and to the sets that sleep and wake."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostjoint_util as HJ                  # noqa: E402
import joint_batches as B                    # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 16
NH_ERR_INVALID, NH_ERR_STALE_SETUP = 1, 10
CASES = B.schedule_cases()


def _dev(w, a, dtype=None, guard=0):
    """A device copy of a numpy array as uint8, `guard` sentinel bytes behind it (at least 16 bytes in all)."""
    import torch
    raw = np.ascontiguousarray(a, dtype=dtype).view(np.uint8).reshape(-1)
    t = torch.full((max(raw.size + guard, 16),), SENTINEL, dtype=torch.uint8, device=w.dev)
    if raw.size:
        t[:raw.size] = torch.from_numpy(raw.copy()).to(w.dev)
    return t


def _back(t, dtype, n):
    return np.frombuffer(t.cpu().numpy().tobytes()[:np.dtype(dtype).itemsize * n], dtype=dtype).copy()


class Raw:
    """One list on the device through the C ABI itself: sentinel-filled plan arrays with guards behind them."""

    def __init__(self, w, jnt, offsets=None, capacity=None):
        self.w, self.n = w, len(jnt)
        self.cap = self.n if capacity is None else capacity
        self.joints = _dev(w, jnt, E.JOINT)
        self.offsets = None if offsets is None else _dev(w, offsets, np.uint32)
        self.status, self.levels, self.order = (_dev(w, np.zeros(0, np.uint32), guard=4 * (k + GUARD)) for k in (4, self.cap, self.cap))
        self.impulses = _dev(w, np.zeros(self.n, E.JOINT_IMPULSE), guard=32)
        self.list = E.JointList(self.joints.data_ptr(), self.offsets.data_ptr() if offsets is not None else 0, self.n, 0 if offsets is None else len(offsets) - 1)
        self.plan = E.JointPlan(self.status.data_ptr(), self.levels.data_ptr(), self.order.data_ptr(), self.cap, 0)

    def prepare(self, body_count):
        return self.w.L.nh_joints_prepare(self.w.ctx, body_count, C.byref(self.list), C.byref(self.plan))

    def setup(self, prm=None, impulses=True):
        prm = HJ.params() if prm is None else prm
        w = self.w
        return w.L.nh_joints_setup(w.ctx, C.byref(w.active), C.byref(w.bodies), C.byref(self.list), C.byref(self.plan), C.byref(prm),
                                   C.c_void_p(self.impulses.data_ptr() if impulses else 0))

    def apply(self, iterations=1):
        w = self.w
        return w.L.nh_joints_apply(w.ctx, C.byref(w.bodies), C.byref(self.list), C.byref(self.plan), C.c_void_p(self.impulses.data_ptr()), iterations)

    def plan_back(self):
        """(status, levels, order) with the guards checked; the words the call did not write are still the sentinel."""
        out = []
        for t, k in ((self.status, 4), (self.levels, self.cap), (self.order, self.cap)):
            a = _back(t, np.uint32, k + GUARD)
            assert set(a[k:].tobytes()) == {SENTINEL}, "words behind a plan array were written"
            out.append(a[:k])
        return out


@pytest.fixture(scope="module")
def small():
    w = E.World(HJ.world(B._scatter(8, 1)))
    yield w
    w.close()


# ---- the schedule ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_prepare_equals_the_oracle(small, name):
    jnt, offsets, body_count = CASES[name]
    r = Raw(small, jnt, offsets)
    assert r.prepare(body_count) == 0
    status, levels, order = r.plan_back()
    hs, hl, ho = HJ.prepare(jnt, body_count, offsets)
    assert status.tolist() == hs.tolist(), name
    assert levels.tobytes() == hl.tobytes() and order.tobytes() == ho.tobytes(), name
    # twice: the bits are a function of the input alone
    assert r.prepare(body_count) == 0
    again = r.plan_back()
    assert again[0].tolist() == hs.tolist() and again[1].tobytes() == hl.tobytes() and again[2].tobytes() == ho.tobytes()


def test_connections_equal_the_oracle(small):
    import torch
    jnt = B.invalid_kinds(5)
    r = Raw(small, jnt)
    assert r.prepare(5) == 0
    out = torch.full((8 * len(jnt) + 64,), SENTINEL, dtype=torch.uint8, device=small.dev)
    assert small.L.nh_joint_connections(small.ctx, C.byref(r.list), C.c_void_p(out.data_ptr())) == 0
    got = _back(out, np.uint32, 2 * len(jnt) + 16)
    assert got[:2 * len(jnt)].reshape(-1, 2).tolist() == HJ.connections(jnt, 5).tolist()
    assert set(got[2 * len(jnt):].tobytes()) == {SENTINEL}


# ---- setup and sweeps against the serial loop ----------------------------------------------------------------------------------------------------------------
def _host_state(w, scene):
    b = w.get_bodies()
    return dict(transforms=b["transforms"], properties=scene["body_properties"].copy(), momentum=b["momentum"], idle=b["idle"])


def _same_bytes(got, ref, what):
    size = got.dtype.itemsize
    bad = (np.ascontiguousarray(got).view(np.uint8).reshape(-1, size) != np.ascontiguousarray(ref).view(np.uint8).reshape(-1, size)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(got)} records differ, first at {int(np.argmax(bad))}: {got[np.argmax(bad)]} != {ref[np.argmax(bad)]}"


def _impulses(w):
    return _back(w.joint_impulses, E.JOINT_IMPULSE, w._joints["n"])


def _compare(scene, jnt, offsets, calls=(("setup", dict(warm=1.0)), ("apply", 1)), asleep=None, levels=None, unused=True):
    """The device and the serial loop through the same sequence of calls from the same state: momentum and impulses byte for byte after every call."""
    scene = dict(scene)
    if unused:
        scene["body_momentum"] = scene["body_momentum"].copy()
        scene["body_momentum"]["unused0"] = np.arange(len(scene["body_momentum"]), dtype=np.float32) + 0.5          # (must keep their bits)
        scene["body_momentum"]["unused1"] = -scene["body_momentum"]["unused0"]
    w = E.World(scene)
    try:
        w.joints_prepare(jnt, offsets, connect=asleep is not None)
        status = w.joint_status()
        assert status[0] == 0 and status[1] == int(HJ.np_valid(jnt, len(scene["body_transforms"])).sum())
        if levels is not None:
            assert status[2] == levels
        if asleep is not None:
            idle = scene["idle_counters"].copy()
            idle[asleep] = 0xff
            w.set_bodies(idle=idle)
        w.collide()
        active = w.get_active()
        if asleep is not None:
            assert sorted(active.tolist()) == sorted(set(range(1, len(idle))) - set(np.asarray(asleep).tolist()))
        bd = _host_state(w, scene)
        host = HJ.Host(jnt)
        rng = np.random.default_rng(5)
        start = rng.uniform(-0.2, 0.2, (len(jnt), 6)).astype(np.float32)          # accumulated impulses of an earlier step
        host.impulses["row"] = start
        w.joint_impulses[:32 * len(jnt)] = _dev(w, host.impulses, E.JOINT_IMPULSE)[:32 * len(jnt)]
        for k, (call, arg) in enumerate(calls):
            if call == "setup":
                w.joints_setup(**arg)
                host.setup(bd, active, time_step=scene["params"]["time_step"], **arg)
            else:
                w.joints_apply(arg)
                host.apply(bd, arg)
            what = f"after call {k} ({call} {arg})"
            _same_bytes(w.get_bodies()["momentum"], bd["momentum"], what + ", momentum")
            _same_bytes(_impulses(w), host.impulses[:len(jnt)], what + ", impulses")
        return w.get_bodies()["momentum"], _impulses(w), scene, start
    finally:
        w.close()


def test_each_type_against_body_0_and_between_two_bodies():
    scene, jnt, offsets = B.each_type_world()
    mom, imp, scene, _ = _compare(scene, jnt, offsets, calls=(("setup", dict(warm=1.0)), ("apply", 1), ("apply", 3)))
    assert (mom["velocity"][1:] != scene["body_momentum"]["velocity"][1:]).any(axis=1).sum() >= 10          # every body is jointed (a slack rope moves nobody)
    assert mom[0].tobytes() == scene["body_momentum"][0].tobytes()


def test_300_copies_of_a_mixed_assembly():
    scene, jnt, offsets = B.copies_world()
    assert len(jnt) == 4500 and E.NH_JOINT_BIN % 15 != 0          # spans merge assemblies, and cut points fall inside the 256-windows
    _compare(scene, jnt, offsets, calls=(("setup", dict(warm=1.0)), ("apply", 1), ("apply", 4)))


@pytest.mark.parametrize("split", (False, True))
def test_rope_of_1024_joints(split):
    scene, jnt, offsets = B.rope_world(1024, split=split)
    _compare(scene, jnt, offsets, calls=(("setup", dict(warm=1.0)), ("apply", 1), ("apply", 2)), levels=2 if split else 1024)


def test_partial_active_list_leaves_the_absent_assemblies_alone():
    scene, jnt, offsets = B.copies_world(copies=40)
    asleep = np.concatenate([np.arange(1 + 8 * c, 9 + 8 * c) for c in range(0, 40, 3)])
    mom, imp, scene, start = _compare(scene, jnt, offsets, asleep=asleep)
    gone = np.isin(jnt["a"], asleep) | np.isin(jnt["b"], asleep)
    assert gone.sum() == 15 * 14
    assert mom[asleep].tobytes() == scene["body_momentum"][asleep].tobytes()
    assert imp["row"][gone].tobytes() == start[gone].tobytes() and (imp["row"][~gone] != start[~gone]).any(axis=1).all()


def test_four_times_one_sweep_is_four_sweeps():
    scene, jnt, offsets = B.copies_world(copies=20)
    a = _compare(scene, jnt, offsets, calls=(("setup", dict(warm=1.0)), ("apply", 4)))
    b = _compare(scene, jnt, offsets, calls=(("setup", dict(warm=1.0)),) + (("apply", 1),) * 4)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("warm", (0.0, 1.0))
def test_warm_start_across_two_setups(warm):
    scene, jnt, offsets = B.copies_world(copies=20)
    _compare(scene, jnt, offsets, calls=(("setup", dict(warm=warm)), ("apply", 2), ("setup", dict(warm=warm)), ("apply", 1)))


# ---- whole steps ------------------------------------------------------------------------------------------------------------------------------------------
def test_hanging_world_equals_the_host_loop_after_240_sub_steps():
    scene, jnt, offsets = B.hanging_world()
    w = E.World(scene)
    try:
        w.joints_prepare(jnt, offsets)
        w.step_joints(240, iterations=4)
        assert w.counts()["contacts"] == 0
        got = w.get_bodies()
        imp = _impulses(w)
    finally:
        w.close()
    bd = HJ.bodies_of(scene)
    host = HJ.Host(jnt)
    HJ.host_steps(bd, host, 240, 4, scene["params"])
    _same_bytes(got["transforms"], bd["transforms"], "transforms")
    _same_bytes(got["momentum"], bd["momentum"], "momentum")
    assert got["idle"].tobytes() == bd["idle"].tobytes()
    _same_bytes(imp, host.impulses[:len(jnt)], "impulses")
    moved = np.linalg.norm(got["transforms"]["position"][1:] - scene["body_transforms"]["position"][1:], axis=1)
    err = HJ.anchor_errors(got["transforms"], jnt)
    print(f"hanging world: bodies moved {moved.min():.3f} .. {moved.max():.3f}, worst anchor error {err.max():.3e}")
    assert moved.min() > 0.05 and err.max() < 0.1          # they swung, and they hang where they were hung


def _chains(steps, look=None):
    scene, jnt, offsets = B.chains_world()
    w = E.World(scene)
    try:
        w.joints_prepare(jnt, offsets)
        assert w.joint_status()[0] == 0
        w.step_joints(steps, iterations=8)
        if look:
            look(w, scene, jnt)
        return w.get_bodies(), _impulses(w), scene, jnt
    finally:
        w.close()


def test_crates_on_chains_run_twice_to_the_same_bytes():
    a, ia, scene, jnt = _chains(60)
    b, ib, _, _ = _chains(60)
    for k in ("transforms", "momentum", "idle"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert ia.tobytes() == ib.tobytes()
    assert np.isfinite(a["transforms"]["position"]).all()
    err = HJ.anchor_errors(a["transforms"], jnt)
    speed = np.linalg.norm(a["momentum"]["velocity"][1:], axis=1)
    print(f"crates on chains after 60 sub-steps: worst anchor error {err.max():.3e}, mean {err.mean():.3e}; speeds up to {speed.max():.3e}")


def test_assemblies_sleep_and_wake_as_one_set():
    def look(w, scene, jnt):
        nb = len(scene["body_transforms"])
        per = 6
        crates = (nb - 1) // per
        sets = [sorted({int(x) for x in np.concatenate([jnt["a"][c * per:(c + 1) * per], jnt["b"][c * per:(c + 1) * per]])} - {0}) for c in range(crates)]
        assert all(len(s) == per for s in sets)
        speed = np.linalg.norm(w.get_bodies()["momentum"]["velocity"][1:], axis=1)
        print(f"speeds when put to sleep: up to {speed.max():.3e}")
        # everybody's counter saturated but ONE link of chain 1: that whole assembly stays awake, every other one sleeps
        idle = np.full(nb, 0xff, dtype=np.uint8)
        idle[sets[1][2]] = 0
        w.set_bodies(idle=idle)
        w.step_joints(1, iterations=8)
        assert sorted(w.get_active().tolist()) == sets[1]
        before = w.get_bodies()
        # all asleep; then one link of chain 3 is pushed awake
        w.set_bodies(idle=np.full(nb, 0xff, dtype=np.uint8))
        w.step_joints(1, iterations=8)
        assert len(w.get_active()) == 0
        w.body_impulses([sets[3][4]], [[0.0, 0.0, 1e-3]], wake=True)
        w.step_joints(1, iterations=8)
        assert sorted(w.get_active().tolist()) == sets[3]
        after = w.get_bodies()
        others = np.array(sorted(set(range(1, nb)) - set(sets[3]) - set(sets[1])))
        assert after["transforms"][others].tobytes() == before["transforms"][others].tobytes()          # the sleepers did not move

    _chains(30, look)


def test_a_world_that_only_prepares_joints_steps_like_one_that_never_heard_of_them():
    scene = S.pile(n_boxes=64)
    out = []
    for mode in ("never", "prepare", "prepare and connect"):
        w = E.World(scene)
        try:
            if mode != "never":
                w.joints_prepare(B.pairs([(1, 2), (2, 3), (0, 5), (7, 9)]), connect=mode.endswith("connect"))
            w.step(40)
            out.append(w.get_bodies())
        finally:
            w.close()
    for other in out[1:]:
        for k in ("transforms", "momentum", "idle"):
            assert out[0][k].tobytes() == other[k].tobytes(), k


# ---- the ABI's edges -----------------------------------------------------------------------------------------------------------------------------------------
def test_abi_edge_cases():
    import torch
    scene, jnt, offsets = B.copies_world(copies=4)
    nb = len(scene["body_transforms"])
    w = E.World(scene)
    try:
        L, ctx = w.L, w.ctx
        w.collide()
        mom0 = w.get_bodies()["momentum"].tobytes()

        def untouched(r):
            for t in (r.status, r.levels, r.order):
                assert set(t.cpu().numpy().tobytes()) == {SENTINEL}
            assert w.get_bodies()["momentum"].tobytes() == mom0
            assert r.impulses.cpu().numpy().tobytes()[:32 * r.n] == bytes(32 * r.n)

        r = Raw(w, jnt, offsets)
        ok_list, ok_plan, prm = r.list, r.plan, HJ.params()
        lists = dict(null_joints=E.JointList(0, ok_list.offsets, r.n, ok_list.assemblies), odd_joints=E.JointList(ok_list.joints + 8, ok_list.offsets, r.n, ok_list.assemblies),
                     odd_offsets=E.JointList(ok_list.joints, ok_list.offsets + 2, r.n, ok_list.assemblies), huge=E.JointList(ok_list.joints, ok_list.offsets, 1 << 31, ok_list.assemblies))
        plans = dict(null_status=E.JointPlan(0, ok_plan.levels, ok_plan.order, r.n, 0), null_levels=E.JointPlan(ok_plan.status, 0, ok_plan.order, r.n, 0),
                     null_order=E.JointPlan(ok_plan.status, ok_plan.levels, 0, r.n, 0), odd_status=E.JointPlan(ok_plan.status + 2, ok_plan.levels, ok_plan.order, r.n, 0),
                     odd_order=E.JointPlan(ok_plan.status, ok_plan.levels, ok_plan.order + 1, r.n, 0), small=E.JointPlan(ok_plan.status, ok_plan.levels, ok_plan.order, r.n - 1, 0))
        imp = C.c_void_p(r.impulses.data_ptr())
        for name, lst in lists.items():
            assert L.nh_joints_prepare(ctx, nb, C.byref(lst), C.byref(ok_plan)) == NH_ERR_INVALID, name
            assert L.nh_joints_setup(ctx, C.byref(w.active), C.byref(w.bodies), C.byref(lst), C.byref(ok_plan), C.byref(prm), imp) == NH_ERR_INVALID, name
            assert L.nh_joints_apply(ctx, C.byref(w.bodies), C.byref(lst), C.byref(ok_plan), imp, 1) == NH_ERR_INVALID, name
        for name, pl in plans.items():
            assert L.nh_joints_prepare(ctx, nb, C.byref(ok_list), C.byref(pl)) == NH_ERR_INVALID, name
            assert L.nh_joints_setup(ctx, C.byref(w.active), C.byref(w.bodies), C.byref(ok_list), C.byref(pl), C.byref(prm), imp) == NH_ERR_INVALID, name
            assert L.nh_joints_apply(ctx, C.byref(w.bodies), C.byref(ok_list), C.byref(pl), imp, 1) == NH_ERR_INVALID, name
        assert L.nh_joints_prepare(None, nb, C.byref(ok_list), C.byref(ok_plan)) == NH_ERR_INVALID
        assert L.nh_joints_prepare(ctx, nb, None, C.byref(ok_plan)) == NH_ERR_INVALID and L.nh_joints_prepare(ctx, nb, C.byref(ok_list), None) == NH_ERR_INVALID
        for bad in (dict(time_step=float("nan")), dict(baumgarte=float("inf")), dict(max_bias=-1.0), dict(warm=-0.5), dict(warm=1.5), dict(time_step=-1.0)):
            assert r.setup(HJ.params(**bad)) == NH_ERR_INVALID, bad
        assert r.setup(impulses=False) == NH_ERR_INVALID
        assert L.nh_joints_setup(ctx, C.byref(w.active), C.byref(w.bodies), C.byref(ok_list), C.byref(ok_plan), C.byref(prm), C.c_void_p(r.impulses.data_ptr() + 4)) == NH_ERR_INVALID
        assert L.nh_joints_setup(ctx, None, C.byref(w.bodies), C.byref(ok_list), C.byref(ok_plan), C.byref(prm), imp) == NH_ERR_INVALID
        assert L.nh_joints_setup(ctx, C.byref(w.active), None, C.byref(ok_list), C.byref(ok_plan), C.byref(prm), imp) == NH_ERR_INVALID
        assert L.nh_joints_setup(ctx, C.byref(w.active), C.byref(w.bodies), C.byref(ok_list), C.byref(ok_plan), None, imp) == NH_ERR_INVALID
        assert r.apply(0) == NH_ERR_INVALID
        assert L.nh_joint_connections(ctx, None, imp) == NH_ERR_INVALID and L.nh_joint_connections(ctx, C.byref(ok_list), None) == NH_ERR_INVALID
        assert L.nh_joint_connections(ctx, C.byref(ok_list), C.c_void_p(r.impulses.data_ptr() + 4)) == NH_ERR_INVALID
        untouched(r)
        # before any nh_joints_prepare there is no body count to judge a pair by
        assert L.nh_joint_connections(ctx, C.byref(ok_list), imp) == NH_ERR_INVALID
        # apply without setup; setup, then a prepare or a collide in between
        assert r.prepare(nb) == 0
        assert r.apply(1) == NH_ERR_STALE_SETUP
        assert w.get_bodies()["momentum"].tobytes() == mom0
        assert r.setup() == 0 and r.apply(1) == 0
        moved = w.get_bodies()["momentum"].tobytes()
        assert moved != mom0
        assert r.prepare(nb) == 0 and r.apply(1) == NH_ERR_STALE_SETUP
        assert r.setup() == 0
        w.collide()
        assert r.apply(1) == NH_ERR_STALE_SETUP
        # count == 0: pending work is completed, nothing else happens
        w.gravity(); w.read_cache(); w.setup()
        empty = Raw(w, HJ.joints(0))
        assert empty.prepare(nb) == 0 and empty.plan_back()[0].tolist() == [0, 0, 0, 0]
        mom1 = w.get_bodies()["momentum"].tobytes()
        assert empty.setup() == 0 and empty.apply(3) == 0
        assert w.get_bodies()["momentum"].tobytes() == mom1
        w.apply(1); w.update(); w.write_cache(); w.advance()
        # a plan with a status bit set leaves momentum and impulses untouched
        bad = Raw(w, jnt, np.array([0, 30, 15, 60], dtype=np.uint32))
        assert bad.prepare(nb) == 0 and bad.plan_back()[0][0] == E.NH_JOINT_ERR_OFFSETS
        w.collide()
        mom2 = w.get_bodies()["momentum"].tobytes()
        assert bad.setup() == 0 and bad.apply(2) == 0
        assert w.get_bodies()["momentum"].tobytes() == mom2
        assert bad.impulses.cpu().numpy().tobytes()[:32 * bad.n] == bytes(32 * bad.n)
        torch.cuda.synchronize()
    finally:
        w.close()
