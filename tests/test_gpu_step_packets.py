"""What travels in the stream around a still step's solver (pytest -m gpu): the timer's events and the ring event.

A still step that reports itself has no event behind its solver: the host spins on the number the solver's first thread leaves in pinned memory (nh_still_await_number,
nudge_amd/csrc/nh_step.hip); under option no_early_counts the ring event is recorded and waited for as before; a timed launch has the timer's two events around it
(NH_LAUNCH, nudge_amd/csrc/nh_internal.h).  None of it may show in the results: the same call sequence on a small landed world under the four ways a step can be watched --
not at all, with the ring event, with the timing filter on the still solver, with every launch timed -- gives the same bits; the steps that fail are the ones the parent
library failed; and what the timer reports is one positive time per launch that fits into the wall time of the calls."""
import os
import sys
import time

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_pair_begin import CALLS, LANDED, _arrange, _same, _scene, _world          # noqa: E402  (the world of that file: a hovering box, two close neighbours)

pytestmark = pytest.mark.gpu

SEQUENCE = CALLS + CALLS

# (still steps, steps that started at the solver, still steps that did not happen) over SEQUENCE, as the PARENT library (commit 07f0502, loaded through NUDGE_HIP_LIBRARY)
# reports them for each setting on this world -- profiles/r10_steady_step_ab.log, "tests".
PARENT_COUNTS = {
    "default": (98, 92, 1),
    "no_early_counts": (98, 92, 1),
    "filter": (98, 92, 1),
    "full": (98, 92, 1),
}
# launches per timer name over SEQUENCE with every launch timed, parent library
PARENT_FULL_LAUNCHES = {
    "active_flags": 1, "active_write": 2, "adjacency_simple": 2, "advance_rest": 1, "ahead_check": 6, "ahead_map": 6, "bucket_count": 2, "bucket_scan": 2, "bucket_scatter":
    2, "bucket_sort": 2, "cache_to_slots": 2, "cell_keys": 2, "cell_scan": 4, "cell_scatter": 2, "coarse_flatten": 1, "collide_begin": 2, "filter_records": 1, "find_pairs":
    2, "gather_contacts": 7, "gravity_rest": 1, "grid_setup": 2, "kept_filter": 2, "large_pairs": 2, "narrowphase": 2, "narrowphase_still": 7, "pair_begin": 92, "pair_list":
    2, "pair_mark": 2, "reinsert": 2, "scan_final": 10, "scan_sums": 10, "slot_counts": 7, "slots_to_cache": 7, "solve_one_body": 2, "solve_still": 99, "sorted_counts": 2,
    "uf_flatten": 1, "uf_union_records": 1, "write_cache": 2, "xform_aabb": 2, "xform_still": 7,
}
# still steps that did not happen in the landing sequence of test (iii), parent library (the figure tests/test_gpu_pair_begin.py holds its test (ii) to)
PARENT_LANDING_REPLAYS = 4


def _delta(c1, c0):
    return (c1["still_steps"] - c0["still_steps"], c1["pair_steps"] - c0["pair_steps"], c1["still_replays"] - c0["still_replays"])


def test_four_ways_of_watching_a_step_do_not_show():
    """(i) Default, ring event, timing filter, full timing: bodies, contacts, cache and counters identical after every call; still, pair and failed steps as on the parent;
    under the filter one time per solver launched, their sum positive and within the wall time of the call, each of eight single launches positive; under full timing the parent's names and launch counts."""
    scene = _scene()
    names = ("default", "no_early_counts", "filter", "full")
    w = {k: _world(scene) for k in names}
    w["no_early_counts"].set_option("no_early_counts", 1)
    for k in names:
        w[k].step(LANDED)
    _arrange(tuple(w.values()))
    for k in names:
        w[k].synchronize()
    w["filter"].enable_timing(True, only="solve_still")
    w["full"].enable_timing(True)
    c0 = {k: w[k].counts() for k in names}
    done = 0
    full = {}
    for n in SEQUENCE:
        before = w["filter"].counts()
        for k in names:
            t0 = time.perf_counter()
            w[k].step(n)
            if k == "filter":
                kt = w[k].kernel_times()          # (synchronises the stream and collects)
                wall_ms = (time.perf_counter() - t0) * 1e3
                after = w[k].counts()
                launched = sum(_delta(after, before)[i] for i in (0, 2))          # (still steps that happened + those that did not: one solver each)
                ms, launches = kt.get("solve_still", (0.0, 0))
                print(f"\n[packets] call of {n}: solve_still {launches} launches {ms:.4f} ms, {launched} still solvers launched, wall {wall_ms:.3f} ms")
                assert set(kt) <= {"solve_still"}, kt
                assert launches == launched, (n, kt, before, after)
                if launches:
                    assert ms > 0.0 and ms <= wall_ms, (n, ms, wall_ms)
                    assert ms / launches < 1.0, (n, ms, launches)          # (a launch on a world of 289 bodies, five waves: tens of microseconds)
            elif k == "full":
                for name, (ms, launches) in w[k].kernel_times().items():
                    assert launches > 0 and ms > 0.0, (name, ms, launches)
                    full[name] = full.get(name, 0) + launches
        done += n
        for k in names[1:]:
            _same(w["default"], w[k], f"call of {n}, step {done} (default vs {k})")
    got = {k: _delta(w[k].counts(), c0[k]) for k in names}
    print(f"\n[packets] (still, pair, failed) steps in {done}: {got}")
    # every single time, not only their sums: calls of one sub-step, collected one by one (the world is at rest by now: each is one still solver)
    singles = []
    for _ in range(8):
        for k in names:
            w[k].step(1)
        ms, launches = w["filter"].kernel_times().get("solve_still", (0.0, 0))
        assert launches == 1 and 0.0 < ms < 1.0, (ms, launches)
        singles.append(ms)
        w["full"].kernel_times()
    for k in names[1:]:
        _same(w["default"], w[k], f"eight calls of 1 (default vs {k})")
    print(f"[packets] eight single launches, ms: {[round(x, 4) for x in singles]}")
    print(f"[packets] full timing, launches by name: {dict(sorted(full.items()))}")
    for k in names:
        assert w[k].counts()["error"] == 0
    assert got == PARENT_COUNTS, (got, PARENT_COUNTS)
    assert got["default"][1] > 0 and got["default"][2] >= 1          # (steps did start at the solver, and a verdict read by spin did fail one)
    assert dict(sorted(full.items())) == PARENT_FULL_LAUNCHES, (full, PARENT_FULL_LAUNCHES)
    for k in names:
        w[k].close()


def test_a_landing_inside_a_call_read_by_spin():
    """(ii) Two boxes come down inside a 20-step call whose verdicts the host takes by spin, one step late: after every call the bits of the library that never speculates
    -- the landing is seen in the step in which it happens -- and as many steps failed as on the parent."""
    scene = _scene()
    a, c = _world(scene), _world(scene, env=["NH_NO_STILL"])
    for x in (a, c):
        x.step(LANDED)
    _arrange((a, c), drop=0.05)
    c0 = a.counts()
    done = 0
    for n in (3, 20, 10):
        a.step(n); c.step(n)
        done += n
        _same(a, c, f"call of {n}, step {done}")
    c1 = a.counts()
    replays = c1["still_replays"] - c0["still_replays"]
    print(f"\n[packets, landing] replays {replays}; pair {c1['pair_steps'] - c0['pair_steps']} of {c1['still_steps'] - c0['still_steps']} still steps in {done}")
    assert c1["error"] == 0 and c1["pair_steps"] > c0["pair_steps"] and c.counts()["still_steps"] == 0, (c0, c1)
    assert replays == PARENT_LANDING_REPLAYS, (replays, PARENT_LANDING_REPLAYS)
    a.close(); c.close()
