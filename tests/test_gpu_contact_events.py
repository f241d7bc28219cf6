"""Contact events on the GPU (pytest -m gpu): nh_contact_pairs / nh_contact_events / nh_step_contact_pairs (include/nudge_hip.h, "contact events").

The oracle is tests/hostcontacts_util.py's C++ one (the per-item functions of nudge_amd/csrc/nh_contact_events.h on the host around a serial stable
sort; tests/test_cpu_contact_events.py holds it against an independent numpy implementation and asserts that the batches of tests/contact_batches.py
hold what they are for).  Counts and records must equal the oracle's byte for byte, and so must every byte behind a written prefix: a 0xA5 sentinel
there stays the sentinel."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_batches as B                  # noqa: E402
import hostcontacts_util as HC               # noqa: E402
import list_util as LU                       # noqa: E402
import query_util as Q                       # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SLACK = 2          # sentinel records kept behind every output's capacity
NH_ERR_INVALID = 1


@pytest.fixture(scope="module")
def w():
    """A context to call through; the list calls read nothing of its world."""
    world = E.World(S.pile(8, 0, seed=1), flags=Q.FUSED)
    yield world
    world.close()


def sentinel(n):
    return np.frombuffer(bytes([SENTINEL]) * 64 * n, dtype=E.CONTACT_PAIR).copy()


def dev_contacts(w, lst, count=None):
    """The device tensors of a contact list: (data, bodies, impulses or None, count word or None, capacity)."""
    import torch
    n = len(lst["data"])
    up = lambda a: Q.upload(w, a) if len(a) else torch.zeros(64, dtype=torch.uint8, device=w.dev)
    ct = None if count is None else torch.tensor([count], dtype=torch.int64, device=w.dev).to(torch.int32)
    return up(lst["data"]), up(lst["bodies"]), (None if lst["impulses"] is None else up(lst["impulses"])), ct, n


def dev_out(w, capacity):
    """An output list (count, pairs, capacity): the count word and capacity + SLACK records of the sentinel; capacity None: count only."""
    import torch
    ct = torch.full((1,), -0x5A5A5A5B, dtype=torch.int32, device=w.dev)          # 0xA5A5A5A5
    if capacity is None:
        return ct, None, 0
    return ct, torch.full((capacity + SLACK, 64), SENTINEL, dtype=torch.uint8, device=w.dev), capacity


def dev_pairs(w, lst):
    """A pair list (count, records, capacity) on the device."""
    import torch
    n, rec, cap = lst
    ct = torch.tensor([n], dtype=torch.int64, device=w.dev).to(torch.int32)
    return ct, (Q.upload(w, rec[:cap]).reshape(-1, 64) if cap else None), cap


def read(out):
    """(count, every record slot of the output, the slack included)."""
    ct, pt, _ = out
    n = int(ct.cpu().numpy().view(np.uint32)[0])
    return n, (None if pt is None else np.frombuffer(pt.cpu().numpy().tobytes(), dtype=E.CONTACT_PAIR).copy())


def same(got, want, what):
    assert got[0] == want[0], f"{what}: count {got[0]}, the oracle's {want[0]}"
    if got[1] is not None:
        a, b = got[1].view(np.uint8).reshape(-1, 64), want[1].view(np.uint8).reshape(-1, 64)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {int((a != b).any(axis=1).sum())} of {len(a)} record slots differ"


def gpu_pairs(w, lst, body_count, capacity, count=None, dev=None):
    d = dev or dev_contacts(w, lst, count)
    out = dev_out(w, capacity)
    w.contact_pairs_records(d[0], d[1], d[2], count=d[3], capacity=d[4], body_count=body_count, out=out)
    return read(out)


def check_pairs(w, lst, body_count, what, expect=None):
    """Count only, then a list of exactly the count, against the oracle on `expect` (default: the list itself).  Returns the count."""
    expect = lst if expect is None else expect
    total = HC.count_pairs(expect)
    same(gpu_pairs(w, lst, body_count, None), (total, None), f"{what}, count only")
    same(gpu_pairs(w, lst, body_count, total), HC.pairs(expect, capacity=total, out=sentinel(total + SLACK)), what)
    return total


# ---- nh_contact_pairs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", B.SIZES)
def test_lists_of_every_size(w, n):
    """count == NULL: the capacity is the count.  70,001 contacts: more than one tile per block of the 512-block sort, a scan over several blocks."""
    for mode in B.MODES:
        lst, body_count = B.sized(n, mode)
        total = check_pairs(w, lst, body_count, f"{mode} {n}")
        assert total == {"one_pair": min(n, 1), "distinct": n}.get(mode, total)


def test_every_rule_and_every_key_width(w):
    lst = B.features()
    B.check_features(lst)
    for body_count in (10, 0):
        check_pairs(w, lst, body_count, f"features, body_count {body_count}")
    cases = B.key_widths()
    B.check_key_widths(cases)
    for lst, body_count, passes in cases:
        for bc in (body_count, 0):
            check_pairs(w, lst, bc, f"{passes} key bytes, body_count {bc}")


def test_a_device_count_below_the_capacity(w):
    """The tail is NaNs and body 0xFFFFFFFF; the result is that of the truncated list.  A count above the capacity is clamped to it."""
    lst, body_count = B.sized(513, "mixed")
    for keep in (300, 1, 0):
        tail = dict(data=lst["data"].copy(), bodies=lst["bodies"].copy(), impulses=lst["impulses"].copy())
        tail["data"].view(np.float32).reshape(-1, 8)[keep:] = np.nan
        tail["impulses"].view(np.float32).reshape(-1, 4)[keep:] = np.nan
        tail["bodies"][keep:] = 0xFFFFFFFF
        short = HC.truncated(lst, keep)
        total = HC.count_pairs(short)
        d = dev_contacts(w, tail, count=keep)
        same(gpu_pairs(w, tail, body_count, total, dev=d), HC.pairs(short, capacity=total, out=sentinel(total + SLACK)), f"count {keep} of 513")
    total = HC.count_pairs(lst)
    d = dev_contacts(w, lst, count=100000)
    same(gpu_pairs(w, lst, body_count, total, dev=d), HC.pairs(lst, capacity=total, out=sentinel(total + SLACK)), "count above the capacity")


def test_null_impulses_are_an_array_of_zeros(w):
    lst, body_count = B.sized(257, "mixed")
    none = dict(lst, impulses=None)
    zeros = dict(lst, impulses=np.zeros(len(lst["data"]), dtype=S.IMPULSE))
    total = check_pairs(w, none, body_count, "impulses NULL")
    a, b = gpu_pairs(w, none, body_count, total), gpu_pairs(w, zeros, body_count, total)
    same(a, b, "NULL against zeros")
    assert not a[1]["impulse"][:total].view(np.uint32).any() and not a[1]["normal_impulse"][:total].view(np.uint32).any()


def test_capacity_one_short_exact_and_count_only(w):
    for lst, body_count in ((B.features(), 10), B.sized(257, "mixed")):
        total = HC.count_pairs(lst)
        assert total > 1
        same(gpu_pairs(w, lst, body_count, None), (total, None), "count only")
        same(gpu_pairs(w, lst, body_count, total - 1), (total, sentinel(total - 1 + SLACK)), "one short: the count, and every record byte the sentinel")
        same(gpu_pairs(w, lst, body_count, total), HC.pairs(lst, capacity=total, out=sentinel(total + SLACK)), "exact")
        same(gpu_pairs(w, lst, body_count, total + 7), HC.pairs(lst, capacity=total + 7, out=sentinel(total + 7 + SLACK)), "room to spare")


# ---- nh_contact_events --------------------------------------------------------------------------------------------------------------------------
def gpu_events(w, prev, cur, began_capacity, ended_capacity):
    began, ended = dev_out(w, began_capacity), dev_out(w, ended_capacity)
    w.contact_events_records(None if prev is None else dev_pairs(w, prev), dev_pairs(w, cur), began=began, ended=ended)
    return read(began), read(ended)


def want_events(prev, cur, began_capacity, ended_capacity):
    def room(c):
        return None if c is None else sentinel(c + SLACK)
    (nb, b), (ne, e) = HC.events(prev, cur, began_capacity=began_capacity or 0, ended_capacity=ended_capacity or 0,
                                 began=room(began_capacity), ended=room(ended_capacity))
    return (nb, None if began_capacity is None else b), (ne, None if ended_capacity is None else e)


def check_events(w, prev, cur, what):
    (nb, _), (ne, _) = HC.events(prev, cur)
    for caps in ((None, None), (nb, ne)):
        got, want = gpu_events(w, prev, cur, *caps), want_events(prev, cur, *caps)
        same(got[0], want[0], f"{what}: began, capacities {caps}")
        same(got[1], want[1], f"{what}: ended, capacities {caps}")
    return nb, ne


def test_events_of_every_crafted_case(w):
    cases = B.event_cases()
    B.check_event_cases(cases)
    for name, (prev, cur) in cases.items():
        check_events(w, prev, cur, name)
        nb, ne = check_events(w, None, cur, f"{name}, the first frame")
        assert nb == cur[0] and ne == 0
        nb, ne = check_events(w, cur, cur, f"{name}, identical lists")
        assert nb == 0 and ne == 0


def test_events_of_absent_inputs_and_small_outputs(w):
    prev, cur = B.event_cases()["both"]
    (nb, _), (ne, _) = HC.events(prev, cur)
    assert nb > 1 and ne > 1
    for a, b, what in (((prev[0], prev[1], prev[0] - 1), cur, "prev absent"), (prev, (cur[2] + 1, cur[1], cur[2]), "cur absent")):
        got = gpu_events(w, a, b, 4, 4)
        same(got[0], (0, sentinel(4 + SLACK)), f"{what}: began")
        same(got[1], (0, sentinel(4 + SLACK)), f"{what}: ended")
    for caps in ((nb - 1, ne), (nb, ne - 1), (nb - 1, ne - 1), (nb + 3, 0)):
        got, want = gpu_events(w, prev, cur, *caps), want_events(prev, cur, *caps)
        same(got[0], want[0], f"began, capacities {caps}")
        same(got[1], want[1], f"ended, capacities {caps}")
    assert gpu_events(w, prev, cur, nb - 1, ne)[0][1].tobytes() == sentinel(nb - 1 + SLACK).tobytes()


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_return_before_any_launch(w):
    import torch
    lst, body_count = B.sized(65, "mixed")
    d = dev_contacts(w, lst)
    L, ctx = w.L, w.ctx

    def contact_list(**kw):
        f = dict(data=d[0].data_ptr(), bodies=d[1].data_ptr(), impulses=d[2].data_ptr(), count=0, capacity=d[4], body_count=body_count)
        f.update(kw)
        return E.ContactList(f["data"], f["bodies"], f["impulses"], f["count"], f["capacity"], f["body_count"])

    outs = []

    def pair_list(**kw):
        o = dev_out(w, 8)          # (eight records, whatever capacity the struct then claims: nothing may be written)
        outs.append(o)
        f = dict(count=o[0].data_ptr(), pairs=o[1].data_ptr(), capacity=8)
        f.update(kw)
        return E.PairList(f["count"], f["pairs"], f["capacity"], 0)

    ok_in, ref = C.byref(contact_list()), C.byref
    bad_lists = [dict(pairs=0), dict(count=0), dict(capacity=1 << 31), dict(capacity=0xFFFFFFFF)]
    calls = [
        lambda: L.nh_contact_pairs(ctx, ok_in, ref(pair_list()), 1),
        lambda: L.nh_contact_pairs(ctx, None, ref(pair_list()), 0),
        lambda: L.nh_contact_pairs(ctx, ok_in, None, 0),
        lambda: L.nh_contact_pairs(None, ok_in, ref(pair_list()), 0),
        lambda: L.nh_contact_pairs(ctx, ref(contact_list(data=0)), ref(pair_list()), 0),
        lambda: L.nh_contact_pairs(ctx, ref(contact_list(bodies=0)), ref(pair_list()), 0),
        lambda: L.nh_contact_pairs(ctx, ref(contact_list(capacity=1 << 31)), ref(pair_list()), 0),
        lambda: L.nh_step_contact_pairs(ctx, ref(w.contacts), ref(w.cache), w.nb, ref(pair_list()), 2),
        lambda: L.nh_step_contact_pairs(ctx, None, ref(w.cache), w.nb, ref(pair_list()), 0),
        lambda: L.nh_step_contact_pairs(ctx, ref(w.contacts), None, w.nb, ref(pair_list()), 0),
        lambda: L.nh_step_contact_pairs(ctx, ref(w.contacts), ref(w.cache), w.nb, None, 0),
        lambda: L.nh_contact_events(ctx, None, ref(pair_list()), ref(pair_list()), ref(pair_list()), 4),
        lambda: L.nh_contact_events(ctx, None, None, ref(pair_list()), ref(pair_list()), 0),
        lambda: L.nh_contact_events(ctx, None, ref(pair_list()), None, ref(pair_list()), 0),
        lambda: L.nh_contact_events(ctx, None, ref(pair_list()), ref(pair_list()), None, 0),
    ]
    for bad in bad_lists:
        calls += [
            lambda bad=bad: L.nh_contact_pairs(ctx, ok_in, ref(pair_list(**bad)), 0),
            lambda bad=bad: L.nh_step_contact_pairs(ctx, ref(w.contacts), ref(w.cache), w.nb, ref(pair_list(**bad)), 0),
            lambda bad=bad: L.nh_contact_events(ctx, ref(pair_list(**bad)), ref(pair_list()), ref(pair_list()), ref(pair_list()), 0),
            lambda bad=bad: L.nh_contact_events(ctx, None, ref(pair_list(**bad)), ref(pair_list()), ref(pair_list()), 0),
            lambda bad=bad: L.nh_contact_events(ctx, None, ref(pair_list()), ref(pair_list(**bad)), ref(pair_list()), 0),
            lambda bad=bad: L.nh_contact_events(ctx, None, ref(pair_list()), ref(pair_list()), ref(pair_list(**bad)), 0),
        ]
    # misaligned `pairs` (8 bytes into the buffer) and a misaligned count word
    calls += [
        lambda: L.nh_contact_pairs(ctx, ok_in, ref(pair_list(pairs=outs[0][1].data_ptr() + 8)), 0),
        lambda: L.nh_contact_events(ctx, None, ref(pair_list()), ref(pair_list(pairs=outs[0][1].data_ptr() + 8)), ref(pair_list()), 0),
        lambda: L.nh_contact_pairs(ctx, ok_in, ref(pair_list(count=outs[0][1].data_ptr() + 2)), 0),
    ]
    for k, call in enumerate(calls):
        assert call() == NH_ERR_INVALID, f"call {k} did not return NH_ERR_INVALID"
    torch.cuda.synchronize()
    for o in outs:
        n, rec = read(o)
        assert n == 0xA5A5A5A5 and rec.tobytes() == sentinel(len(rec)).tobytes(), "an output was written by a call that returned NH_ERR_INVALID"
    # capacity 0 with a NULL count: the empty list -- *out->count = 0 and nothing else
    out = dev_out(w, 4)
    w.contact_pairs_records(None, None, None, count=None, capacity=0, body_count=0, out=out)
    same(read(out), (0, sentinel(4 + SLACK)), "capacity 0, count NULL")


# ---- nh_step_contact_pairs ----------------------------------------------------------------------------------------------------------------------
# single steps around the step numbers at which pairs begin and end in these worlds (the fall, the first landings and bounces)
WINDOWS = {
    "compound": (lambda: S.compound(), ((40, 46), (70, 78), (100, 108), (118, 124), (138, 142))),
    "pile": (lambda: S.pile(n_boxes=64, n_spheres=32), ((12, 16), (38, 44), (58, 68), (78, 83), (160, 166))),
}


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_step_contact_pairs_equals_the_oracle_on_the_downloaded_views(name):
    make, windows = WINDOWS[name]
    scene = make()
    wd = E.World(scene, flags=Q.FUSED)
    began_steps = ended_steps = multi_run = checked = 0
    for first, last in windows:
        wd.step(first - wd.steps_done)
        prev = None
        for _ in range(first, last + 1):
            cap = wd.max_contacts
            out = dev_out(wd, cap)
            wd.step_contact_pairs(out=out)
            wd.export_views(E.NH_VIEW_CONTACTS | E.NH_VIEW_CACHE)
            wd.synchronize()
            contacts, cache = wd.get_contacts(), wd.get_cache()
            n, rec = HC.step_pairs(contacts, cache, capacity=cap, out=sentinel(cap + SLACK))
            got = read(out)
            same(got, (n, rec), f"{name}, step {wd.steps_done}")
            assert int(rec["count"][:n].sum()) == contacts["count"]
            cur = (n, rec[:n].copy(), n)
            multi_run += HC.count_pairs(HC.contact_list(contacts["data"], contacts["bodies"])) < sum(1 for _ in B._runs(dict(bodies=contacts["bodies"])))
            if prev is not None:
                nb, ne = check_events(wd, prev, cur, f"{name}, steps {wd.steps_done - 1} -> {wd.steps_done}")
                began_steps += nb > 0
                ended_steps += ne > 0
            prev = cur
            checked += 1
            wd.step(1)
    wd.close()
    assert began_steps > 0 and ended_steps > 0, (began_steps, ended_steps, "the test must not pass on empty event lists")
    if name == "compound":
        assert multi_run > 0, "no pair of several runs: compound bodies carry several colliders"


# ---- speculation ----------------------------------------------------------------------------------------------------------------------------------
def _tiles():
    return S.grid_tiles(1, side=12, seed=2)


def test_the_pair_list_after_a_still_step_is_that_of_a_world_that_never_speculates():
    scene = _tiles()
    a, b = E.World(scene, flags=Q.FUSED), E.World(scene, flags=Q.FUSED)
    b.set_option("no_still", 1)
    landed = False
    for _ in range(40):          # (a world in free fall takes still steps too: wait for still steps of the LANDED world, every body on the ground)
        before = a.counts()["still_steps"]
        a.step(20); b.step(20)
        ca = a.counts()
        if ca["contacts"] >= a.nb - 1 and ca["still_steps"] > before:
            landed = True
            break
    assert landed and b.counts()["still_steps"] == 0, (a.counts(), b.counts())
    compared = 0
    cap = a.max_contacts
    for _ in range(24):
        before = a.counts()["still_steps"]
        a.step(1); b.step(1)
        if a.counts()["still_steps"] == before:
            continue
        oa, ob = dev_out(a, cap), dev_out(b, cap)
        a.step_contact_pairs(out=oa); b.step_contact_pairs(out=ob)
        ra, rb = read(oa), read(ob)
        same(ra, rb, f"after the still step {a.steps_done}")
        assert ra[0] > 0
        compared += 1
        if compared == 3:
            break
    assert compared > 0, "no still step among the steps looked at"
    a.close(); b.close()


def test_step_contact_pairs_between_nh_step_calls_changes_nothing():
    """Bodies, contacts, cache and nh_Counts -- the still and replay counters included -- are those of a world that never calls it."""
    def make_batch(a, scene):
        return (dev_out(a, a.max_contacts),)

    def query(a, out):
        a.step_contact_pairs(out=out)

    (out,) = LU.queries_between_nh_step_calls_change_nothing(_tiles, make_batch, query, "step_contact_pairs", still=True)
    assert read(out)[0] > 0
