"""Contact events without a GPU: nh_contact_pairs / nh_contact_events / nh_step_contact_pairs (include/nudge_hip.h, "contact events").

The declarations and the structs' layouts; the two oracles of tests/hostcontacts_util.py against each other byte for byte on every crafted batch
(tests/contact_batches.py) -- tests/hostoracle/hostcontacts.cpp, which runs the per-item functions of nudge_amd/csrc/nh_contact_events.h that the
device's lanes run, and an independent numpy implementation; hand-built lists with known answers; and the conditions of the batches the GPU tests compare
byte for byte, so that those tests cannot pass on lists that miss a rule."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_batches as B                  # noqa: E402
import hostcontacts_util as HC               # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

SENTINEL = 0xA5
CALLS = ("nh_contact_pairs", "nh_contact_events", "nh_step_contact_pairs")


def sentinel(n):
    return np.frombuffer(bytes([SENTINEL]) * 64 * max(n, 1), dtype=E.CONTACT_PAIR).copy()


# ---- the declarations -------------------------------------------------------------------------------------------------------------------------
def test_the_calls_are_declared_exported_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "nudge_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "int nh_contact_pairs(nh_context* ctx, const nh_ContactList* in, const nh_PairList* out, uint32_t flags );" in flat
    assert ("int nh_contact_events(nh_context* ctx, const nh_PairList* prev , const nh_PairList* cur, const nh_PairList* began, "
            "const nh_PairList* ended, uint32_t flags );") in flat
    assert ("int nh_step_contact_pairs(nh_context* ctx, const nh_ContactData* contacts, const nh_ContactCache* cache, uint32_t body_count, "
            "const nh_PairList* out, uint32_t flags );") in flat
    syms = subprocess.check_output(["nm", "-D", "--defined-only", E._LIB_PATH], text=True)
    for name in CALLS:
        assert name in E.EXPORTS
        assert re.search(r"\bT %s$" % name, syms, flags=re.M), name
        assert hasattr(E.lib(), name)
    for name in ("contact_pairs_records", "contact_events_records", "step_contact_pairs", "contact_events"):
        assert callable(getattr(E.World, name))
    assert list(inspect.signature(E.World.contact_events).parameters) == ["self", "prev", "cur", "capacity", "synchronize"]
    # the header says what the step-bound call reads between nh_collide and nh_write_cached_impulses
    text = re.sub(r"\s+", " ", hdr)
    assert "BETWEEN nh_collide AND nh_write_cached_impulses THE CACHE IS STILL LAST STEP'S" in text and "warm-start values" in text


def test_the_structs_are_laid_out_as_their_mirrors(tmp_path):
    probes = [("nh_ContactPair", "deepest", E.ContactPair), ("nh_ContactList", "body_count", E.ContactList), ("nh_PairList", "reserved", E.PairList)]
    members = {"nh_ContactPair": ("lo", "hi", "first", "count", "impulse", "normal_impulse", "position", "penetration", "normal", "deepest")}
    body = "".join(f'  printf("%zu %zu\\n", sizeof({c}), offsetof({c}, {m}));\n' for c, m, _ in probes)
    body += "".join(f'  printf("%zu\\n", offsetof(nh_ContactPair, {m}));\n' for m in members["nh_ContactPair"])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nudge_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    for (cname, member, mirror), line in zip(probes, lines):
        size, off = (int(v) for v in line.split())
        assert ctypes.sizeof(mirror) == size, (cname, ctypes.sizeof(mirror), size)
        assert getattr(mirror, member).offset == off, (cname, member)
    assert ctypes.sizeof(E.ContactPair) == 64 == E.CONTACT_PAIR.itemsize
    for m, line in zip(members["nh_ContactPair"], lines[len(probes):]):
        assert int(line) == getattr(E.ContactPair, m).offset == E.CONTACT_PAIR.fields[m][1], m


# ---- the batches hold what they are for ---------------------------------------------------------------------------------------------------------
def test_the_batches_contain_what_they_are_for():
    B.check_features(B.features())
    B.check_key_widths(B.key_widths())
    B.check_event_cases(B.event_cases())
    for mode in B.MODES:
        lst, body_count = B.sized(513, mode)
        n = HC.count_pairs(lst)
        assert n == {"one_pair": 1, "distinct": 513}.get(mode, n) and int(lst["bodies"].max()) < body_count
        if mode == "mixed":
            assert 1 < n < 513


# ---- hand-built answers -------------------------------------------------------------------------------------------------------------------------
def test_a_hand_built_list():
    data = np.zeros(5, dtype=S.CONTACT)
    data["position"] = [[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12], [13, 14, 15]]
    data["penetration"] = [0.1, 0.3, 0.2, 0.3, 0.05]
    data["normal"] = [[0, 1, 0], [0, 1, 0], [1, 0, 0], [0, -1, 0], [0, 0, 1]]
    imp = np.zeros(5, dtype=S.IMPULSE)
    imp["impulse"] = [[0, 2, 0], [1, 3, 0], [5, 0, 0], [0, -4, 1], [0, 0, 7]]
    lst = HC.contact_list(data, [[2, 1], [2, 1], [0, 3], [1, 2], [3, 0]], imp)
    for fn in (HC.pairs, HC.pairs_np):
        n, rec = fn(lst)
        assert n == 2
        a, b = rec[0], rec[1]
        assert (a["lo"], a["hi"], a["first"], a["count"], a["deepest"]) == (0, 3, 2, 2, 2)
        assert a["impulse"].tolist() == [5.0, 0.0, -7.0] and a["normal_impulse"] == 12.0          # (3, 0) is flipped: its impulse counts negated, its dot as it is
        assert a["position"].tolist() == [7.0, 8.0, 9.0] and a["normal"].tolist() == [1.0, 0.0, 0.0]
        assert (b["lo"], b["hi"], b["first"], b["count"], b["deepest"]) == (1, 2, 0, 3, 1)      # 0.3 twice: the lower index
        assert b["impulse"].tolist() == [-1.0, -9.0, 1.0] and b["normal_impulse"] == 9.0
        assert b["position"].tolist() == [4.0, 5.0, 6.0] and b["normal"].tolist() == [0.0, -1.0, 0.0] and b["penetration"] == np.float32(0.3)


def test_null_impulses_are_zeros():
    lst = B.features()
    zeros = dict(lst, impulses=np.zeros(len(lst["data"]), dtype=S.IMPULSE))
    none = dict(lst, impulses=None)
    for fn in (HC.pairs, HC.pairs_np):
        assert fn(zeros)[1].tobytes() == fn(none)[1].tobytes()
    assert not HC.pairs(none)[1]["impulse"].view(np.uint32).any(), "a sum of zeros of either sign is +0"


# ---- the two oracles, byte for byte -------------------------------------------------------------------------------------------------------------
def _lists():
    yield "features", B.features()
    for lst, body_count, _ in B.key_widths():
        yield f"key_width_{body_count}", lst
    for n in B.SIZES[:-1]:
        for mode in B.MODES:
            yield f"{mode}_{n}", B.sized(n, mode)[0]
    yield "mixed_70001", B.sized(B.SIZES[-1], "mixed")[0]


def test_the_cpp_oracle_equals_numpy_on_every_list():
    for name, lst in _lists():
        n, rec = HC.pairs(lst)
        m, ref = HC.pairs_np(lst)
        assert n == m, (name, n, m)
        assert rec[:n].tobytes() == ref[:n].tobytes(), (name, int((rec[:n] != ref[:n]).sum()))
        keys = (rec["lo"][:n].astype(np.uint64) << np.uint64(32)) | rec["hi"][:n]
        assert (keys[1:] > keys[:-1]).all(), name
        assert int(rec["count"][:n].sum()) == len(lst["data"]), name


def test_the_output_rule_on_the_host():
    lst = B.features()
    n, full = HC.pairs(lst)
    for fn in (HC.pairs, HC.pairs_np):
        m, out = fn(lst, capacity=n - 1, out=sentinel(n + 2))
        assert m == n and out.tobytes() == sentinel(n + 2).tobytes(), "one short: the count, and not a byte"
        m, out = fn(lst, capacity=n, out=sentinel(n + 2))
        assert m == n and out[:n].tobytes() == full[:n].tobytes() and out[n:].tobytes() == sentinel(2).tobytes()


def test_events_cpp_equals_numpy_on_every_case():
    cases = B.event_cases()
    for name, (prev, cur) in cases.items():
        for p in (prev, None):
            got, ref = HC.events(p, cur), HC.events_np(p, cur)
            for (n, rec), (m, exp) in zip(got, ref):
                assert n == m and rec[:n].tobytes() == exp[:m].tobytes(), (name, p is None, n, m)
            if p is None:
                assert got[0][0] == cur[0] and got[0][1][:cur[0]].tobytes() == cur[1][:cur[0]].tobytes() and got[1][0] == 0
    prev, cur = cases["both"]
    # identical lists; an absent input; an output too small
    for fn in (HC.events, HC.events_np):
        (nb, _), (ne, _) = fn(cur, cur)
        assert nb == 0 and ne == 0
        for absent in ((prev[0], prev[1], prev[0] - 1), (cur[2] + 1, cur[1], cur[2])):
            a, b = (absent, cur) if absent[1] is prev[1] else (prev, absent)
            (nb, rb), (ne, re_) = fn(a, b, began_capacity=4, ended_capacity=4, began=sentinel(4), ended=sentinel(4))
            assert nb == 0 and ne == 0 and rb.tobytes() == sentinel(4).tobytes() and re_.tobytes() == sentinel(4).tobytes()
        (nb, fb), (ne, fe) = fn(prev, cur)
        (mb, rb), (me, re_) = fn(prev, cur, began_capacity=nb - 1, ended_capacity=ne, began=sentinel(nb), ended=sentinel(ne))
        assert (mb, me) == (nb, ne) and rb.tobytes() == sentinel(nb).tobytes() and re_[:ne].tobytes() == fe[:ne].tobytes()


def test_the_step_bound_oracle_finds_its_cache_entries():
    lst = B.features()
    n = len(lst["data"])
    rng = np.random.default_rng(4)
    tags = np.sort(rng.integers(1, 40, size=n).astype(np.uint64) | (rng.integers(1, 40, size=n).astype(np.uint64) << np.uint64(32)))
    feats = np.arange(n, dtype=np.uint32)          # (unique (tag, feature), ascending within a tag)
    contacts = dict(count=n, data=lst["data"], bodies=lst["bodies"], tags=tags, features=feats)
    keep = rng.random(n) < 0.7                     # the cache: most of the contacts, shifted by the missing ones, and two strangers
    ct, cf, cd = tags[keep], feats[keep], lst["impulses"][keep]
    cache = dict(count=int(keep.sum()), tags=ct, features=cf, data=cd)
    expect = lst["impulses"].copy()
    expect["impulse"][~keep] = 0.0
    n1, got = HC.step_pairs(contacts, cache)
    n2, ref = HC.pairs_np(dict(lst, impulses=expect))
    assert 0 < int(keep.sum()) < n and n1 == n2 and got[:n1].tobytes() == ref[:n2].tobytes()
    n3, none = HC.step_pairs(contacts, dict(count=0, tags=ct[:0], features=cf[:0], data=cd[:0]))
    assert none[:n3].tobytes() == HC.pairs_np(dict(lst, impulses=None))[1][:n3].tobytes()
