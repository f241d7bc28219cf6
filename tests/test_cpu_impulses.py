"""Body impulses without a GPU: nh_impulse_sums / nh_body_impulses / nh_blast_impulses / nh_touch_impulses (include/nudge_hip.h, "body impulses").

The declarations and the structs' layouts; the two oracles of tests/hostimpulse_util.py against each other byte for byte on every crafted batch
(tests/impulse_batches.py) -- tests/hostoracle/hostimpulse.cpp, which runs the per-item functions of nudge_amd/csrc/nh_impulse.h that the device's
lanes run, and an independent numpy implementation; hand-built lists with known answers; and the conditions of the batches the GPU tests compare byte
for byte, so that those tests cannot pass on lists that miss a rule."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostimpulse_util as HI                # noqa: E402
import impulse_batches as B                  # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

SENTINEL = 0xA5
CALLS = ("nh_impulse_sums", "nh_body_impulses", "nh_blast_impulses", "nh_touch_impulses")
NUMPY_SIZES = tuple(n for n in B.SIZES if n <= 513)          # (the explicit numpy loops are slow: 70,001 records once, below)


def sentinel(n):
    return np.frombuffer(bytes([SENTINEL]) * 32 * max(n, 1), dtype=E.IMPULSE_SUM).copy()


# ---- the declarations -------------------------------------------------------------------------------------------------------------------------
def test_the_calls_are_declared_exported_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "nudge_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "int nh_impulse_sums (nh_context* ctx, const nh_BodyData* bodies, const nh_ImpulseList* in, const nh_ImpulseSumList* out, uint32_t flags );" in flat
    assert "int nh_body_impulses(nh_context* ctx, const nh_BodyData* bodies, const nh_ImpulseList* in, uint32_t flags );" in flat
    assert ("int nh_blast_impulses(nh_context* ctx, const nh_BodyData* bodies, const nh_Blast* blasts, uint32_t count, const nh_HitList* hits, "
            "nh_BodyImpulse* out, uint32_t flags );") in flat
    assert ("int nh_touch_impulses (nh_context* ctx, const nh_Push* pushes, uint32_t count, uint32_t k, const uint32_t* counts, const nh_Touch* touches, "
            "nh_BodyImpulse* out, uint32_t flags );") in flat
    syms = subprocess.check_output(["nm", "-D", "--defined-only", E._LIB_PATH], text=True)
    for name in CALLS:
        assert name in E.EXPORTS
        assert re.search(r"\bT %s$" % name, syms, flags=re.M), name
        assert hasattr(E.lib(), name)
    for name in ("impulse_sums_records", "body_impulses_records", "blast_impulses_records", "touch_impulses_records", "body_impulses", "blast"):
        assert callable(getattr(E.World, name))
    text = re.sub(r"\s+", " ", hdr)
    for line in ("velocity-change records", "torque-only records", "forces over time", "impulses on partitioned worlds", "`namespace nudge` extension",
                 "a second path for huge bodies", "merged by ONE lane: correct and slow"):
        assert line in text, line


def test_the_structs_are_laid_out_as_their_mirrors(tmp_path):
    probes = [("nh_BodyImpulse", "flags", E.BodyImpulse, E.BODY_IMPULSE), ("nh_ImpulseList", "reserved", E.ImpulseList, None),
              ("nh_ImpulseSum", "angular", E.ImpulseSum, E.IMPULSE_SUM), ("nh_ImpulseSumList", "reserved", E.ImpulseSumList, None),
              ("nh_Blast", "reserved", E.Blast, E.BLAST), ("nh_Push", "flags", E.Push, E.PUSH)]
    body = "".join(f'  printf("%zu %zu\\n", sizeof({c}), offsetof({c}, {m}));\n' for c, m, _, _ in probes)
    body += '  printf("%u %u %u\\n", (unsigned)NH_IMPULSE_AT_CENTRE, (unsigned)NH_IMPULSE_NO_BODY, (unsigned)NH_IMPULSE_WAKE);\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nudge_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    for (c, m, mirror, dtype), line in zip(probes, lines):
        size, off = (int(x) for x in line.split())
        assert (size, off) == (C.sizeof(mirror), getattr(mirror, m).offset), (c, size, off)
        if dtype is not None:
            assert (size, off) == (dtype.itemsize, dtype.fields[m][1]), (c, size, off)
    assert [int(x) for x in lines[len(probes)].split()] == [E.NH_IMPULSE_AT_CENTRE, E.NH_IMPULSE_NO_BODY, E.NH_IMPULSE_WAKE]
    assert C.sizeof(E.BodyImpulse) == C.sizeof(E.ImpulseSum) == C.sizeof(E.Blast) == 32 and C.sizeof(E.Push) == 16


import ctypes as C          # noqa: E402


# ---- the two oracles against each other ----------------------------------------------------------------------------------------------------------
def same_sums(t, lst, what, count=None, body_count=None):
    total = HI.count_sums(t, lst, count, body_count)
    for cap in (total, total + 3, max(total - 1, 0), 0):
        a = HI.sums(t, lst, count, capacity=cap, out=sentinel(cap + 2), body_count=body_count)
        b = HI.sums_np(t, lst, count, capacity=cap, out=sentinel(cap + 2), body_count=body_count)
        assert a[0] == b[0] == total and a[1].tobytes() == b[1].tobytes(), f"{what}, capacity {cap}: the oracles differ"
        if cap < total:
            assert a[1].tobytes() == sentinel(cap + 2).tobytes(), f"{what}: records written although they do not all fit"
    return total


def test_the_feature_batch_holds_every_rule_and_the_oracles_agree_on_it():
    bodies = B.feature_bodies()
    lst = B.features(bodies)
    B.check_features(bodies, lst)
    assert same_sums(bodies["transforms"], lst, "features") == 7
    for wake in (False, True):
        (ma, ia), (mb, ib) = HI.apply(bodies, lst, wake=wake), HI.apply_np(bodies, lst, wake=wake)
        assert ma.tobytes() == mb.tobytes() and ia.tobytes() == ib.tobytes(), f"apply, wake {wake}: the oracles differ"
        before = bodies["momentum"].view(np.uint32).reshape(-1, 8)
        after = ma.view(np.uint32).reshape(-1, 8)
        assert (after[:, [3, 7]] == before[:, [3, 7]]).all(), "unused0 / unused1 keep their bits"
        assert after[[0, 8]].tobytes() == before[[0, 8]].tobytes(), "bodies without a record are untouched"
        assert ma[B.MASSLESS].tobytes() == bodies["momentum"][B.MASSLESS].tobytes(), "mass_inverse == 0 and no inertia: nothing moves"
        changed = [b for b in range(B.FEATURE_BODIES) if ma[b].tobytes() != bodies["momentum"][b].tobytes()]
        assert changed == [B.ROTATED, B.SEVERAL, B.SPLIT, B.BOTH_KINDS, B.NOT_A_NUMBER], changed          # (MINUS_ZERO: v + 0 is v)
        touched = sorted(set(changed) | {B.MASSLESS, B.MINUS_ZERO})
        assert (ia[touched] == 0).all() == wake and (np.delete(ia, touched) == np.delete(bodies["idle"], touched)).all()
        if not wake:
            assert ia.tobytes() == bodies["idle"].tobytes()


def test_known_answers():
    t = np.zeros(4, dtype=S.TRANSFORM)
    t["rotation"] = (0, 0, 0, 1)
    t["position"][2] = (1, 0, 0)
    lst = HI.records([2, 2, 3], [(0, 1, 0), (0, 1, 0), (1, 0, 0)], point=[(2, 0, 0), (1, 0, 5), (0, 0, 0)], flags=[0, E.NH_IMPULSE_AT_CENTRE, 0])
    n, s = HI.sums(t, lst)
    assert n == 2 and s["body"].tolist() == [2, 3] and s["count"].tolist() == [2, 1]
    assert s[0]["linear"].tolist() == [0, 2, 0] and s[0]["angular"].tolist() == [0, 0, 1]          # (1, 0, 0) x (0, 1, 0); the second record: at the centre
    assert s[1]["linear"].tolist() == [1, 0, 0] and s[1]["angular"].tolist() == [0, 0, 0]
    bodies = dict(transforms=t, properties=np.zeros(4, dtype=S.PROPERTIES), momentum=np.zeros(4, dtype=S.MOMENTUM), idle=np.full(4, 9, dtype=np.uint8))
    bodies["properties"][2] = ((1, 2, 4), 0.5)
    m, idle = HI.apply(bodies, lst, wake=True)
    assert m[2]["velocity"].tolist() == [0, 1, 0] and m[2]["angular_velocity"].tolist() == [0, 0, 4] and idle.tolist() == [9, 9, 0, 0]
    assert HI.count_sums(t, lst, count=1) == 1 and HI.count_sums(t, lst, count=99) == 2 and HI.count_sums(t, lst[:0]) == 0


@pytest.mark.parametrize("mode", B.MODES)
def test_the_oracles_agree_on_lists_of_every_size(mode):
    for n in NUMPY_SIZES:
        t, lst = B.sized(n, mode)
        total = same_sums(t, lst, f"{mode} {n}")
        assert total == {"one_body": min(n, 1), "distinct": n}.get(mode, total)
        if n == 513:
            for keep in (300, 1, 0, 100000):
                same_sums(t, lst, f"{mode} {n}, count {keep}", count=keep)


def test_the_oracles_agree_on_the_largest_list():
    t, lst = B.sized(B.SIZES[-1], "mixed")
    a, b = HI.sums(t, lst), HI.sums_np(t, lst)
    assert a[0] == b[0] > 250 and a[1].tobytes() == b[1].tobytes(), "mixed, the largest: the oracles differ"
    for mode in ("one_body", "distinct"):
        t, lst = B.sized(B.SIZES[-1], mode)
        assert HI.count_sums(t, lst) == (1 if mode == "one_body" else len(lst))


def test_the_oracles_agree_on_every_key_width():
    cases = B.key_widths()
    B.check_key_widths(cases)
    for count, used, t, lst, passes in cases:
        assert same_sums(B.dense(count, used, t), lst, f"{passes} key bytes") == len(used)


def test_the_oracles_agree_on_the_blasts_and_the_touches():
    cases = B.blast_cases()
    B.check_blast_cases(cases)
    for name, (t, blasts, offsets, hits) in cases.items():
        for cap in (len(hits), max(len(hits) - 2, 0)):
            fill = np.frombuffer(bytes([SENTINEL]) * 32 * (len(hits) + 2), dtype=E.BODY_IMPULSE)
            a, b = HI.blast(t, blasts, offsets, hits, capacity=cap, out=fill.copy()), HI.blast_np(t, blasts, offsets, hits, capacity=cap, out=fill.copy())
            assert a.tobytes() == b.tobytes(), f"{name}, capacity {cap}: the oracles differ"
            assert a[cap:].tobytes() == fill[cap:].tobytes()
    case = B.touch_case()
    B.check_touch_case(case)
    assert HI.touch(*case).tobytes() == HI.touch_np(*case).tobytes()
