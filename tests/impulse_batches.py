"""The crafted batches of the body-impulse tests (include/nudge_hip.h, "body impulses"): numpy alone, so that tests/test_cpu_impulses.py can hold the
two oracles of tests/hostimpulse_util.py against each other on exactly what tests/test_gpu_impulses.py sends to the device, and assert that each batch
holds what it is for (check_*): a GPU test then cannot pass on lists that miss a rule.

NaNs: the header leaves the payload of a sum with a NaN in it unspecified.  The batches hold ONE NaN, the canonical quiet one, in a record AT THE CENTRE:
it meets additions and one product only, which hand a quiet NaN operand on unchanged on the host and on the device alike -- a difference or a product
of two NaNs, whose sign the two may choose differently, never occurs."""
import numpy as np

import hostimpulse_util as HI
from nudge_amd import engine as E
from nudge_amd import scenes as S

F32 = np.float32
NAN = np.array([0x7FC00000], dtype=np.uint32).view(F32)[0]
NEG0 = F32(-0.0)
AT_CENTRE, NO_BODY = E.NH_IMPULSE_AT_CENTRE, E.NH_IMPULSE_NO_BODY
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 513, 70001)
MODES = ("mixed", "one_body", "distinct")
FEATURE_BODIES = 9          # S.pile(8, 0): the static world and eight boxes
ROTATED, MASSLESS, SEVERAL, SPLIT, BOTH_KINDS, MINUS_ZERO, NOT_A_NUMBER = 1, 2, 3, 4, 5, 6, 7          # what each body of features() is for; 8: no record


def unit(q):
    q = np.asarray(q, dtype=np.float64)
    return (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(F32)


def transforms(n, seed):
    """n body poses: random positions, random rotations; body 0 at the origin, unrotated."""
    rng = np.random.default_rng(seed)
    t = np.zeros(n, dtype=S.TRANSFORM)
    t["position"] = rng.uniform(-20.0, 20.0, size=(n, 3)).astype(F32)
    t["rotation"] = unit(rng.normal(size=(n, 4)))
    if n:
        t[0] = ((0, 0, 0), 0, (0, 0, 0, 1))
    return t


def feature_bodies(seed=5):
    """The nine bodies of features(): randomised poses, distinct inertia terms on every body, one massless body, momentum with set unused words."""
    rng = np.random.default_rng(seed)
    n = FEATURE_BODIES
    b = dict(transforms=transforms(n, seed), properties=np.zeros(n, dtype=S.PROPERTIES), momentum=np.zeros(n, dtype=S.MOMENTUM),
             idle=rng.integers(1, 200, size=n).astype(np.uint8))
    b["properties"]["inertia_inverse"][1:] = rng.uniform(0.05, 2.0, size=(n - 1, 3)).astype(F32)
    b["properties"]["mass_inverse"][1:] = rng.uniform(0.05, 0.5, size=n - 1).astype(F32)
    b["properties"][MASSLESS] = ((0, 0, 0), 0)
    b["momentum"]["velocity"] = rng.normal(size=(n, 3)).astype(F32)
    b["momentum"]["angular_velocity"] = rng.normal(size=(n, 3)).astype(F32)
    b["momentum"].view(np.uint32).reshape(n, 8)[:, 3] = 0xDEAD0000 + np.arange(n)          # unused0 / unused1: bit patterns that are no numbers
    b["momentum"].view(np.uint32).reshape(n, 8)[:, 7] = 0x7FA00000 + np.arange(n)          # (signalling NaNs: moved as bits or not at all)
    b["momentum"][0] = np.zeros(1, dtype=S.MOMENTUM)[0]
    return b


def features(bodies=None):
    """One list with every rule of the header in it, for FEATURE_BODIES bodies."""
    t = (bodies or feature_bodies())["transforms"]
    rows = []

    def rec(body, impulse, offset=None, flags=0):
        """offset: the point relative to the body's centre (None: at the centre)"""
        point = (0.0, 0.0, 0.0) if offset is None else (t[body]["position"] if body < len(t) else 0.0) + np.asarray(offset, dtype=F32)
        rows.append((body, impulse, point, flags | (AT_CENTRE if offset is None else 0)))

    big, small = 1.0e8, 3.0
    rec(SEVERAL, (big, 1, 2), (0.5, 0, 0)); rec(SEVERAL, (small, 1, 2), (0, 0.5, 0))          # run 1 of SEVERAL
    rec(ROTATED, (1, 2, 3), (0.25, -0.5, 1.0))
    rec(SEVERAL, (-big, 3, 1), (0, 0, 0.5)); rec(SEVERAL, (small, 1, 1), (0.5, 0.5, 0))       # run 2: big + small - big + small tells the associations apart
    rec(0, (9, 9, 9)); rec(NO_BODY, (9, 9, 9), (1, 1, 1)); rec(FEATURE_BODIES, (9, 9, 9))      # nobody's: the static world, NO_BODY, body == count
    rec(SEVERAL, (0.125, 0, 0))                                                                 # run 3, behind invalid records
    rec(SPLIT, (1, 0, 0), (0, 1, 0)); rec(0, (5, 5, 5)); rec(SPLIT, (0, 1, 0), (1, 0, 0))      # two runs of one body, split by an invalid record alone
    rec(BOTH_KINDS, (0, 0, 2)); rec(BOTH_KINDS, (0, 0, 2), (1, 0, 0)); rec(BOTH_KINDS, (1, 1, 1), (5, 5, 5), AT_CENTRE)   # (the last: a point that is not read)
    rec(MINUS_ZERO, (NEG0, NEG0, NEG0))
    rec(NOT_A_NUMBER, (NAN, 1, 2)); rec(NOT_A_NUMBER, (1, 1, 1))
    rec(MASSLESS, (4, 5, 6), (0.5, 0.5, 0.5))
    rec(ROTATED, (0.5, 0.25, -1), (-1, 0.5, 0.25))                                              # ROTATED's second run
    out = np.zeros(len(rows), dtype=E.BODY_IMPULSE)
    for k, (body, impulse, point, flags) in enumerate(rows):
        out[k] = (point, body, impulse, flags)
    return out


def check_features(bodies, lst):
    t, n = bodies["transforms"], FEATURE_BODIES
    groups = HI._groups(lst, len(lst), n)
    assert len(groups[SEVERAL]) >= 3 and len(groups[SPLIT]) == 2 and len(groups[ROTATED]) == 2
    at = [i for run in groups[SPLIT] for i in run]
    assert at[1] == at[0] + 2 and int(lst[at[0] + 1]["body"]) == 0, "SPLIT's runs are split by one invalid record"
    assert {0, NO_BODY, n} <= set(int(b) for b in lst["body"]) and 8 not in groups
    kinds = [int(lst[i]["flags"]) & AT_CENTRE for run in groups[BOTH_KINDS] for i in run]
    assert 0 in kinds and AT_CENTRE in kinds
    (_, two), (_, flat) = HI.sums_np(t, lst), HI.sums_np(t, lst, flat=True)
    by = {int(r["body"]): r for r in two}
    assert two[by[SEVERAL]["body"] == two["body"]].tobytes() != flat[flat["body"] == SEVERAL].tobytes(), "the two associations give the same bits"
    assert not by[MINUS_ZERO]["linear"].view(np.uint32).any(), "+0 + -0 is +0"
    assert lst[groups[MINUS_ZERO][0][0]]["impulse"].view(np.uint32).tolist() == [0x80000000] * 3
    assert np.isnan(by[NOT_A_NUMBER]["linear"][0]) and not np.isnan(by[NOT_A_NUMBER]["linear"][1:]).any()
    assert bodies["properties"][MASSLESS]["mass_inverse"] == 0 and MASSLESS in groups
    ii, q = bodies["properties"][ROTATED]["inertia_inverse"], t[ROTATED]["rotation"]
    assert len(set(ii.tolist())) == 3 and np.count_nonzero(q) == 4
    assert [int(r["body"]) for r in two] == sorted(groups) and int(two["count"].sum()) == sum(len(r) for g in groups.values() for r in g)


def sized(n, mode, seed=11):
    """(transforms, list): n records.  "mixed": 300 bodies, runs of 1 - 4 records, one record in eight nobody's, a third at the centre; "one_body": every
    record body 1's, of a world of two bodies; "distinct": record i is body n - i's."""
    rng = np.random.default_rng(seed + n)
    if mode == "one_body":
        body = np.ones(n, dtype=np.uint32)
        count = 2
    elif mode == "distinct":
        body = (n - np.arange(n)).astype(np.uint32)
        count = n + 1
    else:
        count = 300
        heads = rng.integers(1, count, size=n + 1)
        body = heads[np.cumsum(rng.random(n) < 0.5)].astype(np.uint32)
        nobody = rng.random(n) < 0.125
        body[nobody] = rng.choice(np.array([0, count, count + 7, NO_BODY], dtype=np.uint32), size=int(nobody.sum()))
    t = transforms(count, seed)
    lst = np.zeros(n, dtype=E.BODY_IMPULSE)
    lst["body"] = body
    lst["impulse"] = (rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-3, 4, size=(n, 1))).astype(F32)
    lst["point"] = t["position"][np.minimum(body, count - 1)] + rng.normal(size=(n, 3)).astype(F32)
    lst["flags"] = np.where(rng.random(n) < 0.33, AT_CENTRE, 0)
    return t, lst


def key_widths():
    """[(body_count, used bodies, their transforms, list, key bytes)]: worlds whose sort takes 1, 2, 3 and 4 passes, with records on the highest bodies and
    on bodies that differ in the top byte alone.  The transforms are given sparsely: every other body's are zeros (dense())."""
    cases = []
    for passes, count in ((1, 256), (2, 65536), (3, (1 << 24)), (4, (1 << 24) + 2)):
        rng = np.random.default_rng(count)
        top = count - 1
        used = np.unique(np.array([1, 2, 255 % count, top, top - 1, top >> 8 or 3, (top >> 16) or 4, top & 0xFF or 5, top & 0xFFFF or 6], dtype=np.uint32))
        used = used[used > 0]
        t = transforms(len(used), count)
        t["position"] += 1.0
        body = np.concatenate([used[::-1], used, rng.permutation(used), used[::-1]]).astype(np.uint32)
        lst = np.zeros(len(body), dtype=E.BODY_IMPULSE)
        lst["body"] = body
        lst["impulse"] = rng.normal(size=(len(body), 3)).astype(F32)
        lst["point"] = rng.normal(size=(len(body), 3)).astype(F32)
        lst["flags"][::3] = AT_CENTRE
        cases.append((count, used, t, lst, passes))
    return cases


def dense(count, used, t):
    """The host's whole transform array of a key_widths case (untouched pages of zeros cost nothing)."""
    out = np.zeros(count, dtype=S.TRANSFORM)
    out[used] = t
    return out


def check_key_widths(cases):
    assert [c[4] for c in cases] == [1, 2, 3, 4]
    for count, used, _, lst, passes in cases:
        assert HI.key_bytes(count) == passes and int(used.max()) == count - 1 and used.min() > 0
        assert len(np.unique(lst["body"])) == len(used) and len(lst) == 4 * len(used)


# ---- blasts ---------------------------------------------------------------------------------------------------------------------------------
def blast_cases():
    """{name: (transforms, blasts, offsets, hits)}: hit lists for two or three blasts each."""
    t = transforms(12, 21)
    centre = np.array([1.0, 2.0, -3.0], dtype=F32)
    t["position"][1] = centre                                        # d == 0
    t["position"][2] = centre + np.array([3, 0, 4], dtype=F32)        # d == 5 exactly
    t["position"][3] = centre + np.array([0, 6, 8], dtype=F32)        # d == 10
    t["position"][4] = centre + np.array([1, 2, 2], dtype=F32)        # d == 3

    def blasts(*rows):
        b = np.zeros(len(rows), dtype=E.BLAST)
        for k, (c, radius, strength, falloff) in enumerate(rows):
            b[k]["centre"], b[k]["radius"], b[k]["strength"], b[k]["falloff"] = c, radius, strength, falloff
        return b

    def hits(*segments):
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in segments])]).astype(np.uint32)
        h = np.zeros(int(offsets[-1]), dtype=E.OVERLAP_HIT)
        h["body"] = [b for s in segments for b in s]
        h["collider"], h["tag"] = np.arange(len(h)), 7
        return offsets, h

    everybody = [1, 2, 3, 4, 0, 12, 5, NO_BODY, 11]
    return {
        "falloff 1 and 0": (t, blasts((centre, 5.0, 10.0, 1.0), (centre, 5.0, 10.0, 0.0)), *hits(everybody, everybody)),
        "an empty segment between two": (t, blasts((centre, 20.0, 2.0, 1.0), (centre, 1.0, 1.0, 1.0), (t["position"][7], 15.0, -3.0, 0.5)), *hits([1, 2, 6], [], [7, 8, 9, 10, 11])),
        "one record": (t, blasts((centre, 4.0, 1.0, 0.5)), *hits([4])),
    }


def check_blast_cases(cases):
    t, b, offsets, h = cases["falloff 1 and 0"]
    out = HI.blast_np(t, b, offsets, h)
    n = int(offsets[1])
    first, second = out[:n], out[n:2 * n]
    body = h["body"][:n].tolist()
    at = {k: body.index(k) for k in (1, 2, 3, 4)}
    assert first[at[1]]["impulse"].tolist() == [0.0, 10.0, 0.0], "d == 0: straight up, full strength"
    assert int(first[at[2]]["body"]) == NO_BODY and int(first[at[3]]["body"]) == NO_BODY, "falloff 1: nothing at d == radius or beyond"
    assert int(first[at[4]]["body"]) == 4 and abs(float(np.linalg.norm(first[at[4]]["impulse"])) - 4.0) < 1e-5
    assert all(abs(float(np.linalg.norm(second[at[k]]["impulse"])) - 10.0) < 1e-5 for k in (2, 3, 4)), "falloff 0: full strength at any distance"
    assert all(int(first[body.index(k)]["body"]) == NO_BODY for k in (0, 12, NO_BODY)) and int(first[body.index(11)]["body"]) in (11, NO_BODY)
    assert not first[at[2]].tobytes()[:12].strip(b"\0") and first[at[2]]["flags"] == 0, "a NO_BODY record's other words are 0"
    offsets = cases["an empty segment between two"][2]
    assert offsets[1] == offsets[2] and offsets[3] > offsets[2]


# ---- touches --------------------------------------------------------------------------------------------------------------------------------
TOUCH_K = 4


def touch_case(seed=31):
    """(pushes, k, counts, touches): six movers of TOUCH_K slots.  Slots at and behind counts[i] are poison: NaNs and a body that would be real."""
    rng = np.random.default_rng(seed)
    n, k = 6, TOUCH_K
    pushes = np.zeros(n, dtype=E.PUSH)
    pushes["mass_over_dt"], pushes["max_impulse"] = 80.0 * 60.0, 1.0e9
    pushes["phases"] = [0b11111, 0b00101, 0b11111, 0b11111, 0, 0b11111]
    pushes["flags"] = [0, AT_CENTRE, 0, 0, 0, AT_CENTRE]
    pushes["max_impulse"][3] = 2.5                                      # mover 3: clamped
    counts = np.array([4, 4, 2, 9, 4, 0], dtype=np.uint32)              # (9: more than k, clamped; 0: nothing written)
    t = np.zeros((n, k), dtype=E.TOUCH)
    t["origin"] = rng.uniform(-5, 5, size=(n, k, 3)).astype(F32)
    d = unit(rng.normal(size=(n, k, 3)))
    t["direction"] = d
    nrm = unit(-d + 0.3 * rng.normal(size=(n, k, 3)))                   # roughly against the direction: approaching
    t["hit"]["normal"] = nrm
    t["hit"]["t"] = rng.uniform(0.1, 2.0, size=(n, k)).astype(F32)
    t["hit"]["body"] = rng.integers(1, 9, size=(n, k))
    t["hit"]["shape"], t["hit"]["collider"], t["hit"]["tag"] = 0, 3, 5
    t["phase"] = np.add.outer(np.arange(n), np.arange(k)) % 5                    # every phase, in every mask
    t["cast"] = np.arange(k)
    t["hit"]["t"][0, 1] = 0.0                                           # a touch at the start of its cast
    t["hit"]["normal"][0, 2] = d[0, 2]                                  # receding: the normal along the direction
    t["hit"]["shape"][0, 3] = HI.NONE
    t["hit"]["body"][3, 0] = 0                                          # the static world
    t["phase"][3, 2] = 40                                               # no phase at all
    for i in range(n):                                                  # poison behind the counts
        for j in range(min(int(counts[i]), k), k):
            t[i, j] = np.frombuffer(np.full(16, 0x7FC00000, dtype=np.uint32).tobytes(), dtype=E.TOUCH)[0]
            t[i, j]["hit"]["body"], t[i, j]["hit"]["shape"], t[i, j]["phase"] = 1, 0, 0
    return pushes, k, counts, t


def check_touch_case(case):
    pushes, k, counts, t = case
    out = HI.touch_np(pushes, k, counts, t).reshape(len(pushes), k)
    real = out["body"] != NO_BODY
    assert set(int(p) for p in t["phase"][real]) == {0, 1, 2, 3, 4}, "a pushing touch of every phase"
    assert not real[0, 1] and not real[0, 2] and not real[0, 3] and real[0, 0], "t == 0, receding, no shape"
    assert not real[2, 2:].any() and real[2, :2].all() and not real[5].any() and not real[4].any(), "slots at and behind counts[i]; an empty mask"
    assert real[1].tolist() == [bool((0b00101 >> int(p)) & 1) for p in t["phase"][1]], "the phase mask"
    assert not real[3, 0] and not real[3, 2] and real[3, 1] and real[3, 3], "body 0, phase 40; counts above k"
    assert all(abs(float(np.linalg.norm(out[3, j]["impulse"])) - 2.5) < 1e-5 for j in (1, 3)), "clamped by max_impulse"
    assert float(np.linalg.norm(out[0, 0]["impulse"])) > 100.0
    assert (out["flags"][1][real[1]] == AT_CENTRE).all() and (out["flags"][0][real[0]] == 0).all()
    assert not out[~real].view(np.uint32).reshape(-1, 8)[:, [0, 1, 2, 4, 5, 6, 7]].any(), "a NO_BODY record's other words are 0"
