"""Crafted inputs of the contact-event tests (tests/test_cpu_contact_events.py, tests/test_gpu_contact_events.py): contact lists and pair lists, and
check_*() functions that assert that each holds what it is for -- so that neither test can pass on lists that do not exercise the rules.

A contact list is hostcontacts_util's: dict(data, bodies, impulses).  A pair list is (count, records, capacity)."""
import numpy as np

import hostcontacts_util as HC
from nudge_amd import engine as E
from nudge_amd import scenes as S

NAN = np.float32(np.nan)
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 513, 70001)
MODES = ("mixed", "one_pair", "distinct")


def _fill(rng, bodies, pens=None, impulse_x=None):
    """A contact list over the (a, b) rows of `bodies` with random positions, normals, impulses; pens / impulse_x: values to put in place (None entries
    keep the random ones)."""
    n = len(bodies)
    data = np.zeros(n, dtype=S.CONTACT)
    data["position"] = rng.uniform(-50.0, 50.0, size=(n, 3))
    data["penetration"] = rng.uniform(-0.01, 0.2, size=n)
    nrm = rng.normal(size=(n, 3))
    data["normal"] = nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-9)
    data["friction"] = 0.5
    imp = np.zeros(n, dtype=S.IMPULSE)
    imp["impulse"] = rng.normal(size=(n, 3)) * rng.choice([1e-3, 1.0, 3e4], size=(n, 1))
    imp["unused"] = rng.integers(0, 64, size=n).astype(np.uint32).view(np.float32)          # (the solver keeps a colour there: not to be read as a number)
    for k, v in enumerate(pens or []):
        if v is not None:
            data["penetration"][k] = v
    for k, v in enumerate(impulse_x or []):
        if v is not None:
            imp["impulse"][k, 0] = v
    return HC.contact_list(data, np.array(bodies, dtype=np.uint32).reshape(-1, 2), imp)


def features():
    """ONE list with every rule in it; check_features() says what and asserts it."""
    rows = [
        # pair (1, 2), run A: both orientations; impulse x = 2^24, then a flipped 0 and a 0
        ((1, 2), None, 16777216.0), ((2, 1), None, 0.0), ((1, 2), None, 0.0),
        ((0, 3), None, None),                                       # a run of 1
        # pair (1, 2), run B, flipped: x = -1, -1 contribute +1, +1 -- two-level 2^24 + 2, flat 2^24
        ((2, 1), None, -1.0), ((2, 1), None, -1.0),
        ((4, 4), None, None),                                       # lo == hi
        *[((0, 5), None, None)] * 10,                               # a run of 10
        ((1, 2), None, 0.0),                                        # pair (1, 2), run C: three non-adjacent runs
        ((3, 6), 0.5, None), ((6, 3), 0.5, None), ((3, 6), 0.25, None),          # a penetration tie: the lower index stays
        ((3, 7), NAN, None), ((3, 7), 1.0, None), ((7, 3), 2.0, None),           # a NaN first in its pair: never replaced
        ((6, 7), 0.1, None), ((7, 6), NAN, None), ((6, 7), 0.3, None),           # a NaN that is not first: never replaces
        ((2, 8), 0.2, None),
        ((5, 9), NAN, None), ((5, 9), 5.0, None),                                # a NaN first in its pair, the pair in two runs
        ((8, 2), NAN, None), ((2, 8), 0.9, None),                                # a NaN first in its RUN, not in its pair: the run still counts
        ((9, 5), 7.0, None),
        ((2, 9), 0.3, None), ((0, 3), None, None), ((2, 9), NAN, None), ((9, 2), NAN, None),   # a run of NaNs only, behind a number
        ((0, 3), None, None), ((3, 0), None, None),                 # a run of 2
    ]
    rng = np.random.default_rng(11)
    return _fill(rng, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])


def _runs(lst):
    """[(lo, hi, first index, length)] in list order."""
    out = []
    for i, (a, b) in enumerate(lst["bodies"].tolist()):
        key = (min(a, b), max(a, b))
        if out and out[-1][:2] == key and out[-1][2] + out[-1][3] == i:
            out[-1] = (*key, out[-1][2], out[-1][3] + 1)
        else:
            out.append((*key, i, 1))
    return out


def check_features(lst):
    runs = _runs(lst)
    by_pair = {}
    for lo, hi, first, length in runs:
        by_pair.setdefault((lo, hi), []).append((first, length))
    bodies, pen = lst["bodies"], lst["data"]["penetration"]
    members = {k: [i for f, n in v for i in range(f, f + n)] for k, v in by_pair.items()}
    assert any(len({bool(bodies[i, 0] > bodies[i, 1]) for i in m}) == 2 for m in members.values()), "no pair with contacts in both orientations"
    assert any(len(v) >= 3 for v in by_pair.values()), "no pair split over three runs"
    lengths = {n for _, _, _, n in runs}
    assert 1 in lengths and 2 in lengths and max(lengths) >= 9, lengths
    assert any(lo == hi for lo, hi in by_pair), "no pair with lo == hi"
    ties = nan_first = nan_later = nan_run_head = 0
    for key, m in members.items():
        p = pen[m]
        top = np.nanmax(p) if not np.isnan(p).all() else None
        ties += top is not None and int((p == top).sum()) >= 2 and not np.isnan(p[0])
        nan_first += bool(np.isnan(p[0])) and len(m) > 1
        nan_later += (not np.isnan(p[0])) and bool(np.isnan(p[1:]).any())
        nan_run_head += any(np.isnan(pen[f]) and f != m[0] and n > 1 and not np.isnan(pen[f:f + n]).all() for f, n in by_pair[key])
    assert ties and nan_first and nan_later and nan_run_head, (ties, nan_first, nan_later, nan_run_head)
    _, two = HC.pairs_np(lst)
    _, flat = HC.pairs_np(lst, flat=True)
    assert (two["impulse"].view(np.uint32) != flat["impulse"].view(np.uint32)).any(), "the two-level sums equal the flat ones: a wrong association would pass"
    assert all(np.array_equal(two[k], flat[k]) for k in ("lo", "hi", "first", "count", "deepest"))


def sized(n, mode, seed=5):
    """(contact list, body_count) of n contacts: "mixed" -- runs of 1 to 12 contacts over few bodies, so that pairs come back in later runs, in both
    orientations; "one_pair" -- all of them one pair; "distinct" -- n pairs, none twice, in shuffled order."""
    rng = np.random.default_rng(seed + n)
    if mode == "one_pair":
        bodies = np.where((np.arange(n) % 3 == 1)[:, None], [5, 3], [3, 5])
        return _fill(rng, bodies), 6
    if mode == "distinct":
        a = rng.permutation(n).astype(np.int64)
        bodies = np.stack([a, a + n], axis=1)
        flip = rng.random(n) < 0.5
        bodies[flip] = bodies[flip][:, ::-1]
        return _fill(rng, bodies), 2 * n + 1
    nb = max(2, n // 7)
    rows = []
    while len(rows) < n:
        a, b = (int(v) for v in rng.integers(0, nb, size=2))
        for _ in range(min(int(rng.integers(1, 13)), n - len(rows))):
            rows.append((a, b) if rng.random() < 0.7 else (b, a))
    return _fill(rng, np.array(rows, dtype=np.int64).reshape(-1, 2)), nb


def key_widths():
    """[(contact list, body_count, 8-bit sort passes)]: lists whose highest body index is body_count - 1, for the counts that need 1, 2, 3 and 4 key bytes."""
    out = []
    for body_count, passes in ((16, 1), (256, 2), (4096, 3), (65536, 4), (65537, 5)):
        rng = np.random.default_rng(body_count)
        top = body_count - 1
        some = rng.integers(0, body_count, size=(40, 2))
        rows = [(top, 0), (0, top), (top, top), (1, top), *map(tuple, some.tolist()), (top, 0), (top - 1, top)]
        out.append((_fill(rng, np.array(rows, dtype=np.int64)), body_count, passes))
    return out


def check_key_widths(cases):
    assert [p for _, _, p in cases[:4]] == [1, 2, 3, 4]
    for lst, body_count, passes in cases:
        assert int(lst["bodies"].max()) == body_count - 1
        assert HC.key_bytes(body_count) == passes, (body_count, HC.key_bytes(body_count), passes)
    assert HC.key_bytes(0) == 8 and HC.key_bytes(1) == 1 and HC.key_bytes(2) == 1 and HC.key_bytes(17) == 2


def pair_list(keys, seed, spare=0):
    """A pair list of exactly len(keys) records (+ `spare` capacity) with the given (lo, hi) keys, sorted, and a random payload."""
    rng = np.random.default_rng(seed)
    keys = sorted(set(keys))
    rec = np.zeros(len(keys) + spare, dtype=E.CONTACT_PAIR)
    raw = rng.integers(0, 256, size=(len(rec), 64), dtype=np.uint8)
    rec[:] = np.frombuffer(raw.tobytes(), dtype=E.CONTACT_PAIR)
    for k, (lo, hi) in enumerate(keys):
        rec["lo"][k], rec["hi"][k] = lo, hi
    return len(keys), rec, len(rec)


def event_cases():
    """{name: (prev, cur)}; check_event_cases() says what each is for."""
    base = [(0, 1), (0, 2), (0, 7), (1, 2), (1, 9), (2, 2), (2, 0xFFFFFFFF), (3, 4), (7, 8), (0xFFFFFFFE, 0xFFFFFFFF)]
    more = [(0, 0), (0, 3), (1, 3), (2, 3), (5, 6), (9, 9), (0xFFFFFFFF, 0xFFFFFFFF)]
    rng = np.random.default_rng(3)
    many = sorted({(int(a), int(a) + int(d)) for a, d in zip(rng.integers(0, 2000, size=3000), rng.integers(0, 4, size=3000))})
    return {
        "entries_only": (pair_list(base, 1), pair_list(base + more, 2)),
        "exits_only": (pair_list(base + more, 3), pair_list(base[2:], 4)),
        "both": (pair_list(base[:6] + more[:4], 5, spare=3), pair_list(base[3:] + more[2:], 6, spare=5)),
        "neither": (pair_list(base, 7), pair_list(base, 8)),
        "empty_prev": (pair_list([], 9, spare=2), pair_list(base, 10)),
        "empty_cur": (pair_list(more, 11), pair_list([], 12)),
        "many": (pair_list(many[::2] + many[1::3], 13), pair_list(many[1::2] + many[::5], 14)),
    }


def check_event_cases(cases):
    expect = {"entries_only": (True, False), "exits_only": (False, True), "both": (True, True), "neither": (False, False),
              "empty_prev": (True, False), "empty_cur": (False, True), "many": (True, True)}
    assert set(cases) == set(expect)
    for name, (prev, cur) in cases.items():
        (nb, _), (ne, _) = HC.events_np(prev, cur)
        assert (nb > 0, ne > 0) == expect[name], (name, nb, ne)
    assert cases["empty_prev"][0][0] == 0 and cases["empty_cur"][1][0] == 0
    prev, cur = cases["neither"]
    assert prev[1].tobytes() != cur[1].tobytes(), "`neither` must differ in its payload: only the keys decide"
    (nb, _), (ne, _) = HC.events_np(*cases["many"])
    assert nb > 256 and ne > 256, (nb, ne)
