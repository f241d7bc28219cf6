"""nh_query_refit on the host (no GPU): the symbol through the header, the Python list and the built library; and a numpy model of the cut the box
pass makes (nudge_amd/csrc/nh_query_build.hip: k_q_boxes_runs / k_q_boxes_top) -- the Karras tree of seeded key sets built on the host, every internal node
classified by nh_q_run_crossing itself (nudge_amd/csrc/nh_query.h, built for the host by tests/hostrefit_util.py), and the two phases replayed with
the kernels' slots, sides and arrival counters against a plain refit of the whole tree."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostrefit_util as R                   # noqa: E402
from nudge_amd import engine as E           # noqa: E402

NONE = 0xFFFFFFFF
RUN = R.run()


def test_the_symbol_is_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "nudge_hip.h")).read()
    assert re.search(r"^int nh_query_refit\(nh_context\* ctx, const nh_BodyData\* bodies, const nh_ColliderData\* colliders\);", header, re.M)
    assert "an incremental refit" not in header
    assert "nh_query_refit" in E.EXPORTS
    so = os.path.join(ROOT, "nudge_amd", "libnudge_hip.so")
    exported = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert re.search(r" T nh_query_refit$", exported, re.M) and re.search(r" T nh_query_build$", exported, re.M)
    assert hasattr(E.World, "query_refit")


def test_the_parent_word():
    top, right, ident = (int(getattr(R.lib(), "hr_parent_" + k)()) for k in ("top", "right", "id"))
    assert top | right | ident == NONE and top & right == 0 and (top | right) & ident == 0
    assert ident + 1 >= 1 << 30                      # every internal node of the largest world (< 2^30 colliders) fits
    assert NONE & top                                # the root's parent word reads as "top": the bottom phase stops there
    for p in (0, 1, 12345, ident):
        for r in (0, 1):
            for t in (0, 1):
                w = R.parent_word(p, r, t)
                assert (w & ident, bool(w & right), bool(w & top)) == (p, bool(r), bool(t))


# ---- the Karras tree on the host (k_q_tree's arithmetic) ------------------------------------------------------------------------------------
def _tree(keys):
    """(left, right, first, last, parent) of the radix tree over sorted 64-bit `keys`, ties extended by the position: node ids as in the library
    (internal 0 .. n-2, leaf j = n-1+j)."""
    n = len(keys)
    keys = [int(k) for k in keys]

    def delta(i, j):
        if j < 0 or j >= n:
            return -1
        x = keys[i] ^ keys[j]
        if x == 0:
            return 64 + (32 - (i ^ j).bit_length())
        return 64 - x.bit_length()

    left, right = np.zeros(max(n - 1, 0), np.int64), np.zeros(max(n - 1, 0), np.int64)
    first, last = np.zeros(max(n - 1, 0), np.int64), np.zeros(max(n - 1, 0), np.int64)
    parent = np.full(2 * n - 1, -1, np.int64)
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) > delta(i, i - 1) else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax *= 2
        l, t = 0, lmax // 2
        while t >= 1:
            if delta(i, i + (l + t) * d) > dmin:
                l += t
            t //= 2
        j = i + l * d
        dnode = delta(i, j)
        s, t = 0, l
        while True:
            t = (t + 1) // 2
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t <= 1:
                break
        gamma = i + s * d + (-1 if d < 0 else 0)
        first[i], last[i] = min(i, j), max(i, j)
        left[i] = n - 1 + gamma if first[i] == gamma else gamma
        right[i] = n - 1 + gamma + 1 if last[i] == gamma + 1 else gamma + 1
        parent[left[i]] = parent[right[i]] = i
    return left, right, first, last, parent


def _key_sets():
    rng = np.random.default_rng(2024)
    for n in (1, 2, 3, RUN - 1, RUN, RUN + 1, 4097):
        yield f"random {n}", np.sort(rng.integers(0, 1 << 48, size=n, dtype=np.uint64))
        yield f"equal {n}", np.full(n, 0x123456789ab, dtype=np.uint64)
        yield f"few distinct {n}", np.sort(rng.integers(0, 7, size=n).astype(np.uint64) << np.uint64(40))


@pytest.mark.parametrize("what,keys", list(_key_sets()), ids=[w for w, _ in _key_sets()])
def test_the_cut_of_the_tree_by_leaf_runs(what, keys):
    n = len(keys)
    left, right, first, last, parent = _tree(keys)
    rng = np.random.default_rng(n)
    lo = rng.uniform(-100, 100, size=(n, 3)).astype(np.float32)
    hi = lo + rng.uniform(0, 5, size=(n, 3)).astype(np.float32)
    nan = rng.random(n) < 0.02                                   # colliders of bodies that do not exist: NaN leaves
    lo[nan] = hi[nan] = np.nan
    box_lo, box_hi = np.full((2 * n - 1, 3), 7.0, np.float32), np.full((2 * n - 1, 3), 7.0, np.float32)

    # the plain refit: children before parents, by ascending range length
    ref_lo, ref_hi = box_lo.copy(), box_hi.copy()
    ref_lo[n - 1:], ref_hi[n - 1:] = lo, hi
    for u in np.argsort(last - first, kind="stable"):
        ref_lo[u] = np.fmin(ref_lo[left[u]], ref_lo[right[u]])
        ref_hi[u] = np.fmax(ref_hi[left[u]], ref_hi[right[u]])
    if n > 1:
        assert first[0] == 0 and last[0] == n - 1 and parent[0] == -1 and (parent[1:] >= 0).all()

    # every node is inside one run or crossing, never both; the ranges contain the node's own index, at one end
    crossing = np.array([R.crossing(first[u], last[u]) for u in range(n - 1)], dtype=bool)
    assert np.array_equal(crossing, first // RUN != last // RUN)
    for u in range(n - 1):
        assert u in (first[u], last[u])
        if not crossing[u]:
            run = u // RUN
            assert first[u] // RUN == run == last[u] // RUN               # its index lies in its run: index - run start is its slot
            for c in (left[u], right[u]):                                # children: inside nodes or leaves of the same run
                if c >= n - 1:
                    assert (c - (n - 1)) // RUN == run
                else:
                    assert not crossing[c] and c // RUN == run
        # the side bit of the parent word: the left child of a split has the split's index, the right child the next
        li, ri = (left[u] - (n - 1) if left[u] >= n - 1 else left[u]), (right[u] - (n - 1) if right[u] >= n - 1 else right[u])
        assert ri == li + 1
    if n <= RUN:
        assert not crossing.any()

    # the parent words as k_q_tree writes them
    word = np.full(2 * n - 1, NONE, np.int64)
    for u in range(n - 1):
        word[left[u]] = R.parent_word(u, False, crossing[u])
        word[right[u]] = R.parent_word(u, True, crossing[u])
    TOP, RIGHT, ID = (int(getattr(R.lib(), "hr_parent_" + k)()) for k in ("top", "right", "id"))

    # bottom phase, run by run: lanes in a random order, slots and arrival counters as in k_q_boxes_runs
    entries = []
    for base in range(0, n, RUN):
        child = np.zeros((RUN, 2, 6), np.float32)
        arrived = np.zeros(RUN, np.int64)
        for j in rng.permutation(np.arange(base, min(base + RUN, n))):
            box_lo[n - 1 + j], box_hi[n - 1 + j] = lo[j], hi[j]
            b = np.concatenate([lo[j], hi[j]])
            pw, me = int(word[n - 1 + j]), n - 1 + j
            while not pw & TOP:
                slot, side = (pw & ID) - base, 1 if pw & RIGHT else 0
                assert 0 <= slot < RUN
                child[slot, side] = b
                arrived[slot] += 1
                if arrived[slot] == 1:
                    me = -1
                    break
                o = child[slot, side ^ 1]
                b = np.concatenate([np.fmin(b[:3], o[:3]), np.fmax(b[3:], o[3:])])
                me = pw & ID
                pw = int(word[me])
            if me >= 0 and pw != NONE:
                entries.append(me)                                   # finished below, parent on top: k_q_tree lists it for the top phase
        assert set(np.unique(arrived)) <= {0, 2}
        for s in np.nonzero(arrived == 2)[0]:
            assert not crossing[base + s]
            box_lo[base + s] = np.fmin(child[s, 0, :3], child[s, 1, :3])
            box_hi[base + s] = np.fmax(child[s, 0, 3:], child[s, 1, 3:])
    inside = np.nonzero(~crossing)[0]
    assert box_lo[inside].tobytes() == ref_lo[inside].tobytes() and box_hi[inside].tobytes() == ref_hi[inside].tobytes()
    assert box_lo[n - 1:].tobytes() == ref_lo[n - 1:].tobytes()

    # the entry list k_q_tree makes: the children of crossing nodes that are not crossing themselves -- one more than there are crossing nodes
    listed = [c for u in np.nonzero(crossing)[0] for c in (left[u], right[u]) if c >= n - 1 or not crossing[c]]
    assert sorted(listed) == sorted(entries) and len(entries) == (int(crossing.sum()) + 1 if crossing.any() else 0)

    # top phase: from the entries, with a counter per node (k_q_boxes_top), in a random order
    arrive = np.zeros(max(n - 1, 0), np.int64)
    height_of = {}
    for me in rng.permutation(np.array(entries, dtype=np.int64)):
        me = int(me)
        b_lo, b_hi, height = box_lo[me].copy(), box_hi[me].copy(), 0
        pw = int(word[me])
        while pw != NONE:
            u = pw & ID
            assert crossing[u]
            arrive[u] += 1
            if arrive[u] == 1:
                height_of[u] = height
                break
            arrive[u] = 0
            height = max(height, height_of[u]) + 1
            other = left[u] if pw & RIGHT else right[u]
            b_lo, b_hi = np.fmin(b_lo, box_lo[other]), np.fmax(b_hi, box_hi[other])
            box_lo[u], box_hi[u] = b_lo, b_hi
            pw = int(word[u])
        if pw == NONE and crossing.any():
            assert u == 0 and 1 <= height <= int(crossing.sum())
    assert not arrive.any()                                          # the counters are left at 0 for the next pass
    assert box_lo.tobytes() == ref_lo.tobytes() and box_hi.tobytes() == ref_hi.tobytes()
