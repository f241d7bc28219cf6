"""nh_recover on the GPU (pytest -m gpu): shapes that overlap the world pushed free of it in one call (include/nudge_hip.h, "nh_recover").

The oracle is the host's brute force (tests/hostoracle/hostrecover.cpp through tests/hostrecover_util.py): the state machine of nudge_amd/csrc/nh_query.h,
"recover" -- the functions the kernel runs -- around nh_overlap's predicates and nh_penetration's pair functions over every collider, so the kernel's 64
bytes per record must equal it bit for bit.  The identities of the header are tested against the GPU's own nh_overlap and nh_penetration: max_iterations
= 0, the REPLAY of the loop from the host, the free-at-position check, half height 0."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_util as F                      # noqa: E402
import hostquery_util as Q                   # noqa: E402
import hostrecover_util as HR                # noqa: E402
import recover_batches as RB                 # noqa: E402
from query_util import OBSERVED, SMALL, same_stepped_world as _same_stepped_world, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
FUSED = E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP
SENTINEL = 0xA5
PUSHED, OVERLAPPING, TOUCHING, INVALID = E.NH_RECOVER_PUSHED, E.NH_RECOVER_OVERLAPPING, E.NH_RECOVER_TOUCHING, E.NH_RECOVER_INVALID
STOPPED = OVERLAPPING | TOUCHING | INVALID


def _recover(w, m):
    raw = w.recover_records(_upload(w, m))
    return np.frombuffer(raw.cpu().numpy().tobytes(), dtype=E.RECOVER_RESULT).copy()


def _penetration(w, q):
    """(offsets, every nh_PenetrationHit record) of the GPU's nh_penetration: a count call, then an exactly sized list call."""
    import torch
    qt = _upload(w, q)
    off, _ = w.penetration_records(qt)
    total = int(off[len(q)].item()) & NONE
    assert total != NONE
    hits = torch.empty((max(total, 1), 32), dtype=torch.uint8, device=w.dev)
    if total:
        w.penetration_records(qt, offsets=off, hits=hits, capacity=total)
    return off.cpu().numpy().view(np.uint32).copy(), np.frombuffer(hits.cpu().numpy().tobytes(), dtype=E.PENETRATION_HIT)[:total].copy()


def _overlap_counts(w, q):
    off, _ = w.overlap_records(_upload(w, q))
    return np.diff(off.cpu().numpy().view(np.uint32).astype(np.int64))


def _same(got, ref, what):
    bad = (got.view(np.uint8).reshape(-1, 64) != ref.view(np.uint8).reshape(-1, 64)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(ref)} recover results differ, first at {int(np.argmax(bad))}: {got[np.argmax(bad)]} != {ref[np.argmax(bad)]}"


def _records(w, scene):
    return Q.records(w.get_bodies()["transforms"], scene, w.nbox, w.nsph)


def _check_world(w, scene, rng, n, what, **kw):
    """n records against the brute force; returns (the records, the GPU's results)."""
    rec = _records(w, scene)
    m = RB.recovers(rng, rec, w.nbox, n, **kw)
    got = _recover(w, m)
    _same(got, HR.recover(rec, w.nbox, m), what)
    return m, got


def _shares(got, what):
    once, twice, overlapping, free = RB.shares(got)
    print(f"{what}: iterations >= 1 {once:.3f}, >= 2 {twice:.3f}, OVERLAPPING {overlapping}, free without a push {free}")
    assert once >= RB.PUSHED_ONCE and twice >= RB.PUSHED_TWICE and overlapping >= 1 and free >= 1, (what, once, twice, overlapping, free)


# ---- bit for bit against the oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SMALL))
def test_recovers_equal_the_brute_force_before_and_after_stepping(name):
    scene = SMALL[name]()
    before, after = RB.SEEDS[name]
    w = E.World(scene, flags=FUSED)
    w.query_build()
    _, got = _check_world(w, scene, np.random.default_rng(before), 4096, f"{name} initial")
    _shares(got, f"{name} initial")
    w.step(50)
    # the refit of the tree built before the bodies moved, then a new build: the same bytes
    w.query_refit()
    m, refit = _check_world(w, scene, np.random.default_rng(after), 4096, f"{name} after 50 steps, refit")
    _shares(refit, f"{name} after 50 steps")
    w.query_build()
    _same(_recover(w, m), refit, f"{name} after 50 steps, built")
    w.close()


# ---- the smallest shapes at which the kernel can go wrong ------------------------------------------------------------------------------------------
def test_an_empty_world_and_a_world_of_one_collider():
    rng = np.random.default_rng(840)
    scene = S.pile(4, 0, seed=3)
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    rec = Q.records(scene["body_transforms"], scene)
    m = RB.recovers(rng, rec[:1], 1, 1024)
    w.set_counts(nb, 0, 0)                                     # no collider at all: nothing overlaps, nothing moves
    w.query_build()
    got = _recover(w, m)
    _same(got, HR.recover(rec[:0], 0, m), "an empty world")
    valid = got["flags"] != INVALID
    assert (got["flags"][valid] == 0).all() and got["position"].tobytes() == m["center"].tobytes() and (~valid).sum() >= 8
    assert all(r.tobytes() == HR.none_record().tobytes() for r in got["last"])
    w.set_counts(nb, 1, 0)                                     # the ground slab alone (body 0)
    w.query_build()
    rec = _records(w, scene)
    assert len(rec) == 1
    got = _recover(w, m)
    _same(got, HR.recover(rec, w.nbox, m), "one collider")
    # one convex collider: a push with a skin frees the shape at once, so nothing is pushed twice but by rounding
    skinned = valid & (m["skin"] > 0) & (m["max_iterations"] >= 1) & (m["ignore_body"] != 0)
    assert (got["iterations"] >= 1).mean() > 0.25 and (got["iterations"][skinned] <= 1).all() and (got["flags"][skinned] & STOPPED == 0).all()
    w.close()


def test_a_tree_of_more_than_one_leaf_run():
    scene = S.pile(1500, 300, seed=3)
    w = E.World(scene, flags=FUSED)
    w.query_build()
    assert w.nbox + w.nsph > 1024
    _, got = _check_world(w, scene, np.random.default_rng(841), 2048, "1801 colliders")
    _shares(got, "1801 colliders")
    w.close()


def test_counts_around_a_block_and_both_ends_of_max_iterations():
    scene = SMALL["stacks"]()
    w = E.World(scene, flags=FUSED)
    w.step(20)
    w.query_build()
    rec = _records(w, scene)
    m = RB.recovers(np.random.default_rng(842), rec, w.nbox, 257, invalid=False)
    for max_iterations in (0, 8):
        m["max_iterations"] = max_iterations
        ref = HR.recover(rec, w.nbox, m)
        for count in (1, 255, 256, 257):
            _same(_recover(w, m[:count]), ref[:count], f"count {count}, max_iterations {max_iterations}")
        if max_iterations == 0:
            assert (ref["iterations"] == 0).all() and ((ref["flags"] & OVERLAPPING) != 0).mean() > 0.25
        else:
            assert (ref["iterations"] >= 2).mean() > 0.02
    w.close()


# ---- the identities, against the GPU's own nh_overlap and nh_penetration ----------------------------------------------------------------------------
def _settled(name, steps, seed, n):
    scene = SMALL[name]()
    w = E.World(scene, flags=FUSED)
    w.step(steps)
    w.query_build()
    rec = _records(w, scene)
    return w, rec, RB.recovers(np.random.default_rng(seed), rec, w.nbox, n)


@pytest.mark.parametrize("name", ["pile", "compound"])
def test_max_iterations_zero_is_the_deepest_record_of_nh_penetration(name):
    w, rec, m = _settled(name, 20, 843, 4096)
    m["max_iterations"] = 0
    got = _recover(w, m)
    off, hits = _penetration(w, HR.queries(m))
    found, kept = HR.deepest(off, hits, len(m))
    valid = got["flags"] != INVALID
    assert got["last"][valid].tobytes() == kept[valid].tobytes()
    assert got["position"].tobytes() == m["center"].tobytes() and (got["iterations"] == 0).all() and not got["push"].any()
    assert np.isin(got["flags"][valid], (0, OVERLAPPING, TOUCHING)).all() and ((got["flags"] == 0) == (found == 0))[valid].all()
    # a query for which nh_overlap counts 0: flags 0 and the NONE record
    free = valid & (_overlap_counts(w, HR.queries(m)) == 0)
    assert free.sum() >= 16 and (got["flags"][free] == 0).all() and all(r.tobytes() == HR.none_record().tobytes() for r in got["last"][free])
    assert (np.diff(off.astype(np.int64))[valid] > 1).mean() > 0.1          # (segments of several records: the choice among them is tested)
    w.close()


def test_replay_from_the_host_gives_the_same_bytes():
    """The loop run from the host -- one GPU nh_penetration per round, nh_q_recover_advance (hr_advance) between them -- gives nh_recover's bytes."""
    w, rec, m = _settled("grid_tiles", 30, 844, 2048)
    got = _recover(w, m)
    st = HR.begin(m)
    last = np.full(len(m), HR.none_record(), dtype=E.PENETRATION_HIT)
    rounds = 0
    while (st["stopped"] == 0).any():
        assert rounds <= E.NH_RECOVER_MAX_ITERATIONS
        live = st["stopped"] == 0
        off, hits = _penetration(w, HR.queries(m, st["p"]))
        found, kept = HR.deepest(off, hits, len(m))
        take = live & (found != 0)
        last[take] = kept[take]
        HR.advance(m, st, found, kept)
        rounds += 1
    ref = np.zeros(len(m), dtype=E.RECOVER_RESULT)
    ref["position"], ref["flags"], ref["iterations"], ref["last"] = st["p"], st["flags"], st["iterations"], last
    ref["push"] = st["p"] - m["center"]
    bad = got["flags"] == INVALID
    ref["flags"][bad], ref["push"][bad] = INVALID, 0.0
    _same(got, ref, "replay")
    assert rounds >= 3 and RB.shares(got)[1] >= RB.PUSHED_TWICE
    w.close()


@pytest.mark.parametrize("name", ["stacks", "ball_pit"])
def test_a_result_that_did_not_stop_short_is_free_where_it_stands(name):
    w, rec, m = _settled(name, 30, 845, 4096)
    got = _recover(w, m)
    n = _overlap_counts(w, HR.queries(m, got["position"]))
    freed = (got["flags"] & STOPPED) == 0
    assert freed.mean() > 0.15 and (freed & (got["iterations"] >= 1)).mean() > 0.1 and (n[freed] == 0).all()
    stuck = (got["flags"] & (OVERLAPPING | TOUCHING)) != 0
    assert stuck.sum() >= 16 and (n[stuck] >= 1).all()
    w.close()


def test_half_height_zero_does_not_read_the_rotation():
    w, rec, m = _settled("grid_tiles", 20, 846, 4096)
    m = m[m["shape"] != E.NH_SHAPE_BOX]
    m = m[HR.recover(rec, w.nbox, m)["flags"] != INVALID]
    m["shape"], m["rotation"] = E.NH_SHAPE_CAPSULE, HR.IDENTITY
    m["size"][:, 1] = 0.0
    plain = _recover(w, m)
    _same(plain, HR.recover(rec, w.nbox, m), "capsules of half height 0")
    m["rotation"] = np.nan
    _same(_recover(w, m), plain, "capsules of half height 0 with NaN rotations")
    # ... and they are the sphere queries' bytes
    m["shape"], m["size"][:, 1:] = E.NH_SHAPE_SPHERE, np.nan
    _same(_recover(w, m), plain, "the sphere queries")
    assert (plain["flags"] & INVALID == 0).all() and RB.shares(plain)[0] >= RB.PUSHED_ONCE
    w.close()


# ---- layer masks ----------------------------------------------------------------------------------------------------------------------------
def test_recovers_under_layer_masks_equal_the_brute_force_over_the_masked_world():
    scene = SMALL["pile"]()
    w = E.World(scene, flags=FUSED)
    w.step(40)
    w.query_build()
    rec = _records(w, scene)
    layer_seed, batch_seed = F.SEEDS["pile"]
    words = F.layers(len(rec), layer_seed)
    w.query_set_layers(words[:w.nbox], words[w.nbox:])
    m = RB.recovers(np.random.default_rng(batch_seed), rec, w.nbox, 4096)
    off = _recover(w, m)
    _same(off, HR.recover(rec, w.nbox, m), "filter off")
    valid = off["flags"] != INVALID
    # uniform masks: the brute force over the masked world (a NaN position wherever the mask sees nothing of the collider's word)
    refs = {}
    for mask in (1, 2, 6, 0xFFFFFFFF):
        w.query_filter(mask)
        refs[mask] = HR.recover(F.masked(rec, words, mask), w.nbox, m)
        _same(_recover(w, m), refs[mask], f"uniform mask {mask:#x}")
        # (the filter changes answers: masks 1, 2 and 6 hide half or a quarter of the colliders, all ones the sixteenth whose word is 0)
        changed = (refs[mask].view(np.uint8).reshape(-1, 64) != off.view(np.uint8).reshape(-1, 64)).any(axis=1).mean()
        assert changed > (0.05 if mask != 0xFFFFFFFF else 0.0), (mask, changed)
        assert (refs[mask]["iterations"] >= 1).mean() > 0.1, mask
    # mask 0 sees nothing: flags 0 and the position untouched
    w.query_filter(0)
    got = _recover(w, m)
    _same(got, HR.recover(F.masked(rec, words, 0), w.nbox, m), "mask 0")
    assert (got["flags"][valid] == 0).all() and got["position"].tobytes() == m["center"].tobytes() and not got["push"].any()
    # per-query masks, alternating within every wave
    masks = np.where(np.arange(len(m)) % 2 == 0, 1, 6).astype(np.uint32)
    w.query_filter(_upload(w, masks).view(w.torch.int32))
    ref = refs[1].copy()
    ref[1::2] = refs[6][1::2]
    _same(_recover(w, m), ref, "per-query masks")
    w.query_filter(None)
    _same(_recover(w, m), off, "filter off again")
    w.close()


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_abi_edge_cases():
    import torch
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    L = w.L
    rec0 = Q.records(scene["body_transforms"], scene)
    m = RB.recovers(np.random.default_rng(847), rec0, len(scene["box_tags"]), 1024)
    t = _upload(w, m)
    out = torch.full((1024 + 1, 64), SENTINEL, dtype=torch.uint8, device=w.dev)
    ptr = lambda x, byte=0: C.c_void_p(x.data_ptr() + byte)               # noqa: E731
    assert L.nh_recover(w.ctx, ptr(t), 1024, ptr(out), 0) == 1             # before any build: NH_ERR_INVALID
    assert L.nh_recover(None, ptr(t), 1024, ptr(out), 0) == 1
    w.query_build()
    assert L.nh_recover(w.ctx, ptr(t), 1024, ptr(out), 1) == 1             # flags != 0
    assert L.nh_recover(w.ctx, ptr(t), 1024, ptr(out), 0x80000000) == 1
    assert L.nh_recover(w.ctx, ptr(t), 1 << 30, ptr(out), 0) == 1          # count >= 2^30
    assert L.nh_recover(w.ctx, ptr(t), 0xFFFFFFFF, ptr(out), 0) == 1
    assert L.nh_recover(w.ctx, None, 1024, ptr(out), 0) == 1               # null
    assert L.nh_recover(w.ctx, ptr(t), 1024, None, 0) == 1
    for byte in (4, 8):                                                    # not 16-byte aligned
        assert L.nh_recover(w.ctx, ptr(t, byte), 1023, ptr(out), 0) == 1
        assert L.nh_recover(w.ctx, ptr(t), 1023, ptr(out, byte), 0) == 1
    assert L.nh_recover(w.ctx, ptr(t), 0, ptr(out), 0) == 0                # count = 0: a no-op
    assert L.nh_recover(w.ctx, None, 0, None, 0) == 0
    assert L.nh_recover(w.ctx, ptr(t), 0, ptr(out), 4) == 1                # (the flags are checked first, as in nh_move)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                   # a refused call writes nothing, and neither does count = 0

    # every byte of `count` results and nothing behind them; two calls, the same bytes
    rec = _records(w, scene)
    assert L.nh_recover(w.ctx, ptr(t), 1000, ptr(out), 0) == 0
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert (raw[1000:] == SENTINEL).all()
    got = np.frombuffer(raw[:1000].tobytes(), dtype=E.RECOVER_RESULT)
    _same(got, HR.recover(rec, w.nbox, m[:1000]), "1000 of 1024 records")
    bad = got["flags"] == INVALID
    assert bad.sum() >= 8 and got["position"][bad].tobytes() == m["center"][:1000][bad].tobytes() and not got["push"][bad].any()
    again = torch.full((1000, 64), 0x5A, dtype=torch.uint8, device=w.dev)
    assert L.nh_recover(w.ctx, ptr(t), 1000, ptr(again), 0) == 0
    torch.cuda.synchronize()
    assert again.cpu().numpy().tobytes() == raw[:1000].tobytes()
    # the Python front end packs the same records
    good = np.nonzero(~bad)[0]
    for shape, kw in ((E.NH_SHAPE_SPHERE, lambda r: dict(radii=r["size"][:, 0])),
                      (E.NH_SHAPE_BOX, lambda r: dict(half_extents=r["size"], rotations=r["rotation"])),
                      (E.NH_SHAPE_CAPSULE, lambda r: dict(radii=r["size"][:, 0], half_heights=r["size"][:, 1], rotations=np.nan_to_num(r["rotation"])))):
        k = good[m["shape"][good] == shape][:128]
        r = m[k]
        py = w.recover(r["center"], skin=r["skin"], max_iterations=r["max_iterations"].astype(np.int64), ignore_body=r["ignore_body"].astype(np.int64),
                       synchronize=True, **kw(r))
        res = np.frombuffer(py["raw"].cpu().numpy().tobytes(), dtype=E.RECOVER_RESULT)
        assert len(k) >= 64 and res.tobytes() == got[k].tobytes(), shape
        assert np.array_equal(py["iterations"].cpu().numpy(), got["iterations"][k]) and np.array_equal(py["flags"].cpu().numpy(), got["flags"][k])
        assert py["position"].cpu().numpy().tobytes() == got["position"][k].tobytes() and py["push"].cpu().numpy().tobytes() == got["push"][k].tobytes()
        assert np.array_equal(py["last"]["shape"].cpu().numpy(), got["last"]["shape"][k]) and py["last"]["depth"].cpu().numpy().tobytes() == got["last"]["depth"][k].tobytes()
    w.close()


# ---- observers -----------------------------------------------------------------------------------------------------------------------------
def test_recovers_between_the_sub_steps_of_a_stepped_world_change_nothing():
    # (the observer tests' pile, boxes only, as in tests/test_gpu_move.py)
    scene = OBSERVED["pile"]()
    rec0 = Q.records(scene["body_transforms"], scene)
    m = RB.recovers(np.random.default_rng(848), rec0, len(scene["box_tags"]), 4096)

    def call(w, mt, rt):
        w.query_build()
        w.recover_records(mt, results=rt)

    # between nh_step calls
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    mt, rt = _upload(a, m), a.torch.empty((4096, 64), dtype=a.torch.uint8, device=a.dev)
    done = 0
    for k in [1, 2, 3, 5, 7, 4, 8] * 4:
        k = min(k, 100 - done)
        if k <= 0:
            break
        call(a, mt, rt)
        a.step(k)
        b.step(k)
        done += k
    call(a, mt, rt)
    assert done == 100
    _same_stepped_world(a, b, "pile, recovers between nh_step calls")
    res = np.frombuffer(rt.cpu().numpy().tobytes(), dtype=E.RECOVER_RESULT)
    assert (res["iterations"] >= 1).mean() > 0.1                            # the recovers did find something
    a.close(); b.close()
    # between every call of the fused step
    a, b = E.World(scene, flags=FUSED), E.World(scene, flags=FUSED)
    mt, rt = _upload(a, m), a.torch.empty((4096, 64), dtype=a.torch.uint8, device=a.dev)
    for s in range(60):
        for name in ("collide", "gravity", "read_cache", "setup", "apply", "update", "write_cache", "advance"):
            call(a, mt, rt)
            getattr(a, name)()
            getattr(b, name)()
        a.step_done(); b.step_done()
    call(a, mt, rt)
    _same_stepped_world(a, b, "pile, recovers call by call")
    a.close(); b.close()


# ---- end to end with nh_move ---------------------------------------------------------------------------------------------------------------------
def test_a_sunk_capsule_is_recovered_and_then_moves():
    scene = S.pile(4, 0, seed=3)
    w = E.World(scene, flags=FUSED)
    w.set_counts(len(scene["body_transforms"]), 1, 0)          # the ground slab alone (body 0)
    w.query_build()
    rec = _records(w, scene)
    top = float(rec["p"][0, 1] + rec["h"][0, 1])
    r, hh, skin = 0.4, 0.5, 0.01
    start = np.float32([[rec["p"][0, 0] + 1.0, top + r + hh - 0.2, rec["p"][0, 2] - 2.0]])      # sunk 0.2 into the slab
    step = np.float32([[1.0, 0.0, 0.5]])
    stuck = w.move(start, step, r, hh, skin=skin, synchronize=True)
    assert int(stuck["flags"][0]) == E.NH_MOVE_START_OVERLAP and stuck["position"].cpu().numpy().tobytes() == start.tobytes()
    out = w.recover(start, radii=r, half_heights=hh, skin=skin, synchronize=True)
    pos = out["position"].cpu().numpy()
    assert int(out["flags"][0]) == PUSHED and int(out["iterations"][0]) == 1
    assert abs(pos[0, 1] - (top + r + hh + skin)) <= 7.5e-6 * max(1.0, abs(top)) and pos[0, 0] == start[0, 0] and pos[0, 2] == start[0, 2]
    assert out["last"]["normal"].cpu().numpy().tolist() == [[0.0, 1.0, 0.0]] and int(out["last"]["collider"][0]) == 0
    q = HR.queries(HR.recovers(pos, radii=r, half_heights=hh))
    assert _overlap_counts(w, q)[0] == 0
    moved = w.move(pos, step, r, hh, skin=skin, synchronize=True)
    assert int(moved["flags"][0]) & E.NH_MOVE_START_OVERLAP == 0 and int(moved["flags"][0]) & E.NH_MOVE_INVALID == 0
    end = moved["position"].cpu().numpy()
    assert np.linalg.norm(end - pos) >= 0.9 * np.linalg.norm(step) and abs(end[0, 1] - pos[0, 1]) <= 2 * skin
    w.close()
