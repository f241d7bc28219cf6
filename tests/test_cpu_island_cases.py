"""The crafted island, sleeping and cache worlds of tests/island_cases_util.py without a GPU: that the worlds are what they claim to be (the graph worlds' pairs and
contacts, known by construction, against the brute-force host build; the geometry worlds' designated near misses and touching pairs), that the numpy oracle -- a full union
over every edge -- equals the compiled reference on every world, phase and crafted cache the reference can hold, exactly, and that uniting only the edges with a sleeping
end (what the kernels do: the comment above emit_pair in nh_collide.hip) gives the same lists as the full union on every world, the two large instances included.  That is
what lets tests/test_gpu_island_cases.py use the oracle beyond the reference's 8192 colliders."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import island_cases_util as U               # noqa: E402
import hostsim_util as H                    # noqa: E402
import parity_util as P                     # noqa: E402
from nudge_amd import scenes as S           # noqa: E402
from oracle import refworld                 # noqa: E402

needs_ref = pytest.mark.skipif(not refworld.available("exact"), reason="oracle/_ref not built (needs the reference sources: make -C oracle)")


def _pair_set(prs):
    return {tuple(sorted(p)) for p in np.asarray(prs).tolist()}


def _contact_pairs(keys):
    keys = np.asarray(keys, dtype=np.uint64)
    a, c = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), (keys >> np.uint64(32)).astype(np.int64)
    return {(min(x, y), max(x, y)) for x, y in zip(a.tolist(), c.tolist())}


@pytest.mark.parametrize("case", U.CASES)
def test_island_worlds_are_well_formed(case):
    scene = U.world(case)
    isl = scene["isl"]
    C, nb = U.ncolliders(scene), len(scene["body_transforms"])
    assert np.array_equal(np.concatenate([scene["box_tags"], scene["sphere_tags"]]), np.arange(C)), case
    assert C <= U.REF_LIMIT and S.narrow_ok(scene), case
    assert not scene["body_momentum"].view(np.float32).any(), case
    own = U.owners(scene)
    assert np.array_equal(np.unique(own[own != 0]), np.arange(1, nb)), case
    con = scene["connections"]
    assert con.dtype == np.uint32 and con.max(initial=0) < nb, case
    for ph in isl["phases"]:
        assert ph["idle"].dtype == np.uint8 and len(ph["idle"]) == nb, case
    prs = H.pairs(scene["body_transforms"], scene)
    h = H.collide(scene["body_transforms"], scene, cap=1 << 16)
    if isl["kind"] == "graph":
        # exactly the N slab pairs and one contact per sphere: what graph_lists states by construction (the same builder makes the two large instances)
        n = isl["n"]
        pairs, contacts = U.graph_lists(scene)
        assert n == U.N_DEFAULT and np.array_equal(prs.astype(np.int64), pairs), case
        assert h["count"] == n and np.array_equal(h["keys"], contacts["keys"]) and np.array_equal(h["features"], contacts["features"]), case
        assert np.array_equal(h["bodies"], contacts["bodies"]), case
        assert (h["data"]["penetration"] == np.float32(U.PUSH)).all(), case
    else:
        have, made = _pair_set(prs), _contact_pairs(h["keys"])
        for p in isl["near"]:
            assert p in have and p not in made, (case, "near miss", p)
        for p in isl["touch"] + isl["asleep_touch"]:
            assert p in have and p in made, (case, "touching", p)
        assert len(have - made) >= len(isl["near"])
        if len(h["keys"]):
            assert int(h["keys"].min()) >= 1 << 32, case          # (no key with a zero high word: crafted_caches' foreign entries sit below every live one)
    # what the case states in words, against the oracle
    for ph in isl["phases"]:
        o = U.expected(scene, ph)
        e = ph["expect"]
        for name, got in (("active", len(o["active"])), ("contacts", len(o["tags"])), ("sleeping", len(o["sleeping"])), ("fine", len(o["fine_sleeping"]))):
            if name in e:
                assert got == e[name], (case, ph["name"], name, got, e[name])
    if case == "sleeping_heap":
        assert len(o["sleeping"]) == len(prs) and (o["sleeping"] & np.uint64(0xFFFFFFFF) > o["sleeping"] >> np.uint64(32)).all()
    if case == "far_connection":
        kinds = {(a >= len(scene["box_tags"]), b >= len(scene["box_tags"])) for a, b in _contact_pairs(o["tags"])}
        assert len(kinds) == 3 and len(o["tags"]) == h["count"]          # (box-box, box-sphere and sphere-sphere contacts, all of them alive)


@pytest.mark.parametrize("case,n", [(c, None) for c in U.CASES] + sorted(U.LARGE.items()))
def test_full_union_and_sleeping_end_union_agree(case, n):
    """The comment above emit_pair, checked: an edge between two awake bodies cannot change which sets are active."""
    scene = U.world(case, n)
    pairs, contacts = U.lists(scene)
    for ph in scene["isl"]["phases"]:
        full, short = U.expected(scene, ph, pairs, contacts), U.expected(scene, ph, pairs, contacts, sleeping_end_only=True)
        for k in ("active", "tags", "features", "bodies", "sleeping", "coarse_sleeping", "fine_sleeping"):
            assert np.array_equal(full[k], short[k]), (case, ph["name"], k)
        if n is not None:          # (the large instances state their counts like the small ones)
            for name, got in (("active", len(full["active"])), ("contacts", len(full["tags"])), ("sleeping", len(full["sleeping"]))):
                assert got == ph["expect"][name], (case, n, name)
    if n is not None:
        U.forget(case, n)
    if case == "awake_bridges":
        # the two unions build different sets here
        con = scene["connections"].astype(np.int64)
        idle = scene["isl"]["phases"][0]["idle"]
        both_awake = (idle[con[:, 0]] != 0xff) & (idle[con[:, 1]] != 0xff)
        assert both_awake.any()
        assert not np.array_equal(U.components(len(idle), con[:, 0], con[:, 1]), U.components(len(idle), con[~both_awake, 0], con[~both_awake, 1]))


def _ref_lists(w):
    rc = w.contacts()
    od, ob, ok, of, _ = P.oracle_contacts_sorted(rc)
    return dict(active=w.active().astype(np.uint32), tags=ok, features=of, bodies=ob, data=od, sleeping=P.widen_sleeping(rc["sleeping_pairs"]))


@needs_ref
@pytest.mark.parametrize("case", U.CASES)
def test_oracle_matches_reference_on_island_worlds(case):
    scene = U.world(case)
    pairs, contacts = U.lists(scene)
    w = refworld.RefWorld(scene)
    seen = 0
    for ph in scene["isl"]["phases"]:
        w.set_bodies(idle=ph["idle"])
        w.collide()
        r, o = _ref_lists(w), U.expected(scene, ph, pairs, contacts)
        where = (case, ph["name"])
        assert np.array_equal(r["active"], o["active"]), where
        assert len(r["tags"]) == len(o["tags"]) and np.array_equal(r["tags"], o["tags"]) and np.array_equal(r["features"], o["features"]), where
        assert np.array_equal(r["bodies"], o["bodies"]), where
        if "data" in o:
            assert P.bits_equal(r["data"], o["data"]), where
        assert np.array_equal(r["sleeping"], o["sleeping"]), where
        assert np.array_equal(w.bodies()["idle"], ph["idle"]), where          # (collide leaves the counters alone)
        seen += len(o["sleeping"]) + len(o["active"])
    assert seen > 0


def _ref_with_cache(scene, cache, max_contacts):
    w = refworld.RefWorld(scene, max_contacts=max_contacts)
    w.restore(dict(bodies=dict(transforms=scene["body_transforms"], momentum=scene["body_momentum"], idle=scene["isl"]["phases"][0]["idle"]),
                   cache_count=cache["count"], cache_tags=U.narrow_cache(cache), cache_data=cache["data"]))
    return w


@needs_ref
@pytest.mark.parametrize("case", U.CACHE_WORLDS)
def test_cache_oracle_matches_reference(case):
    """Every crafted cache through the reference's read_cached_impulses / write_cached_impulses: the cache after collide -> read -> write, the looked-up impulses, and the cache
    after the zero-iteration solve (collide -> read -> setup -> apply(0) -> update -> write) against the numpy model, bit for bit.  (Zero iterations: the solver hands the
    contacts' impulses back after its own clamping, which is no business of the model: for the solve the model is asked for count, tags, features and the payload of the
    entries kept aside; the contacts' payload after a solve is compared between library and reference in the GPU test.)"""
    scene = U.world(case)
    ph = scene["isl"]["phases"][0]
    o = U.expected(scene, ph)
    K = max(4096, 8 * len(scene["body_transforms"]))
    caches = U.crafted_caches(scene, o, K)
    assert sorted(caches) == sorted(U.CACHES)
    culled_total = 0
    for name in U.CACHES:
        cache = caches[name]
        m = U.cache_stages(cache, o, o["sleeping"])
        culled_total += int(m["culled"].sum())
        for solve in (False, True):
            where = (case, name, "solve" if solve else "read-write")
            w = _ref_with_cache(scene, cache, K)
            w.collide()
            r = _ref_lists(w)
            assert np.array_equal(r["tags"], o["tags"]) and np.array_equal(r["sleeping"], o["sleeping"]), where
            w.read_cache()
            if not solve:
                # the reference's contacts are in its own order; the model's in tag order
                order = P.oracle_contacts_sorted(w.contacts())[4]
                assert P.bits_equal(w.contact_impulses()[order], m["lookup"]), where
            else:
                w.setup(); w.apply(0); w.update()
            w.write_cache()
            rk = w.cache()
            wt, wf = U.widen_cache(rk)
            assert rk["count"] == m["write"]["count"], where + (rk["count"], m["write"]["count"])
            assert np.array_equal(wt, m["write"]["tags"]) and np.array_equal(wf, m["write"]["features"]), where
            if not solve:
                assert P.bits_equal(rk["data"], m["write"]["data"]), where
            else:
                from_cull = np.isin(wt, o["sleeping"])
                assert P.bits_equal(rk["data"][from_cull], m["write"]["data"][from_cull]), where
    if case != "far_connection":
        assert culled_total > 0, case          # (sleepers and sleepers_quirk hold entries that are kept aside)


@needs_ref
def test_tie_script_culled_entry_precedes_appended_contact_in_the_reference():
    """island_cases_util.tie_script through the reference: count, tags and features are the model's merge, the FIRST entry of each pair of equal keys is the cache's own
    (kept aside, verbatim), the second the contact's -- which the zero-iteration solve has changed, or the order could not be seen."""
    scene = U.world("near_miss_chain")
    o = U.expected(scene, scene["isl"]["phases"][0])
    extra, cache = U.tie_script(scene, o)
    m = U.cache_stages(cache, extra, o["sleeping"])
    assert int(m["culled"].sum()) == cache["count"] and m["write"]["count"] == cache["count"] + 3
    w = _ref_with_cache(scene, cache, 4096)
    w.collide()
    assert w.contacts()["count"] == 0
    w.append_contacts(extra["data"], extra["bodies"], H.narrow_tags(extra["tags"], extra["features"]))
    w.read_cache(); w.setup(); w.apply(0); w.update(); w.write_cache()
    rk = w.cache()
    wt, wf = U.widen_cache(rk)
    assert rk["count"] == m["write"]["count"] and np.array_equal(wt, m["write"]["tags"]) and np.array_equal(wf, m["write"]["features"])
    ties = 0
    for i in range(rk["count"] - 1):
        if wt[i] == wt[i + 1] and wf[i] == wf[i + 1]:
            ties += 1
            assert P.bits_equal(rk["data"][i], m["write"]["data"][i]) and not P.bits_equal(rk["data"][i + 1]["impulse"], m["write"]["data"][i + 1]["impulse"]), i
    assert ties == 3
