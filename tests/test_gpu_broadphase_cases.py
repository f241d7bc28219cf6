"""The crafted broadphase worlds of tests/broadphase_cases_util.py on the GPU, against brute force: the host build's O(n^2) collide and pair list (tests/hostsim,
proven equal to the compiled reference on these very worlds by tests/test_cpu_broadphase_cases.py), the reference itself for active bodies and sleeping pairs, and
for the one world too large for either a pair list known by construction.  Every world runs as three E.World's -- default, option no_incremental (a leaver costs a
rebuild), option no_kept_pairs (DIRECT search at every call); grid worlds leave no_incremental out -- and after every phase's collide() each of them must show the
oracle's contacts bit for bit, no error, the oracle's number of overlapping pairs, and, in the default world, exactly the path through the broadphase the script
states: the deltas of broadphase_rebuilds and broadphase_inserts (and large_colliders where stated).  That path check is what keeps a phase from passing
without reaching its branch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import broadphase_cases_util as U          # noqa: E402
import hostsim_util as H                    # noqa: E402
import parity_util as P                     # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from oracle import refworld                 # noqa: E402

pytestmark = pytest.mark.gpu
FLAGS = E.NH_FLAG_SYNC_COUNTS


def _world(scene, env=None):
    if env:
        os.environ[env] = "1"
    try:
        return E.World(scene, flags=FLAGS, **scene["bp"]["world"])
    finally:
        if env:
            os.environ.pop(env, None)


def _contact_pairs(tags):
    tags = np.asarray(tags, dtype=np.uint64)
    a, c = (tags & np.uint64(0xFFFFFFFF)).astype(np.int64), (tags >> np.uint64(32)).astype(np.int64)
    return {(min(x, y), max(x, y)) for x, y in zip(a.tolist(), c.tolist())}


class _Oracle:
    """What every world must show after a phase: computed once per distinct placement, shared by the three worlds."""

    def __init__(self, scene):
        self.scene, self.kind = scene, scene["bp"]["oracle"]
        self.cache, self.ref, self.ref_edits = {}, None, -1
        self.use_ref = refworld.available("exact") and U.ncolliders(scene) <= U.REF_LIMIT
        if self.kind == "ref_only":
            assert self.use_ref, "oracle/_ref/libnudge_ref_exact.so did not travel to this box: sleeper_edge has no other oracle"
        self.nbox = len(scene["box_tags"])

    def at(self, k):
        scene = self.scene
        ph = scene["bp"]["phases"][k]
        n_edits = sum(len(p["edits"]) for p in scene["bp"]["phases"][:k + 1])
        key = (ph["transforms"].tobytes(), n_edits)
        if key in self.cache:
            return self.cache[key]
        sc = U.scene_at(scene, k)
        o = {}
        if self.kind == "list":
            # (the O(n^2) oracle is too slow at this size: the pairs are known by construction; the contacts are compared with the no_kept_pairs world's)
            o["pairs"] = len(scene["bp"]["known_pairs"]); o["sphere_pairs"] = 0; o["pair_set"] = set(scene["bp"]["known_pairs"])
        else:
            prs = H.pairs(ph["transforms"], sc)
            o["pairs"] = len(prs); o["sphere_pairs"] = int(((prs[:, 0] >= self.nbox) & (prs[:, 1] >= self.nbox)).sum())
        if self.kind in ("ref", "host"):
            h = H.collide(ph["transforms"], sc, cap=1 << 17)
            assert h["count"] <= 1 << 17
            o.update(tags=h["keys"], features=h["features"], bodies=h["bodies"], data=h["data"])
        if self.use_ref:
            if n_edits != self.ref_edits:
                self.ref, self.ref_edits = refworld.RefWorld(sc, max_contacts=scene["bp"]["world"].get("max_contacts")), n_edits
            self.ref.set_bodies(transforms=ph["transforms"])
            self.ref.collide()
            rc = self.ref.contacts()
            o["active"] = self.ref.active().astype(np.uint32); o["sleeping"] = P.widen_sleeping(rc["sleeping_pairs"])
            if self.kind == "ref_only":
                od, ob, ok, of, _ = P.oracle_contacts_sorted(rc)
                o.update(tags=ok, features=of, bodies=ob, data=od)
        self.cache[key] = o
        return o


def _edit(w, edits):
    for i, size in edits:
        raw = w.records("xd", 16)                                            # box half extents in place
        rec = np.frombuffer(raw[i].cpu().numpy().tobytes(), np.float32).copy(); rec[:3] = size
        raw[i] = w.torch.from_numpy(rec.view(np.uint8).copy()).to(raw.device)


@pytest.mark.parametrize("case", U.CASES)
def test_broadphase_world_against_brute_force(case):
    scene = U.world(case)
    bp = scene["bp"]
    oracle = _Oracle(scene)
    names = ["default", "no_kept_pairs"] if bp["kind"] == "grid" else ["default", "no_incremental", "no_kept_pairs"]
    worlds = {n: _world(scene, None if n == "default" else "NH_" + n.upper()) for n in names}
    last = {n: dict(broadphase_rebuilds=0, broadphase_inserts=0) for n in names}
    seen = 0
    for k, ph in enumerate(bp["phases"]):
        o = oracle.at(k)
        got = {}
        for n, w in worlds.items():
            where = (case, k, ph["name"], n)
            w.set_bodies(transforms=ph["transforms"])
            _edit(w, ph["edits"])
            w.collide()
            c = w.get_contacts()
            cnt = w.counts()
            got[n] = c
            assert cnt["error"] == 0, where
            d = (cnt["broadphase_rebuilds"] - last[n]["broadphase_rebuilds"], cnt["broadphase_inserts"] - last[n]["broadphase_inserts"])
            last[n] = cnt
            if "tags" in o:
                assert c["count"] == len(o["tags"]), where + (c["count"], len(o["tags"]))
                assert np.array_equal(c["tags"], o["tags"]) and np.array_equal(c["features"], o["features"]), where
                assert np.array_equal(c["bodies"], o["bodies"]), where
                assert P.bits_equal(c["data"], o["data"]), where
            if "active" in o:
                assert np.array_equal(w.get_active(), o["active"]), where
                assert np.array_equal(c["sleeping_pairs"], o["sleeping"]), where
            if "pair_set" in o:
                assert _contact_pairs(c["tags"]) <= o["pair_set"], where
            distinct = len(_contact_pairs(c["tags"]))
            if n == "no_kept_pairs":
                # (the DIRECT search may drop pairs of awake spheres that are surely apart)
                assert distinct <= cnt["raw_pairs"] <= o["pairs"], where + (distinct, cnt["raw_pairs"], o["pairs"])
                if o["sphere_pairs"] == 0:
                    assert cnt["raw_pairs"] == o["pairs"], where + (cnt["raw_pairs"], o["pairs"])
                assert d == (1, 0), where + (d,)
            else:
                assert cnt["raw_pairs"] == o["pairs"], where + (cnt["raw_pairs"], o["pairs"])
                if n == "default":
                    assert d == ph["expect"], where + (d, ph["expect"])
                    if ph["large"] is not None:
                        assert cnt["large_colliders"] == ph["large"], where + (cnt["large_colliders"], ph["large"])
                else:
                    assert d == (1 if ph["expect"] != (0, 0) else 0, 0), where + (d,)          # (no re-insertion: whoever leaves costs a rebuild)
        if "tags" not in o:
            ref = got["no_kept_pairs"]
            for n in names[:-1]:
                c = got[n]
                assert c["count"] == ref["count"] and np.array_equal(c["tags"], ref["tags"]) and np.array_equal(c["features"], ref["features"]), (case, k, n)
                assert np.array_equal(c["bodies"], ref["bodies"]) and P.bits_equal(c["data"], ref["data"]), (case, k, n)
            assert _contact_pairs(ref["tags"]) == o["pair_set"], (case, k)          # (every constructed pair is a deep overlap of two cubes: each gives contacts)
        seen += got["default"]["count"]
    assert seen > 0
    cnt = worlds["default"].counts()
    print(f"\n[{case}] colliders {U.ncolliders(scene)}, pairs {cnt['raw_pairs']}, contacts {cnt['contacts']}, rebuilds {cnt['broadphase_rebuilds']}, "
          f"inserts {cnt['broadphase_inserts']}, large {cnt['large_colliders']}; "
          + ", ".join(f"{n}: rebuilds {last[n]['broadphase_rebuilds']}" for n in names[1:]))
    for w in worlds.values():
        w.close()
