"""The crafted island, sleeping and cache worlds of tests/island_cases_util.py on the GPU, against the numpy oracle of that module (a full union over every edge; proven
equal to the compiled reference on every world the reference can hold by tests/test_cpu_island_cases.py) and, where oracle/_ref is present and the world fits, against the
reference itself.  Every world runs in two forms -- the default world and one with the DIRECT search (NH_NO_KEPT_PAIRS) --, one world per case and form across its phases;
a phase states every idle counter through set_bodies(idle=...) and calls collide().  After each: no error, and the active list, its count, the contact count, the contacts'
tags, features and bodies and the sleeping pairs equal the oracle's.  The two large instances (140,000 and 530,000 bodies: beyond the thread counts of the coarse and of the
fine island launches) have the oracle alone; three fresh worlds of the larger one must agree byte for byte.  The cache scripts restore caches the library did not write
and go through collide -> read_cache -> write_cache (against the oracle's cull, lookup and merge) and through collide -> read_cache -> setup -> apply(0) -> update ->
write_cache under the bench flags and under NH_FLAG_EXACT_ORDER (against the reference running the same stages); the tie rule of the merge is reached through
contacts appended behind collide()'s list.  Every comparison is exact.

A HIP error behind any call ends the whole pytest session (pytest.exit, return code 3): nothing more is started on a device that has reported a fault."""
import contextlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostsim_util as H                    # noqa: E402
import island_cases_util as U               # noqa: E402
import parity_util as P                     # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from oracle import refworld                 # noqa: E402

pytestmark = pytest.mark.gpu
FLAGS = E.NH_FLAG_SYNC_COUNTS
BENCH_FLAGS = E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP
EXACT = E.NH_FLAG_SYNC_COUNTS | E.NH_FLAG_EXACT_ORDER
NH_ERR_NO_DEVICE, NH_ERR_HIP = 2, 8        # include/nudge_hip.h
FORMS = ["default", "direct"]
_REF = {}                                   # (case, phase index) -> the reference's lists; (case, cache name) -> its cache after the zero-iteration solve


@contextlib.contextmanager
def hip_guard():
    """Nothing more is started once the device has reported an error."""
    try:
        yield
    except E.NudgeError as e:
        if str(e).endswith(f"({NH_ERR_HIP})") or str(e).endswith(f"({NH_ERR_NO_DEVICE})"):
            pytest.exit(f"HIP error behind a library call: {e}: stopping", returncode=3)
        raise
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e):
            pytest.exit(f"HIP error: {e}: stopping", returncode=3)
        raise


def _world(scene, form, flags=FLAGS):
    if form == "direct":
        os.environ["NH_NO_KEPT_PAIRS"] = "1"
    try:
        return E.World(scene, flags=flags)
    finally:
        os.environ.pop("NH_NO_KEPT_PAIRS", None)


def _use_ref(scene):
    return refworld.available("exact") and U.ncolliders(scene) <= U.REF_LIMIT


def _ref_lists(w):
    rc = w.contacts()
    od, ob, ok, of, _ = P.oracle_contacts_sorted(rc)
    return dict(active=w.active().astype(np.uint32), tags=ok, features=of, bodies=ob, data=od, sleeping=P.widen_sleeping(rc["sleeping_pairs"]))


def _reference(case, scene):
    """The reference's lists after every phase of a world it can hold, computed once and shared by the two forms."""
    if (case, 0) not in _REF:
        w = refworld.RefWorld(scene)
        for k, ph in enumerate(scene["isl"]["phases"]):
            w.set_bodies(idle=ph["idle"])
            w.collide()
            _REF[case, k] = _ref_lists(w)
    return [_REF[case, k] for k in range(len(scene["isl"]["phases"]))]


def _check_lists(w, o, where, ref=None):
    c, act, cnt = w.get_contacts(), w.get_active(), w.counts()
    assert cnt["error"] == 0, where + (cnt["error"],)
    assert cnt["active_bodies"] == len(o["active"]) and np.array_equal(act, o["active"]), where + (cnt["active_bodies"], len(o["active"]))
    assert cnt["contacts"] == c["count"] == len(o["tags"]), where + (cnt["contacts"], len(o["tags"]))
    assert np.array_equal(c["tags"], o["tags"]) and np.array_equal(c["features"], o["features"]) and np.array_equal(c["bodies"], o["bodies"]), where
    if "data" in o:
        assert P.bits_equal(c["data"], o["data"]), where
    assert cnt["sleeping_pairs"] == len(o["sleeping"]) and np.array_equal(c["sleeping_pairs"], o["sleeping"]), where + (cnt["sleeping_pairs"], len(o["sleeping"]))
    if ref is not None:
        assert np.array_equal(act, ref["active"]) and np.array_equal(c["sleeping_pairs"], ref["sleeping"]), where
        assert np.array_equal(c["tags"], ref["tags"]) and np.array_equal(c["features"], ref["features"]) and np.array_equal(c["bodies"], ref["bodies"]), where
        assert P.bits_equal(c["data"], ref["data"]), where
    return c, act, cnt


def _run_phases(case, scene, form, oracle, refs=None):
    with hip_guard():
        w = _world(scene, form)
        last = 0
        out = []
        for k, ph in enumerate(scene["isl"]["phases"]):
            w.set_bodies(idle=ph["idle"])
            w.collide()
            c, act, cnt = _check_lists(w, oracle[k], (case, form, k, ph["name"]), refs[k] if refs else None)
            if scene["isl"]["kind"] == "geometry" and form == "default":
                # the path: the first call builds the kept list, the second re-uses it (k_kept_filter unites); the DIRECT world searches at every call
                assert cnt["broadphase_rebuilds"] - last == (1 if k == 0 else 0), (case, form, k, cnt["broadphase_rebuilds"])
            if form == "direct":
                assert cnt["broadphase_rebuilds"] - last == 1, (case, form, k)
            last = cnt["broadphase_rebuilds"]
            out.append((act.tobytes(), c["sleeping_pairs"].tobytes()))
        w.close()
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", U.CASES)
def test_island_world_against_the_oracle(case, form):
    scene = U.world(case)
    pairs, contacts = U.lists(scene)
    oracle = [U.expected(scene, ph, pairs, contacts) for ph in scene["isl"]["phases"]]
    _run_phases(case, scene, form, oracle, _reference(case, scene) if _use_ref(scene) else None)
    print(f"\n[{case}/{form}] bodies {len(scene['body_transforms']) - 1}, connections {len(scene['connections'])}: "
          + "; ".join(f"{ph['name']}: active {len(o['active'])}, contacts {len(o['tags'])}, sleeping {len(o['coarse_sleeping'])} coarse + {len(o['fine_sleeping'])} fine"
                      for ph, o in zip(scene["isl"]["phases"], oracle)))


def test_chain_shuffled_beyond_the_coarse_launches():
    """140,000 bodies in one chain, edges in random order: more connections and bodies than the 131,072 threads of the coarse-level island launches."""
    case, n = "chain_shuffled", U.LARGE["chain_shuffled"]
    scene = U.world(case, n)
    pairs, contacts = U.lists(scene)
    oracle = [U.expected(scene, ph, pairs, contacts) for ph in scene["isl"]["phases"]]
    assert len(oracle[0]["active"]) == n and len(oracle[1]["sleeping"]) == n
    for form in FORMS:
        _run_phases(case, scene, form, oracle)
    U.forget(case, n)


def test_confetti_beyond_the_fine_launches_and_run_to_run():
    """530,000 bodies in ~50,000 components: more than the 524,288 threads of the fine-level island launches; three fresh worlds give byte-identical lists."""
    case, n = "confetti", U.LARGE["confetti"]
    scene = U.world(case, n)
    pairs, contacts = U.lists(scene)
    oracle = [U.expected(scene, ph, pairs, contacts) for ph in scene["isl"]["phases"]]
    assert 0 < len(oracle[0]["active"]) < n
    runs = [_run_phases(case, scene, "default", oracle) for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]
    _run_phases(case, scene, "direct", oracle)
    U.forget(case, n)


# ---- caches the library did not write -----------------------------------------------------------------------------------------------------------------------------------
def _reference_solve(case, scene, name, cache, K):
    if (case, name) not in _REF:
        w = refworld.RefWorld(scene, max_contacts=K)
        w.restore(dict(bodies=dict(transforms=scene["body_transforms"], momentum=scene["body_momentum"], idle=scene["isl"]["phases"][0]["idle"]),
                       cache_count=cache["count"], cache_tags=U.narrow_cache(cache), cache_data=cache["data"]))
        w.collide(); w.read_cache(); w.setup(); w.apply(0); w.update(); w.write_cache()
        rk = w.cache()
        wt, wf = U.widen_cache(rk)
        _REF[case, name] = dict(count=rk["count"], tags=wt, features=wf, data=rk["data"])
    return _REF[case, name]


def _same_cache(got, want, where, payload="all"):
    assert got["count"] == want["count"], where + (got["count"], want["count"])
    assert np.array_equal(got["tags"], want["tags"]) and np.array_equal(got["features"], want["features"]), where
    if payload == "all":
        assert P.bits_equal(got["data"], want["data"]), where
    else:
        assert P.bits_equal(got["data"]["impulse"], want["data"]["impulse"]), where


@pytest.mark.parametrize("way", ["read_write", "solve_bench", "solve_exact"])
@pytest.mark.parametrize("case", U.CACHE_WORLDS)
def test_crafted_caches(case, way):
    """One world per case and way; every crafted cache is restored into it as a checkpoint (the body arrays unchanged), so a cache also meets the hints and the slots the
    script before it left behind."""
    scene = U.world(case)
    ph = scene["isl"]["phases"][0]
    o = U.expected(scene, ph)
    if way != "read_write":
        assert _use_ref(scene), "oracle/_ref/libnudge_ref_exact.so did not travel to this box: the zero-iteration solve has no other oracle"
    with hip_guard():
        w = _world(scene, "default", {"read_write": FLAGS, "solve_bench": BENCH_FLAGS, "solve_exact": EXACT}[way])
        K = w.max_contacts
        caches = U.crafted_caches(scene, o, K)
        pristine = w.snapshot()
        for name in U.CACHES:
            cache = caches[name]
            m = U.cache_stages(cache, o, o["sleeping"])
            for peek in ((True, False) if way == "read_write" else (False,)):
                where = (case, way, name, peek)
                U.restore_cache(w, cache, pristine)
                w.collide()
                _check_lists(w, o, where)
                w.read_cache()
                if way == "read_write":
                    if peek:          # (the lookup by itself; without the peek write_cache runs it)
                        assert P.bits_equal(w.get_contact_impulses(), m["lookup"]), where
                    w.write_cache()
                    _same_cache(w.get_cache(), m["write"], where)
                else:
                    w.setup(); w.apply(0); w.update(); w.write_cache()
                    got = w.get_cache()
                    assert got["count"] == m["write"]["count"] and np.array_equal(got["tags"], m["write"]["tags"]) and np.array_equal(got["features"], m["write"]["features"]), where
                    _same_cache(got, _reference_solve(case, scene, name, cache, K), where, payload="impulse")
                cnt = w.counts()
                assert cnt["error"] == 0 and cnt["culled"] == int(m["culled"].sum()), where + (cnt["error"], cnt["culled"])
        w.close()


@pytest.mark.parametrize("way", ["solve_bench", "solve_exact"])
def test_culled_entry_precedes_an_appended_contact_of_equal_key(way):
    """island_cases_util.tie_script: the tie rule of k_write_cache ("if (a < b) contact else culled", nudge.cpp:4130), reached through nh_append_contacts."""
    scene = U.world("near_miss_chain")
    o = U.expected(scene, scene["isl"]["phases"][0])
    extra, cache = U.tie_script(scene, o)
    m = U.cache_stages(cache, extra, o["sleeping"])
    assert _use_ref(scene), "oracle/_ref/libnudge_ref_exact.so did not travel to this box"
    with hip_guard():
        w = _world(scene, "default", BENCH_FLAGS if way == "solve_bench" else EXACT)
        U.restore_cache(w, cache, w.snapshot())
        w.collide()
        _check_lists(w, o, (way, "before the append"))
        w.append_contacts(extra["data"], extra["bodies"], extra["tags"], extra["features"])
        w.read_cache(); w.setup(); w.apply(0); w.update(); w.write_cache()
        got, cnt = w.get_cache(), w.counts()
        w.close()
    r = refworld.RefWorld(scene, max_contacts=w.max_contacts)
    r.restore(dict(bodies=dict(transforms=scene["body_transforms"], momentum=scene["body_momentum"], idle=scene["isl"]["phases"][0]["idle"]),
                   cache_count=cache["count"], cache_tags=U.narrow_cache(cache), cache_data=cache["data"]))
    r.collide()
    r.append_contacts(extra["data"], extra["bodies"], H.narrow_tags(extra["tags"], extra["features"]))
    r.read_cache(); r.setup(); r.apply(0); r.update(); r.write_cache()
    rk = r.cache()
    wt, wf = U.widen_cache(rk)
    assert cnt["error"] == 0 and cnt["culled"] == cache["count"]
    assert got["count"] == m["write"]["count"] and np.array_equal(got["tags"], m["write"]["tags"]) and np.array_equal(got["features"], m["write"]["features"])
    ties = [i for i in range(got["count"] - 1) if got["tags"][i] == got["tags"][i + 1] and got["features"][i] == got["features"][i + 1]]
    assert len(ties) == 3
    for i in ties:          # the entry kept aside comes first, verbatim; the contact's solved impulse differs from it
        assert P.bits_equal(got["data"][i], m["write"]["data"][i]), (way, i)
        assert not P.bits_equal(rk["data"][i + 1]["impulse"], m["write"]["data"][i + 1]["impulse"]), (way, i)
    _same_cache(got, dict(count=rk["count"], tags=wt, features=wf, data=rk["data"]), (way, "against the reference"), payload="impulse")
