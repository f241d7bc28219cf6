"""bench.py --dump-outputs without a GPU: what dump_outputs() writes from the arrays a caller of the timed path receives (World.get_bodies / get_contacts /
get_cache / counts layouts): float32 / float64 only, at most 64 MB, the same seeded sample every time, and the sampled records are the right ones."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                        # noqa: E402
from nudge_amd import scenes as S   # noqa: E402


def _outputs(nb, nk):
    rng = np.random.default_rng(11)
    t = np.zeros(nb, S.TRANSFORM)
    t["position"][:, 0] = np.arange(nb)
    t["rotation"] = rng.standard_normal((nb, 4)).astype(np.float32)
    m = np.zeros(nb, S.MOMENTUM)
    m["velocity"] = rng.standard_normal((nb, 3)).astype(np.float32)
    bodies = dict(transforms=t, momentum=m, idle=rng.integers(0, 256, nb).astype(np.uint8))
    d = np.zeros(nk, S.CONTACT)
    d["penetration"] = np.arange(nk)
    tags = rng.integers(0, 2 ** 64, nk, dtype=np.uint64)         # (above 2^53: must survive as two exact halves)
    contacts = dict(count=nk, data=d, bodies=rng.integers(0, nb, (nk, 2)).astype(np.uint32), tags=tags, features=rng.integers(0, 2 ** 32, nk, dtype=np.uint32),
                    sleeping_pairs=np.zeros(0, np.uint64))
    imp = np.zeros(nk, S.IMPULSE)
    imp["impulse"] = rng.standard_normal((nk, 3)).astype(np.float32)
    cache = dict(count=nk, tags=tags.copy(), features=contacts["features"].copy(), data=imp)
    counts = dict(contacts=nk, sleeping_pairs=3, active_bodies=nb, cache=nk, pairs=nk // 4)
    return bodies, contacts, cache, counts


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_float_only_under_64_mb_and_the_same_sample_every_time(tmp_path):
    nb, nk = 2 * bench.DUMP_SAMPLE + 5, 3 * bench.DUMP_SAMPLE + 7
    b, c, k, n = _outputs(nb, nk)
    bench.dump_outputs(str(tmp_path / "a"), b, c, k, n)
    bench.dump_outputs(str(tmp_path / "b"), b, c, k, n)
    a, a2 = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == sorted(a2) and all(np.array_equal(a[x], a2[x]) for x in a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a"))) <= 64 << 20
    idx = a["body_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE and np.all(np.diff(idx) > 0) and idx[-1] < nb
    assert np.array_equal(a["body_position"][:, 0], idx.astype(np.float32))
    assert np.array_equal(a["body_rotation"], b["transforms"]["rotation"][idx])
    assert np.array_equal(a["body_velocity"], b["momentum"]["velocity"][idx])
    assert np.array_equal(a["body_idle"], b["idle"][idx].astype(np.float32))
    ic = a["contact_penetration"].astype(np.int64)
    assert len(ic) == bench.DUMP_SAMPLE and np.all(np.diff(ic) > 0)
    tag = a["contact_tag"].astype(np.uint64)
    assert np.array_equal((tag[:, 0] << np.uint64(32)) | tag[:, 1], c["tags"][ic])
    assert np.array_equal(a["contact_bodies"], c["bodies"][ic].astype(np.float64))
    assert np.array_equal(a["contact_feature"], c["features"][ic].astype(np.float64))
    assert np.array_equal(a["counts"], [nk, 3, nb, nk])


def test_small_world_is_dumped_whole_and_in_order(tmp_path):
    b, c, k, n = _outputs(1000, 3000)
    bench.dump_outputs(str(tmp_path), b, c, k, n, prefix="rank1_")
    a = _load(str(tmp_path))
    assert all(x.startswith("rank1_") for x in a)
    assert np.array_equal(a["rank1_body_index"], np.arange(1000, dtype=np.float64))
    assert np.array_equal(a["rank1_contact_penetration"], np.arange(3000, dtype=np.float32))
    assert np.array_equal(a["rank1_cache_impulse"], k["data"]["impulse"])


def test_partitioned_world_dumps_global_ids_without_contacts(tmp_path):
    b, _, _, _ = _outputs(500, 0)
    b["ids"] = np.arange(1, 501, dtype=np.int64)
    bench.dump_outputs(str(tmp_path), b)
    a = _load(str(tmp_path))
    assert np.array_equal(a["body_index"], np.arange(1, 501, dtype=np.float64))
    assert not [x for x in a if x.startswith(("contact_", "cache_"))] and "counts" not in a
