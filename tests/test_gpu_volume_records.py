"""One volume decode behind three calls: nh_overlap, nh_penetration and nh_distance read a volume record through the same decode (nh_QVolume,
nudge_amd/csrc/nh_query.hip), and the header promises that they agree on which records are valid.  One batch -- one wave -- of every invalid and every
"valid although it looks spoiled" record that tests/volume_records.py enumerates for the CPU tests of the two oracles, with the capsule's own, against
a world of a box, a sphere and a collider of a body that does not exist: each call byte for byte its host oracle, nh_penetration's offsets
nh_overlap's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hostcapsule_util as HC                # noqa: E402
import hostdistance_util as D                # noqa: E402
import hostpen_util as HP                    # noqa: E402
import hostquery_util as Q                   # noqa: E402
from list_util import gpu_list               # noqa: E402
from query_util import upload as _upload      # noqa: E402
from volume_records import distance_bases, distance_lists, overlap_lists      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

FUSED = E.NH_FLAG_SINGLE_APPLY | E.NH_FLAG_FUSED_STEP


def _batch():
    """nh_DistanceQuery records; their first 48 bytes are the nh_OverlapQuery batch.  The records of the overlap lists get max_distance = +inf."""
    nan = np.float32(np.nan)
    invalid, valid = overlap_lists()
    bad, ok = distance_lists()
    recs = [*bad, *(qq for qq, _ in ok)]
    for o in (*invalid, *valid):
        qq = np.zeros(1, dtype=E.DISTANCE_QUERY)
        for f in E.OVERLAP_QUERY.names:
            qq[f] = o[f]
        qq["max_distance"] = np.inf
        recs.append(qq)
    cap = distance_bases()[2]
    for field, at, value, rot in (("size", 1, nan, None), ("size", 1, 0.0, nan), ("size", 0, -1.0, None)):      # NaN half height; half height 0 with a NaN rotation (a sphere: valid); negative radius
        qq = cap.copy()
        qq[field][0, at] = value
        if rot is not None:
            qq["rotation"] = rot
        recs.append(qq)
    q = np.concatenate(recs)
    assert len(q) < 64
    return q


def _as_overlap(q):
    o = np.zeros(len(q), dtype=E.OVERLAP_QUERY)
    for f in E.OVERLAP_QUERY.names:
        o[f] = q[f]
    assert o.tobytes() == q.view(np.uint8).reshape(-1, 64)[:, :48].tobytes()
    return o


def test_the_two_oracles_agree_on_which_records_are_valid():
    """On the host: against one box that contains every finite centre, a valid volume overlaps it (count 1) and is at distance 0 from it; an invalid one
    counts 0 and answers NaN.  Where max_distance itself is valid the two must say the same of every record."""
    rec = np.zeros(1, dtype=Q.REC)
    rec["q"], rec["h"], rec["body"], rec["tag"] = (0, 0, 0, 1), (1e6, 1e6, 1e6), 1, 7
    q = _batch()
    off, _, total = HC.overlap(rec, 1, _as_overlap(q))
    valid = np.diff(off.astype(np.int64)) == 1
    assert total == int(valid.sum())
    off_p, _, _ = HP.penetration(rec, 1, _as_overlap(q))
    assert off_p.tobytes() == off.tobytes()
    d = D.distance(rec, 1, q)["distance"]
    md_ok = q["max_distance"] >= 0
    assert np.array_equal(~np.isnan(d[md_ok]), valid[md_ok]) and np.isnan(d[~md_ok]).all()
    # valid as volumes: the 9 records whose max_distance alone is spoiled, the 2 + 3 that only look spoiled, the capsule of half height 0 -- and the
    # overlap list's "shape 2", which only the oracle without capsules rejects: it is a capsule of half height 0
    assert int((~md_ok).sum()) == 9 and int(valid.sum()) == 9 + 2 + 3 + 1 + 1


@pytest.mark.gpu
def test_one_batch_of_every_invalid_and_every_unspoiled_record():
    scene = S.pile(0, 2, seed=3)
    scene["body_transforms"]["position"][1] = (4.0, 0.0, 0.5)          # the sphere: the small queries at (3, 0, 0) touch it
    nb = len(scene["body_transforms"])
    w = E.World(scene, flags=FUSED)
    w.set_counts(nb - 1, w.nbox, w.nsph)                  # the last sphere belongs to a body that no longer exists: a NaN pose
    w.query_build()
    assert (w.nbox, w.nsph) == (1, 2)
    rec = Q.records(w.get_bodies()["transforms"][: nb - 1], scene, w.nbox, w.nsph)
    assert np.isfinite(rec["p"][:2]).all() and np.isnan(rec["p"][2]).all()
    q = _batch()
    o = _as_overlap(q)

    ref_off, ref_hits, total = HC.overlap(rec, w.nbox, o)
    assert 0 < total < 3 * len(q)
    cnt, _ = gpu_list(w, "overlap_records", o, None, E.OVERLAP_HIT)
    off, hits = gpu_list(w, "overlap_records", o, total, E.OVERLAP_HIT)
    assert cnt.tobytes() == ref_off.tobytes() and off.tobytes() == ref_off.tobytes()
    assert hits.tobytes() == ref_hits[:total].tobytes()

    pen_off, pen_hits, pen_total = HP.penetration(rec, w.nbox, o)
    assert pen_total == total
    pcnt, _ = gpu_list(w, "penetration_records", o, None, HP.HIT)
    poff, phits = gpu_list(w, "penetration_records", o, total, HP.HIT)
    assert pcnt.tobytes() == pen_off.tobytes() and poff.tobytes() == pen_off.tobytes()
    assert phits.tobytes() == pen_hits[:total].tobytes()
    assert poff.tobytes() == off.tobytes()

    got = np.frombuffer(w.distance_records(_upload(w, q)).cpu().numpy().tobytes(), dtype=E.POINT_HIT)
    assert got.tobytes() == D.distance(rec, w.nbox, q).tobytes()
    w.close()
