"""The volume records (nh_OverlapQuery, and nh_DistanceQuery, which starts as one) that nh_overlap, nh_penetration and nh_distance must reject, and the ones
that only look spoiled -- enumerated once, for tests/test_cpu_overlap.py, tests/test_cpu_distance.py and tests/test_gpu_volume_records.py."""
import numpy as np

import hostdistance_util as D
from nudge_amd import engine as E

NONE = 0xFFFFFFFF
IDENT = (0.0, 0.0, 0.0, 1.0)


def overlap_query(shape, center, size, rotation=IDENT, ignore=NONE):
    q = np.zeros(1, dtype=E.OVERLAP_QUERY)
    q["shape"], q["center"], q["rotation"], q["ignore_body"] = shape, center, rotation, ignore
    q["size"][0, :len(size)] = size
    return q


def overlap_lists():
    """(invalid, valid): nh_OverlapQuery records of one query each; the valid ones look spoiled and are not."""
    _query = overlap_query
    nan, inf = float("nan"), float("inf")
    S_, B_ = E.NH_SHAPE_SPHERE, E.NH_SHAPE_BOX
    invalid = [_query(2, (0, 0, 0), (1e5,)), _query(NONE, (0, 0, 0), (1e5,)), _query(S_, (0, nan, 0), (1e5,)), _query(S_, (inf, 0, 0), (1e5,)),
               _query(S_, (0, 0, 0), (inf,)), _query(S_, (0, 0, 0), (nan,)), _query(S_, (0, 0, 0), (-1.0,)),
               _query(B_, (0, 0, 0), (1e5, 1e5, -1.0)), _query(B_, (0, 0, 0), (1e5, nan, 1e5)), _query(B_, (0, 0, 0), (1e5, 1e5, 1e5), rotation=(0, nan, 0, 1)),
               _query(B_, (0, 0, 0), (1e5, 1e5, 1e5), rotation=(0, 0, 0, inf))]
    valid = [_query(S_, (0, 0, 0), (1e5, nan, -1.0), rotation=(nan, nan, nan, nan)),        # a sphere ignores size[1..2] and the rotation
             _query(S_, (0, 0, 0), (-0.0,)), _query(B_, (0, 0, 0), (1e5, 1e5, 1e5))]
    return invalid, valid


def distance_bases():
    """(sphere, box, capsule): one valid nh_DistanceQuery each, at (3, 0, 0)."""
    return D.queries([(3, 0, 0)], radii=0.5), D.queries([(3, 0, 0)], half_extents=(0.5, 0.5, 0.5)), D.queries([(3, 0, 0)], radii=0.5, half_heights=0.5)


def distance_lists():
    """(bad, ok): nh_DistanceQuery records of one query each -- every way to spoil a base, and (record, the base it must answer as) for what is not read."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    bad = []

    def spoil(base, field, value, at=None):
        qq = base.copy()
        if at is None:
            qq[field] = value
        else:
            qq[field][0, at] = value
        bad.append(qq)

    sphere, boxq, cap = distance_bases()
    for base in (sphere, boxq, cap):
        spoil(base, "shape", 7)
        spoil(base, "center", nan, 1)
        spoil(base, "center", inf, 0)
        spoil(base, "size", -1.0, 0)
        spoil(base, "size", nan, 0)
        spoil(base, "max_distance", nan)
        spoil(base, "max_distance", -1.0)
        spoil(base, "max_distance", -inf)
    for base in (boxq, cap):
        spoil(base, "size", -0.5, 1)
        spoil(base, "size", inf, 1)
        spoil(base, "rotation", nan, 2)
    spoil(boxq, "size", nan, 2)
    # what is not read does not spoil: a sphere's rotation and size[1..2], a capsule's size[2], reserved
    ok = []
    qq = sphere.copy()
    qq["rotation"], qq["size"][0, 1:], qq["reserved"] = nan, nan, 0xDEADBEEF
    ok.append((qq, sphere))
    qq = cap.copy()
    qq["size"][0, 2] = nan
    ok.append((qq, cap))
    return bad, ok
