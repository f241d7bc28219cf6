"""The launches of the list calls' host chain, pinned (pytest -m gpu): for each of the nine calls that write variable-length lists, the
{timing label: launches} of one count-only call and of one list call whose capacity is the total must equal the table below, which the library
of the commit before the calls were put on one host chain printed (profiles/list_launches_parent.log).  The byte-for-byte tests cannot see a
dropped memset that happens to be harmless, or a doubled launch; this one cannot see a wrong byte.  Run as a program it prints the table of the
library it loads (NUDGE_HIP_LIBRARY names another build)."""
import os
import sys

import numpy as np
import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import cast_util as CU                       # noqa: E402
from query_util import FUSED, NONE, records as _records, upload as _upload      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

pytestmark = pytest.mark.gpu

# {call: (count-only launches, list launches)}
LAUNCHES = {
    "overlap_records": ({'q_overlap_count': 1, 'q_overlap_count_capsule': 1, 'q_overlap_fin': 1, 'q_overlap_fix': 1, 'scan_final': 1, 'scan_sums': 1},
        {'q_overlap_count': 1, 'q_overlap_count_capsule': 1, 'q_overlap_fin': 1, 'q_overlap_fix': 1, 'q_overlap_gather': 1, 'q_overlap_list': 1, 'q_overlap_list_capsule': 1, 'radix_hist': 2, 'radix_scan': 2, 'radix_scatter': 2, 'scan_final': 1, 'scan_sums': 1}),
    "penetration_records": ({'q_overlap_count': 1, 'q_overlap_count_capsule': 1, 'q_overlap_fin': 1, 'q_overlap_fix': 1, 'scan_final': 1, 'scan_sums': 1},
        {'q_overlap_count': 1, 'q_overlap_count_capsule': 1, 'q_overlap_fin': 1, 'q_overlap_fix': 1, 'q_overlap_list': 1, 'q_overlap_list_capsule': 1, 'q_penetration_gather': 1, 'radix_hist': 2, 'radix_scan': 2, 'radix_scatter': 2, 'scan_final': 1, 'scan_sums': 1}),
    "overlap_wide_records": ({'q_overlap_fin': 1, 'q_overlap_fix': 1, 'q_wide_count': 1, 'q_wide_count_capsule': 1, 'scan_final': 1, 'scan_sums': 1},
        {'q_overlap_fin': 1, 'q_overlap_fix': 1, 'q_overlap_gather': 1, 'q_wide_count': 1, 'q_wide_count_capsule': 1, 'q_wide_list': 1, 'q_wide_list_capsule': 1, 'radix_hist': 2, 'radix_scan': 2, 'radix_scatter': 2, 'scan_final': 1, 'scan_sums': 1}),
    "penetration_wide_records": ({'q_overlap_fin': 1, 'q_overlap_fix': 1, 'q_wide_count': 1, 'q_wide_count_capsule': 1, 'scan_final': 1, 'scan_sums': 1},
        {'q_overlap_fin': 1, 'q_overlap_fix': 1, 'q_penetration_gather': 1, 'q_wide_count': 1, 'q_wide_count_capsule': 1, 'q_wide_list': 1, 'q_wide_list_capsule': 1, 'radix_hist': 2, 'radix_scan': 2, 'radix_scatter': 2, 'scan_final': 1, 'scan_sums': 1}),
    "region_records": ({'q_overlap_fin': 1, 'q_overlap_fix': 1, 'q_region_count': 1, 'scan_final': 1, 'scan_sums': 1},
        {'q_overlap_fin': 1, 'q_overlap_fix': 1, 'q_overlap_gather': 1, 'q_region_count': 1, 'q_region_list': 1, 'radix_hist': 2, 'radix_scan': 2, 'radix_scatter': 2, 'scan_final': 1, 'scan_sums': 1}),
    "raycast_all_records": ({'q_overlap_fin': 1, 'q_overlap_fix': 1, 'q_raycast_all_count': 1, 'scan_final': 1, 'scan_sums': 1},
        {'q_overlap_fin': 1, 'q_overlap_fix': 1, 'q_raycast_all_count': 1, 'q_raycast_all_gather': 1, 'q_raycast_all_list': 1, 'radix_hist': 6, 'radix_scan': 6, 'radix_scatter': 6, 'scan_final': 1, 'scan_sums': 1}),
    "spherecast_all_records": ({'q_overlap_fin': 1, 'q_overlap_fix': 1, 'q_spherecast_all_count': 1, 'scan_final': 1, 'scan_sums': 1},
        {'q_overlap_fin': 1, 'q_overlap_fix': 1, 'q_spherecast_all_count': 1, 'q_spherecast_all_gather': 1, 'q_spherecast_all_list': 1, 'radix_hist': 6, 'radix_scan': 6, 'radix_scatter': 6, 'scan_final': 1, 'scan_sums': 1}),
    "boxcast_all_records": ({'q_boxcast_all_count': 1, 'q_overlap_fin': 1, 'q_overlap_fix': 1, 'scan_final': 1, 'scan_sums': 1},
        {'q_boxcast_all_count': 1, 'q_boxcast_all_gather': 1, 'q_boxcast_all_list': 1, 'q_overlap_fin': 1, 'q_overlap_fix': 1, 'radix_hist': 6, 'radix_scan': 6, 'radix_scatter': 6, 'scan_final': 1, 'scan_sums': 1}),
    "capsulecast_all_records": ({'q_capsulecast_all_count': 1, 'q_overlap_fin': 1, 'q_overlap_fix': 1, 'scan_final': 1, 'scan_sums': 1},
        {'q_capsulecast_all_count': 1, 'q_capsulecast_all_gather': 1, 'q_capsulecast_all_list': 1, 'q_overlap_fin': 1, 'q_overlap_fix': 1, 'radix_hist': 6, 'radix_scan': 6, 'radix_scatter': 6, 'scan_final': 1, 'scan_sums': 1}),
}


def _batches(rec):
    """{World method: 3 records}: two that list something and one, the last, that overlaps nothing."""
    at = rec["p"][[1, 40]].astype(np.float32)
    q = np.zeros(3, dtype=E.OVERLAP_QUERY)
    q["shape"], q["rotation"], q["ignore_body"] = (E.NH_SHAPE_SPHERE, E.NH_SHAPE_BOX, E.NH_SHAPE_CAPSULE), (0, 0, 0, 1), NONE
    q["center"], q["size"] = [at[0], at[1], at[0] + np.float32(1e3)], [(2.0, 0, 0), (1.5, 1.5, 1.5), (0.5, 0.5, 0)]
    regions = np.zeros(3, dtype=E.REGION)
    regions["plane_count"], regions["ignore_body"] = 2, NONE
    regions["planes"][:, :2] = [[(0.0, 1.0, 0.0, 1e6), (0.0, 1.0, 0.0, 1e6)],                                             # everything
                                [(1.0, 0.0, 0.0, 2.0 - at[0, 0]), (-1.0, 0.0, 0.0, 2.0 + at[0, 0])],                       # a slab about a collider
                                [(-1.0, 0.0, 0.0, at[0, 0]), (1.0, 0.0, 0.0, -(at[0, 0] + 1e4))]]                          # a gap: nothing
    rays = np.zeros(3, dtype=E.RAY)
    rays["origin"], rays["max_t"], rays["ignore_body"] = at[[0, 1, 0]] + np.float32([0.0, 50.0, 0.0]), np.inf, NONE
    rays["direction"] = [(0, -1, 0), (0, -1, 0), (0, 1, 0)]               # two straight down through a collider, one up and away
    b = {name: q for name in ("overlap_records", "penetration_records", "overlap_wide_records", "penetration_wide_records")}
    b.update(region_records=regions, raycast_all_records=rays, spherecast_all_records=CU.spheres(rays, 0.5), boxcast_all_records=CU.boxes(rays, 0.5),
             capsulecast_all_records=CU.capsules(rays, 0.5, 0.5))
    return b


def _launches(w, call, records, size):
    """({label: launches} of the count-only call, of the list call with the total as its capacity), the timers read and reset after each."""
    import torch
    qt = _upload(w, records)
    offsets, _ = getattr(w, call)(qt)
    count = {k: v[1] for k, v in w.kernel_times().items()}
    total = int(offsets[len(records)].item()) & NONE
    assert 0 < total < 4096 and int(offsets[len(records) - 1].item()) == total, (call, total)          # (the last record lists nothing)
    getattr(w, call)(qt, offsets=offsets, hits=torch.empty((total, size), dtype=torch.uint8, device=w.dev), capacity=total)
    return count, {k: v[1] for k, v in w.kernel_times().items()}


def _table():
    scene = S.pile(64, 16, seed=3)
    w = E.World(scene, flags=FUSED)
    w.query_build()
    w.synchronize()
    w.enable_timing()
    w.kernel_times()
    out = {call: _launches(w, call, rec, 16 if call in ("overlap_records", "overlap_wide_records", "region_records") else 32)
           for call, rec in _batches(_records(w, scene)).items()}
    w.close()
    return out


def test_each_list_call_launches_what_it_launched_before_the_calls_shared_one_chain():
    got = _table()
    assert sorted(got) == sorted(LAUNCHES)
    for call in got:
        assert got[call] == LAUNCHES[call], (call, got[call], LAUNCHES[call])


if __name__ == "__main__":
    for call, (count, lists) in _table().items():
        print(f'    "{call}": ({dict(sorted(count.items()))},\n        {dict(sorted(lists.items()))}),')
