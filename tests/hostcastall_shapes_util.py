"""ctypes access to the all-hits box and capsule oracle of tests/hostoracle/hostcastall_shapes.cpp (built by tests/hostlib.py): nh_boxcast_all /
nh_capsulecast_all by brute force on the host -- the per-collider arithmetic of nudge_amd/csrc/nh_query.h with the device's bits, and the header's rules
around it (ignore_body, the reach rule, the order by t with ties in index order, offsets, the capacity prefix, the marker): the oracle of the GPU's chain."""
import hostlib as H
from hostlib import records      # noqa: F401
from nudge_amd import engine as E

lib = H.oracle({"hs_boxcast_all": H.BATCH, "hs_capsulecast_all": H.BATCH})


def boxcast_all(rec, nbox, casts, capacity=None, hits=None, threads=None):
    """(offsets, hits, true total) of nh_boxcast_all by brute force over `rec` (hostlib.REC); `casts`: E.BOX_CAST.  capacity=None: room for every
    record.  `hits` (E.RAY_HIT, at least `capacity` long) is written in place when given -- bytes behind the written prefix are left as they are."""
    return H.batch(lib().hs_boxcast_all, E.BOX_CAST, E.RAY_HIT, rec, nbox, casts, capacity, hits, threads)


def capsulecast_all(rec, nbox, casts, capacity=None, hits=None, threads=None):
    """The same for nh_capsulecast_all (`casts`: E.CAPSULE_CAST)."""
    return H.batch(lib().hs_capsulecast_all, E.CAPSULE_CAST, E.RAY_HIT, rec, nbox, casts, capacity, hits, threads)
