"""ctypes access to the all-hits oracle of tests/hostoracle/hostcastall.cpp (built by tests/hostlib.py): nh_raycast_all / nh_spherecast_all by brute
force on the host -- the per-collider arithmetic of nudge_amd/csrc/nh_query.h with the device's bits, and the header's rules around it (ignore_body, the
reach rule, the order by t with ties in index order, offsets, the capacity prefix, the marker): the oracle of the GPU's chain."""
import hostlib as H
from hostlib import records      # noqa: F401
from nudge_amd import engine as E

lib = H.oracle({"hc_raycast_all": H.BATCH, "hc_spherecast_all": H.BATCH})


def raycast_all(rec, nbox, rays, capacity=None, hits=None, threads=None):
    """(offsets, hits, true total) of nh_raycast_all by brute force over `rec` (hostlib.REC).  capacity=None: room for every record.  `hits`
    (E.RAY_HIT, at least `capacity` long) is written in place when given -- bytes behind the written prefix are left as they are."""
    return H.batch(lib().hc_raycast_all, E.RAY, E.RAY_HIT, rec, nbox, rays, capacity, hits, threads)


def spherecast_all(rec, nbox, casts, capacity=None, hits=None, threads=None):
    """The same for nh_spherecast_all (`casts`: E.SPHERE_CAST)."""
    return H.batch(lib().hc_spherecast_all, E.SPHERE_CAST, E.RAY_HIT, rec, nbox, casts, capacity, hits, threads)
