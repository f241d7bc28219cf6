"""The oracles of nh_contact_pairs / nh_contact_events / nh_step_contact_pairs (include/nudge_hip.h, "contact events"), twice:
tests/hostoracle/hostcontacts.cpp, which runs the per-item functions of nudge_amd/csrc/nh_contact_events.h that the device's lanes run around a serial
std::stable_sort, and an independent numpy implementation -- np.float32 scalars, explicit loops, the header's association -- that shares no code with it.

A CONTACT LIST is dict(data=S.CONTACT records, bodies=(n, 2) uint32, impulses=S.IMPULSE records or None).  A PAIR LIST is (count, records, capacity):
the device word, E.CONTACT_PAIR records (at least `capacity`, or None) and the capacity.  An output is (count, records): `records` holds `capacity`
records (capacity=None: exactly the count), written in place into `out` when that is given -- all or none, the other bytes left as they are."""
import ctypes as C

import numpy as np

import hostlib as H
from nudge_amd import engine as E
from nudge_amd import scenes as S

_U, _P = C.c_uint32, C.c_void_p
_SIG = {
    "hc_contact_pairs": ([_P, _P, _P, _U, _P, _P, _U], None),
    "hc_step_contact_pairs": ([_P, _P, _P, _P, _U, _P, _P, _P, _U, _P, _P, _U], None),
    "hc_contact_events": ([_U, _P, _U, _U, _P, _U, _U, _P, _P, _U, _P, _P, _U], None),
    "hc_bits": ([_U], _U),
}
lib = H.oracle(_SIG)
F32 = np.float32


def contact_list(data, bodies, impulses=None):
    data = np.ascontiguousarray(data, dtype=S.CONTACT)
    bodies = np.ascontiguousarray(bodies, dtype=np.uint32).reshape(-1, 2)
    assert len(data) == len(bodies) and (impulses is None or len(impulses) == len(data))
    return dict(data=data, bodies=bodies, impulses=None if impulses is None else np.ascontiguousarray(impulses, dtype=S.IMPULSE))


def truncated(lst, n):
    return dict(data=lst["data"][:n].copy(), bodies=lst["bodies"][:n].copy(), impulses=None if lst["impulses"] is None else lst["impulses"][:n].copy())


def key_bytes(body_count):
    """The 8-bit passes the device's sort takes for this body_count."""
    return (2 * int(lib().hc_bits(body_count)) + 7) // 8


def _out(capacity, out):
    if out is None:
        out = np.zeros(max(capacity, 1), dtype=E.CONTACT_PAIR)
    assert len(out) >= capacity and out.flags.c_contiguous and out.dtype == E.CONTACT_PAIR
    return out


def _ptr(a):
    return H.p(a) if a is not None and len(a) else None


# ---- through hostcontacts.cpp -----------------------------------------------------------------------------------------------------------------
def count_pairs(lst):
    cnt = np.zeros(1, dtype=np.uint32)
    lib().hc_contact_pairs(_ptr(lst["data"]), _ptr(lst["bodies"]), _ptr(lst["impulses"]), len(lst["data"]), H.p(cnt), None, 0)
    return int(cnt[0])


def pairs(lst, capacity=None, out=None):
    """nh_contact_pairs: (count, records)."""
    if capacity is None:
        capacity = count_pairs(lst)
    out = _out(capacity, out)
    cnt = np.zeros(1, dtype=np.uint32)
    lib().hc_contact_pairs(_ptr(lst["data"]), _ptr(lst["bodies"]), _ptr(lst["impulses"]), len(lst["data"]), H.p(cnt), H.p(out) if capacity else None, capacity)
    return int(cnt[0]), out


def step_pairs(contacts, cache, capacity=None, out=None):
    """nh_step_contact_pairs on what World.get_contacts() and World.get_cache() returned: (count, records)."""
    data, bodies = np.ascontiguousarray(contacts["data"], dtype=S.CONTACT), np.ascontiguousarray(contacts["bodies"], dtype=np.uint32)
    tags, feats = np.ascontiguousarray(contacts["tags"], dtype=np.uint64), np.ascontiguousarray(contacts["features"], dtype=np.uint32)
    ct, cf = np.ascontiguousarray(cache["tags"], dtype=np.uint64), np.ascontiguousarray(cache["features"], dtype=np.uint32)
    cd = np.ascontiguousarray(cache["data"], dtype=S.IMPULSE)
    n, m = contacts["count"], cache["count"]
    args = (_ptr(data), _ptr(bodies), _ptr(tags), _ptr(feats), n, _ptr(ct), _ptr(cf), _ptr(cd), m)
    cnt = np.zeros(1, dtype=np.uint32)
    if capacity is None:
        lib().hc_step_contact_pairs(*args, H.p(cnt), None, 0)
        capacity = int(cnt[0])
    out = _out(capacity, out)
    lib().hc_step_contact_pairs(*args, H.p(cnt), H.p(out) if capacity else None, capacity)
    return int(cnt[0]), out


def events(prev, cur, began_capacity=None, ended_capacity=None, began=None, ended=None):
    """nh_contact_events: ((began count, records), (ended count, records)); prev None: the first frame."""
    def args(lst):
        return (None, 0, 0) if lst is None else (_ptr(lst[1]) if lst[2] else None, lst[0], lst[2])
    cb, ce = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    if began_capacity is None or ended_capacity is None:
        lib().hc_contact_events(int(prev is not None), *args(prev), *args(cur), H.p(cb), None, 0, H.p(ce), None, 0)
        began_capacity = int(cb[0]) if began_capacity is None else began_capacity
        ended_capacity = int(ce[0]) if ended_capacity is None else ended_capacity
    began, ended = _out(began_capacity, began), _out(ended_capacity, ended)
    lib().hc_contact_events(int(prev is not None), *args(prev), *args(cur), H.p(cb), H.p(began) if began_capacity else None, began_capacity,
                            H.p(ce), H.p(ended) if ended_capacity else None, ended_capacity)
    return (int(cb[0]), began), (int(ce[0]), ended)


# ---- in numpy, independently ------------------------------------------------------------------------------------------------------------------
def _dot(v, n):
    return F32(F32(F32(v[0] * n[0]) + F32(v[1] * n[1])) + F32(v[2] * n[2]))


def pairs_np(lst, capacity=None, out=None, flat=False):
    """(count, records) by the header's rules.  flat=True: every sum taken left to right over the pair's contacts in list order -- NOT the
    specification; the batches use it to show that they tell the two associations apart."""
    data, bodies, imp = lst["data"], lst["bodies"], lst["impulses"]
    n = len(data)
    groups = {}          # (lo, hi) -> its runs, each a list of contact indices, in list order
    last = None
    for i in range(n):
        a, b = int(bodies[i, 0]), int(bodies[i, 1])
        key = (min(a, b), max(a, b))
        if key != last:
            groups.setdefault(key, []).append([])
        groups[key][-1].append(i)
        last = key
    records = np.zeros(len(groups), dtype=E.CONTACT_PAIR)
    with np.errstate(all="ignore"):
        for k, key in enumerate(sorted(groups)):
            runs = groups[key] if not flat else [[i for run in groups[key] for i in run]]
            total = [F32(0.0)] * 4
            for run in runs:
                s = [F32(0.0)] * 4
                for i in run:
                    v = imp[i]["impulse"] if imp is not None else np.zeros(3, dtype=F32)
                    nrm = data[i]["normal"]
                    flip = int(bodies[i, 0]) != key[0]
                    d = _dot(v, nrm)
                    for c in range(3):
                        s[c] = F32(s[c] + (F32(-v[c]) if flip else F32(v[c])))
                    s[3] = F32(s[3] + d)
                total = [F32(total[c] + s[c]) for c in range(4)]
            members = [i for run in groups[key] for i in run]
            best = members[0]
            for i in members[1:]:
                if data[i]["penetration"] > data[best]["penetration"]:
                    best = i
            r = records[k]
            r["lo"], r["hi"], r["first"], r["count"] = key[0], key[1], members[0], len(members)
            r["impulse"] = total[:3]
            r["normal_impulse"] = total[3]
            r["position"], r["penetration"], r["deepest"] = data[best]["position"], data[best]["penetration"], best
            r["normal"] = -data[best]["normal"] if int(bodies[best, 0]) != key[0] else data[best]["normal"]
    return _emit(records, capacity, out)


def _emit(records, capacity, out):
    if capacity is None:
        capacity = len(records)
    out = _out(capacity, out)
    if len(records) <= capacity:
        out[:len(records)] = records
    return len(records), out


def events_np(prev, cur, began_capacity=None, ended_capacity=None, began=None, ended=None):
    def keys(lst):
        return [(int(r["lo"]), int(r["hi"])) for r in lst[1][:lst[0]]]
    empty = np.zeros(0, dtype=E.CONTACT_PAIR)
    present = cur[0] <= cur[2] and (prev is None or prev[0] <= prev[2])
    if not present:
        b, e = empty, empty
    elif prev is None:
        b, e = cur[1][:cur[0]], empty
    else:
        kc, kp = keys(cur), keys(prev)
        sc, sp = set(kc), set(kp)
        b = cur[1][[i for i, k in enumerate(kc) if k not in sp]] if kc else empty
        e = prev[1][[i for i, k in enumerate(kp) if k not in sc]] if kp else empty
    return _emit(b, began_capacity, began), _emit(e, ended_capacity, ended)
