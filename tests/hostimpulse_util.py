"""The oracles of nh_impulse_sums / nh_body_impulses / nh_blast_impulses / nh_touch_impulses (include/nudge_hip.h, "body impulses"), twice:
tests/hostoracle/hostimpulse.cpp, which runs the per-item functions of nudge_amd/csrc/nh_impulse.h that the device's lanes run around a serial
std::stable_sort, and an independent numpy implementation -- np.float32 scalars, explicit loops, the header's association -- that shares no code with it.

BODIES are dict(transforms=S.TRANSFORM, properties=S.PROPERTIES, momentum=S.MOMENTUM, idle=uint8) arrays of one length, the body count (the sums need
`transforms` alone).  A LIST is E.BODY_IMPULSE records; `count` stands for the device word (None: the capacity is the count).  An output of sums is
(count, records): `records` holds `capacity` records (capacity=None: exactly the count), written in place into `out` when that is given -- all or none,
the other bytes left as they are."""
import ctypes as C

import numpy as np

import hostlib as H
from nudge_amd import engine as E
from nudge_amd import scenes as S

_U, _P = C.c_uint32, C.c_void_p
_SIG = {
    "hi_impulse_sums": ([_P, _U, _P, _U, _U, _P, _P, _U], None),
    "hi_body_impulses": ([_P, _P, _P, _P, _U, _P, _U, _U, _U], None),
    "hi_blast_impulses": ([_P, _U, _P, _U, _P, _P, _U, _P], None),
    "hi_touch_impulses": ([_P, _U, _U, _P, _P, _P], None),
    "hi_key_bytes": ([_U], _U),
}
lib = H.oracle(_SIG)
F32 = np.float32
NO_BODY = E.NH_IMPULSE_NO_BODY
NONE = 0xFFFFFFFF          # NH_SHAPE_NONE


def records(body, impulse, point=None, flags=None):
    """E.BODY_IMPULSE records; point=None: all at the centre."""
    body = np.asarray(body, dtype=np.uint32).reshape(-1)
    r = np.zeros(len(body), dtype=E.BODY_IMPULSE)
    r["body"], r["impulse"] = body, impulse
    if point is None:
        r["flags"] = E.NH_IMPULSE_AT_CENTRE
    else:
        r["point"] = point
    if flags is not None:
        r["flags"] = flags
    return r


def key_bytes(body_count):
    """The 8-bit passes the device's sort takes for this body count."""
    return int(lib().hi_key_bytes(body_count))


def _ptr(a):
    return H.p(a) if a is not None and len(a) else None


def _out(capacity, out):
    if out is None:
        out = np.zeros(max(capacity, 1), dtype=E.IMPULSE_SUM)
    assert len(out) >= capacity and out.flags.c_contiguous and out.dtype == E.IMPULSE_SUM
    return out


def _list(lst, count):
    lst = np.ascontiguousarray(lst, dtype=E.BODY_IMPULSE)
    return lst, (len(lst) if count is None else count)


# ---- through hostimpulse.cpp ------------------------------------------------------------------------------------------------------------------
def count_sums(transforms, lst, count=None, body_count=None):
    lst, count = _list(lst, count)
    cnt = np.zeros(1, dtype=np.uint32)
    lib().hi_impulse_sums(_ptr(transforms), len(transforms) if body_count is None else body_count, _ptr(lst), count, len(lst), H.p(cnt), None, 0)
    return int(cnt[0])


def sums(transforms, lst, count=None, capacity=None, out=None, body_count=None):
    """nh_impulse_sums: (count, records)."""
    if capacity is None:
        capacity = count_sums(transforms, lst, count, body_count)
    lst, count = _list(lst, count)
    out = _out(capacity, out)
    cnt = np.zeros(1, dtype=np.uint32)
    lib().hi_impulse_sums(_ptr(transforms), len(transforms) if body_count is None else body_count, _ptr(lst), count, len(lst), H.p(cnt),
                          H.p(out) if capacity else None, capacity)
    return int(cnt[0]), out


def apply(bodies, lst, count=None, wake=False):
    """nh_body_impulses: the new (momentum, idle) arrays."""
    lst, count = _list(lst, count)
    t, pr = np.ascontiguousarray(bodies["transforms"], dtype=S.TRANSFORM), np.ascontiguousarray(bodies["properties"], dtype=S.PROPERTIES)
    m, idle = np.array(bodies["momentum"], dtype=S.MOMENTUM, copy=True), np.array(bodies["idle"], dtype=np.uint8, copy=True)
    assert len(t) == len(pr) == len(m) == len(idle)
    lib().hi_body_impulses(_ptr(t), _ptr(pr), _ptr(m), _ptr(idle), len(t), _ptr(lst), count, len(lst), int(bool(wake)))
    return m, idle


def blast(transforms, blasts, offsets, hits, capacity=None, out=None, body_count=None):
    """nh_blast_impulses: `out` (given, or capacity records of zeros) with its first min(offsets[-1], capacity) records written."""
    blasts, offsets = np.ascontiguousarray(blasts, dtype=E.BLAST), np.ascontiguousarray(offsets, dtype=np.uint32)
    hits = np.ascontiguousarray(hits, dtype=E.OVERLAP_HIT)
    capacity = len(hits) if capacity is None else capacity
    assert len(offsets) == len(blasts) + 1 and capacity <= len(hits)
    if out is None:
        out = np.zeros(max(capacity, 1), dtype=E.BODY_IMPULSE)
    assert len(out) >= min(int(offsets[-1]), capacity) and out.dtype == E.BODY_IMPULSE and out.flags.c_contiguous
    lib().hi_blast_impulses(_ptr(transforms), len(transforms) if body_count is None else body_count, _ptr(blasts), len(blasts), H.p(offsets), _ptr(hits),
                            capacity, H.p(out))
    return out


def touch(pushes, k, counts, touches, out=None):
    """nh_touch_impulses: len(pushes) x k records."""
    pushes, counts = np.ascontiguousarray(pushes, dtype=E.PUSH), np.ascontiguousarray(counts, dtype=np.uint32)
    touches = np.ascontiguousarray(touches, dtype=E.TOUCH).reshape(-1)
    n = len(pushes)
    assert len(counts) == n and len(touches) == n * k
    if out is None:
        out = np.zeros(max(n * k, 1), dtype=E.BODY_IMPULSE)
    assert len(out) >= n * k and out.dtype == E.BODY_IMPULSE and out.flags.c_contiguous
    lib().hi_touch_impulses(_ptr(pushes), n, k, _ptr(counts), _ptr(touches), H.p(out))
    return out


# ---- in numpy, independently ------------------------------------------------------------------------------------------------------------------
def _neg(x):
    """The sign bit inverted (exact, NaNs included)."""
    return (np.array([x], dtype=F32).view(np.uint32) ^ np.uint32(0x80000000)).view(F32)[0]


def _groups(lst, n, body_count):
    """{body: its runs, each a list of record indices, in list order}."""
    groups, last = {}, None
    for i in range(n):
        b = int(lst[i]["body"])
        if not 0 < b < body_count:
            last = None
            continue
        if b != last:
            groups.setdefault(b, []).append([])
        groups[b][-1].append(i)
        last = b
    return groups


def sums_np(transforms, lst, count=None, capacity=None, out=None, flat=False, body_count=None):
    """(count, records) by the header's rules.  flat=True: every sum taken left to right over the body's records in list order -- NOT the
    specification; the batches use it to show that they tell the two associations apart."""
    lst, count = _list(lst, count)
    body_count = len(transforms) if body_count is None else body_count
    groups = _groups(lst, min(count, len(lst)), body_count)
    res = np.zeros(len(groups), dtype=E.IMPULSE_SUM)
    with np.errstate(all="ignore"):
        for k, b in enumerate(sorted(groups)):
            runs = groups[b] if not flat else [[i for run in groups[b] for i in run]]
            total = [F32(0.0)] * 6
            p = transforms[b]["position"]
            for run in runs:
                s = [F32(0.0)] * 6
                for i in run:
                    J = lst[i]["impulse"]
                    T = [F32(0.0)] * 3
                    if not int(lst[i]["flags"]) & E.NH_IMPULSE_AT_CENTRE:
                        r = [F32(lst[i]["point"][c] - p[c]) for c in range(3)]
                        T = [F32(F32(r[1] * J[2]) - F32(r[2] * J[1])), F32(F32(r[2] * J[0]) - F32(r[0] * J[2])), F32(F32(r[0] * J[1]) - F32(r[1] * J[0]))]
                    for c in range(3):
                        s[c] = F32(s[c] + J[c])
                        s[3 + c] = F32(s[3 + c] + T[c])
                total = [F32(total[c] + s[c]) for c in range(6)]
            res[k]["body"], res[k]["count"] = b, sum(len(run) for run in groups[b])
            res[k]["linear"], res[k]["angular"] = total[:3], total[3:]
    if capacity is None:
        capacity = len(res)
    out = _out(capacity, out)
    if len(res) <= capacity:
        out[:len(res)] = res
    return len(res), out


def _world_inertia(q, ii):
    """The solver's six terms of R diag(ii) R^T (nudge.cpp:1142-1163, 4182-4197), every product and sum rounded to fp32, left to right."""
    x, y, z, s = (F32(v) for v in q)
    kx, ky, kz = F32(x + x), F32(y + y), F32(z + z)
    xx, yy, zz = F32(kx * x), F32(ky * y), F32(kz * z)
    xy, xz, yz = F32(kx * y), F32(kx * z), F32(ky * z)
    sx, sy, sz = F32(kx * s), F32(ky * s), F32(kz * s)
    one = F32(1.0)
    c0 = (F32(F32(one - yy) - zz), F32(xy + sz), F32(xz - sy))
    c1 = (F32(xy - sz), F32(F32(one - xx) - zz), F32(yz + sx))
    c2 = (F32(xz + sy), F32(yz - sx), F32(F32(one - xx) - yy))

    def term(a, b):
        return F32(F32(F32(F32(ii[0] * c0[a]) * c0[b]) + F32(F32(ii[1] * c1[a]) * c1[b])) + F32(F32(ii[2] * c2[a]) * c2[b]))
    return dict(xx=term(0, 0), yy=term(1, 1), zz=term(2, 2), xy=term(0, 1), xz=term(0, 2), yz=term(1, 2))


def apply_np(bodies, lst, count=None, wake=False):
    n, res = sums_np(bodies["transforms"], lst, count)
    m, idle = np.array(bodies["momentum"], dtype=S.MOMENTUM, copy=True), np.array(bodies["idle"], dtype=np.uint8, copy=True)
    with np.errstate(all="ignore"):
        for r in res[:n]:
            b = int(r["body"])
            pr, t = bodies["properties"][b], bodies["transforms"][b]
            v = [F32(m[b]["velocity"][c] + F32(r["linear"][c] * pr["mass_inverse"])) for c in range(3)]
            W = _world_inertia(t["rotation"], pr["inertia_inverse"])
            T = r["angular"]
            rows = ((W["xx"], W["xy"], W["xz"]), (W["xy"], W["yy"], W["yz"]), (W["xz"], W["yz"], W["zz"]))
            a = [F32(m[b]["angular_velocity"][c] + F32(F32(F32(row[0] * T[0]) + F32(row[1] * T[1])) + F32(row[2] * T[2]))) for c, row in enumerate(rows)]
            m[b]["velocity"], m[b]["angular_velocity"] = v, a
            if wake:
                idle[b] = 0
    return m, idle


def _nobody():
    r = np.zeros(1, dtype=E.BODY_IMPULSE)[0]
    r["body"] = NO_BODY
    return r


def blast_np(transforms, blasts, offsets, hits, capacity=None, out=None, body_count=None):
    capacity = len(hits) if capacity is None else capacity
    body_count = len(transforms) if body_count is None else body_count
    if out is None:
        out = np.zeros(max(capacity, 1), dtype=E.BODY_IMPULSE)
    count = len(blasts)
    with np.errstate(all="ignore"):
        for j in range(min(int(offsets[count]), capacity) if count else 0):
            seg = min(max(i for i in range(count + 1) if int(offsets[i]) <= j), count - 1)
            b, body = blasts[seg], int(hits[j]["body"])
            o = _nobody()
            if 0 < body < body_count:
                p = transforms[body]["position"]
                r = [F32(p[c] - b["centre"][c]) for c in range(3)]
                d = F32(np.sqrt(F32(F32(F32(r[0] * r[0]) + F32(r[1] * r[1])) + F32(r[2] * r[2]))))
                s = F32(b["strength"] * F32(F32(1.0) - F32(b["falloff"] * F32(d / b["radius"]))))
                if s > 0:
                    direction = [F32(r[c] / d) for c in range(3)] if d > 0 else [F32(0.0), F32(1.0), F32(0.0)]
                    o["point"], o["body"], o["flags"] = p, body, E.NH_IMPULSE_AT_CENTRE
                    o["impulse"] = [F32(direction[c] * s) for c in range(3)]
            out[j] = o
    return out


def touch_np(pushes, k, counts, touches, out=None):
    n = len(pushes)
    touches = np.asarray(touches).reshape(-1)
    if out is None:
        out = np.zeros(max(n * k, 1), dtype=E.BODY_IMPULSE)
    with np.errstate(all="ignore"):
        for i in range(n):
            for j in range(k):
                o = _nobody()
                if j < min(int(counts[i]), k):
                    t, p = touches[i * k + j], pushes[i]
                    h, d, nrm = t["hit"], t["direction"], t["hit"]["normal"]
                    a = _neg(F32(F32(F32(d[0] * nrm[0]) + F32(d[1] * nrm[1])) + F32(d[2] * nrm[2])))
                    phase = int(t["phase"])
                    if (int(h["shape"]) != NONE and int(h["body"]) != 0 and h["t"] > 0 and phase < 32 and (int(p["phases"]) >> phase) & 1 and a > 0):
                        m = F32(p["mass_over_dt"] * a)
                        if p["max_impulse"] < m:
                            m = p["max_impulse"]
                        o["point"] = [F32(t["origin"][c] + F32(d[c] * h["t"])) for c in range(3)]
                        o["impulse"] = [F32(_neg(nrm[c]) * m) for c in range(3)]
                        o["body"], o["flags"] = h["body"], p["flags"]
                out[i * k + j] = o
    return out
