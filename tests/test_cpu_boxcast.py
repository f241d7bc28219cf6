"""Box casts on the host (no GPU): the nh_BoxCast record of include/nudge_hip.h against its Python mirrors, and the box-cast arithmetic of
nudge_amd/csrc/nh_query.h -- built for the host by tests/hostcast_util.py, the same bits as the device -- against a float64 model of the same
definition, the named cases of its exact semantics, near-parallel edges and far casts, the ray predicates at size 0 and the overlap predicates at t = 0."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hostcast_util as CAST                 # noqa: E402
import hostoverlap_util as O                 # noqa: E402
import hostquery_util as Q                   # noqa: E402
from cast_util import sweep_box64 as _sweep_box64      # noqa: E402
from query_util import mat as _mat, unit_quats as _unit_quats      # noqa: E402
from nudge_amd import engine as E           # noqa: E402
from nudge_amd import scenes as S           # noqa: E402

NONE = 0xFFFFFFFF
EPS = 2.0 ** -20           # NH_Q_SAT_EPS: the radii of the 15-axis test use |R| + EPS


def test_box_cast_record_matches_the_header(tmp_path):
    """nh_BoxCast: 64 bytes, every member offset as gcc lays it out, the ctypes mirror and the numpy record; its first 32 bytes are nh_Ray's."""
    members = ("origin", "max_t", "direction", "ignore_body", "rotation", "size", "reserved")
    body = "".join(f'  printf("%zu %zu\\n", sizeof(nh_BoxCast), offsetof(nh_BoxCast, {m}));\n' for m in members)
    body += "".join(f'  printf("%zu\\n", offsetof(nh_Ray, {m}));\n' for m in members[:4])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nudge_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    for k, m in enumerate(members):
        size, off = (int(v) for v in lines[k].split())
        assert ctypes.sizeof(E.BoxCast) == size == E.BOX_CAST.itemsize == 64, size
        assert getattr(E.BoxCast, m).offset == off == E.BOX_CAST.fields[m][1], (m, off)
        if k < 4:
            assert int(lines[len(members) + k]) == off == E.RAY.fields[m][1] == getattr(E.Ray, m).offset, m
    assert "nh_boxcast" in E.EXPORTS


# ---- the float64 model: the 15-axis translational SAT of the same definition ------------------------------------------------------------------
def _axes64(o, d, Ra, ha, p, Rb, hb):
    """(s, u, rho, world axis, kind) of the 15 axes in the cast box's frame, exactly degenerate edge axes dropped: over t the axis holds while
    |s - t u| <= rho.  kind: 'face a', 'face b' or 'edge'."""
    R = Ra.T @ Rb
    Ee = np.abs(R) + EPS
    t, u = Ra.T @ (p - o), Ra.T @ d
    out = []
    for k in range(3):
        out.append((t[k], u[k], ha[k] + hb @ Ee[k, :], Ra[:, k], "face a"))
    for k in range(3):
        out.append((t @ R[:, k], u @ R[:, k], ha @ Ee[:, k] + hb[k], Rb[:, k], "face b"))
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        for j in range(3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            L = np.cross(np.eye(3)[i], R[:, j])
            if not L.any():
                continue
            rho = ha[i1] * Ee[i2, j] + ha[i2] * Ee[i1, j] + hb[j1] * Ee[i, j2] + hb[j2] * Ee[i, j1]
            out.append((L @ t, L @ u, rho, np.cross(Ra[:, i], Rb[:, j]), "edge"))
    return out


def _static64(o, Ra, ha, p, Rb, hb):
    return all(abs(s) <= rho for s, _, rho, _, _ in _axes64(o, np.zeros(3), Ra, ha, p, Rb, hb))


def _sweep64(o, d, Ra, ha, p, Rb, hb):
    """(hit, t, normal, kind, t_exit) in float64; kind 'start' for a start overlap."""
    if _static64(o, Ra, ha, p, Rb, hb):
        return True, 0.0, -d / np.linalg.norm(d), "start", np.inf
    te, tx, best = -np.inf, np.inf, None
    for s, u, rho, L, kind in _axes64(o, d, Ra, ha, p, Rb, hb):
        if u == 0.0:
            if abs(s) > rho:
                return False, 0.0, None, None, None
            continue
        lo, hi = sorted(((s - rho) / u, (s + rho) / u))
        if lo > te:
            te, best = lo, (L, u, kind)
        tx = min(tx, hi)
    if best is None or te > tx or tx < 0:
        return False, 0.0, None, None, None
    if te <= 0:
        return True, 0.0, -d / np.linalg.norm(d), "start", tx
    L, u, kind = best
    n = L / np.linalg.norm(L)
    return True, te, (-n if u > 0 else n), kind, tx


def _poses(rng, n, far=(2.0, 10.0)):
    """Random cast boxes aimed near a box at the origin's neighbourhood: (o, d, qa, ha, p, qb, hb) as float32."""
    p = rng.uniform(-5.0, 5.0, size=(n, 3)).astype(np.float32)
    qa, qb = _unit_quats(rng, n), _unit_quats(rng, n)
    ha = rng.uniform(0.2, 2.0, size=(n, 3)).astype(np.float32)
    hb = rng.uniform(0.2, 2.0, size=(n, 3)).astype(np.float32)
    dirn = rng.normal(size=(n, 3))
    dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
    dist = rng.uniform(*far, size=(n, 1)) + 4.0
    o = (p + dirn * dist).astype(np.float32)
    aim = p + rng.normal(scale=1.5, size=(n, 3))
    d = aim - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, size=(n, 1))).astype(np.float32)
    return o, d, qa, ha, p, qb, hb


def _f64(*a):
    return [np.asarray(x, dtype=np.float64) for x in a]


EDGE = 1e-5      # casts whose float64 answer changes (hit / miss, entering axis) when the sizes move by this (relative) are not compared


def test_box_box_sweeps_against_the_float64_model():
    rng = np.random.default_rng(41)
    n = 3000
    o, d, qa, ha, p, qb, hb = _poses(rng, n)
    compared, kinds = 0, {}
    for i in range(n):
        o64, d64, p64, ha64, hb64 = _f64(o[i], d[i], p[i], ha[i], hb[i])
        Ra, Rb = _mat(qa[i]), _mat(qb[i])
        ref = _sweep64(o64, d64, Ra, ha64, p64, Rb, hb64)
        lo = _sweep64(o64, d64, Ra, ha64 * (1 - EDGE), p64, Rb, hb64 * (1 - EDGE))
        hi = _sweep64(o64, d64, Ra, ha64 * (1 + EDGE), p64, Rb, hb64 * (1 + EDGE))
        if not (ref[0] == lo[0] == hi[0] and ref[3] == lo[3] == hi[3]):
            continue
        if ref[0] and ref[3] != "start":
            if not (np.allclose(lo[2], ref[2], atol=1e-9) and np.allclose(hi[2], ref[2], atol=1e-9)):
                continue            # (the entering axis changes with the sizes)
            if max(abs(lo[1] - ref[1]), abs(hi[1] - ref[1])) > 1e-3 * max(ref[1], 1.0):
                continue
        t, nn, hit = CAST.sweep_box_box(o[i], d[i], qa[i], ha[i], p[i], qb[i], hb[i])
        compared += 1
        assert hit == ref[0], (i, hit, ref)
        if not hit:
            continue
        kinds[ref[3]] = kinds.get(ref[3], 0) + 1
        assert abs(t - ref[1]) <= 1e-5 * max(abs(ref[1]), 1.0), (i, ref[3], t, ref[1])
        assert abs(np.linalg.norm(nn.astype(np.float64)) - 1.0) <= 1e-6, (i, nn)
        assert np.abs(nn - ref[2]).max() <= 1e-5, (i, ref[3], nn, ref[2])
        if ref[3] != "start":
            assert nn.astype(np.float64) @ d64 < 0.0
            # the float64 model cross-checked by its own static SAT: separated just before t, overlapping just after
            if ref[4] - ref[1] > 2e-7 * max(ref[1], 1.0):
                dt = 1e-7 * max(ref[1], 1.0)
                assert not _static64(o64 + (ref[1] - dt) * d64, Ra, ha64, p64, Rb, hb64), i
                assert _static64(o64 + (ref[1] + dt) * d64, Ra, ha64, p64, Rb, hb64), i
    assert compared > 0.97 * n, compared
    assert all(kinds.get(k, 0) > 30 for k in ("face a", "face b", "edge")), kinds


def test_the_float64_model_by_bisection_of_its_static_test():
    """The interval solution is the first touch: bisect the static 15-axis test along the sweep and land on the same t."""
    rng = np.random.default_rng(42)
    o, d, qa, ha, p, qb, hb = _poses(rng, 400)
    checked = 0
    for i in range(len(o)):
        o64, d64, p64, ha64, hb64 = _f64(o[i], d[i], p[i], ha[i], hb[i])
        Ra, Rb = _mat(qa[i]), _mat(qb[i])
        ref = _sweep64(o64, d64, Ra, ha64, p64, Rb, hb64)
        if not ref[0] or ref[3] == "start" or ref[4] - ref[1] < 1e-3:
            continue
        a, b = 0.0, ref[1] + 0.5 * (ref[4] - ref[1])          # separated at a, overlapping at b
        for _ in range(80):
            m = 0.5 * (a + b)
            if _static64(o64 + m * d64, Ra, ha64, p64, Rb, hb64):
                b = m
            else:
                a = m
        assert abs(b - ref[1]) <= 1e-9 * max(ref[1], 1.0), (i, b, ref[1])
        checked += 1
    assert checked > 100, checked


def _qaxis(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    s = np.sin(angle / 2)
    return np.array([axis[0] * s, axis[1] * s, axis[2] * s, np.cos(angle / 2)])


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def _near_parallel_case(rng, angle, dist, upright):
    if upright:         # boxes standing upright with a yaw, as in scenes.grid_tiles: the vertical edges are parallel, the others `angle` apart
        y = rng.uniform(0, 2 * np.pi)
        qb = _qaxis((0, 1, 0), y)
        qa = _qaxis((0, 1, 0), y + angle * rng.choice([-1.0, 1.0]))
    else:
        qb = _unit_quats(rng, 1)[0].astype(np.float64)
        qa = _qmul(_qaxis(rng.normal(size=3), angle), qb)
    qa, qb = qa.astype(np.float32), qb.astype(np.float32)
    hb = rng.uniform(0.3, 2.0, size=3).astype(np.float32)
    ha = rng.uniform(0.3, 2.0, size=3).astype(np.float32)
    p = rng.uniform(-50.0, 50.0, size=3).astype(np.float32)
    dirn = rng.normal(size=3)
    if upright:
        dirn[1] *= 0.1
    dirn /= np.linalg.norm(dirn)
    o = (p + dirn * dist).astype(np.float32)
    aim = p + rng.uniform(-0.5, 0.5, size=3) * hb            # (the centre's path crosses the collider: a hit with room to spare)
    d = (aim - o) / dist * rng.uniform(0.5, 2.0)
    return o, d.astype(np.float32), qa, ha, p, qb, hb


def test_near_parallel_edges_and_far_casts_never_miss():
    rng = np.random.default_rng(43)
    hits = 0
    for k in range(3000):
        angle = 10.0 ** rng.uniform(-7, -3)
        dist = 10.0 ** rng.uniform(np.log10(2.0), np.log10(5000.0))
        o, d, qa, ha, p, qb, hb = _near_parallel_case(rng, angle, dist, upright=k % 2 == 0)
        o64, d64, p64, ha64, hb64 = _f64(o, d, p, ha, hb)
        ref = _sweep64(o64, d64, _mat(qa), ha64, p64, _mat(qb), hb64)
        if not ref[0]:
            continue
        t, nn, hit = CAST.sweep_box_box(o, d, qa, ha, p, qb, hb)
        assert hit, (k, angle, dist, ref[1])
        assert abs(t - ref[1]) <= 1e-5 * max(ref[1], 1.0) + 1e-3 / np.linalg.norm(d64), (k, angle, dist, t, ref[1])
        assert abs(np.linalg.norm(nn.astype(np.float64)) - 1.0) <= 1e-6 and nn.astype(np.float64) @ d64 < 0.0
        hits += 1
    assert hits > 2500, hits


def test_elongated_rolled_bars_near_parallel_are_not_hit_across_a_gap():
    """Long bars rolled about their long axis, one turned 1e-5 .. 1e-3 rad against the other: the near-parallel cross axis is the only one that
    separates them, and its gap grows with the bars' length.  Cast towards the collider, t must be the float64 model's; moving away or sliding along
    from a pose nh_overlap finds free, the cast must not hit at t = 0 when the float64 gap is beyond rounding."""
    rng = np.random.default_rng(48)
    towards = away = 0
    for k in range(2000):
        half = np.float32([10.0 ** rng.uniform(0, np.log10(45.0)), rng.uniform(0.05, 0.3), rng.uniform(0.05, 0.3)])
        roll = rng.uniform(0.2, 1.4)
        qb = _qaxis((1, 0, 0), roll)
        qa = _qmul(_qaxis(rng.normal(size=3) * (0, 1, 1), 10.0 ** rng.uniform(-5, -3)), _qaxis((1, 0, 0), roll))
        qa, qb = qa.astype(np.float32), qb.astype(np.float32)
        Ra, Rb = _mat(qa), _mat(qb)
        n = np.array([0.0, np.cos(rng.uniform(0, 2 * np.pi)), 0.0])
        n[2] = np.sqrt(1.0 - n[1] ** 2) * rng.choice([-1.0, 1.0])      # the offset: a direction across the bars
        ext = np.abs(Ra.T @ n) @ half + np.abs(Rb.T @ n) @ half        # the two supports along it
        gap = rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-5, -1.5)
        p = np.zeros(3, np.float32)
        o = (-(ext + gap) * n + rng.uniform(-0.5, 0.5) * np.array([1.0, 0, 0])).astype(np.float32)
        o64, p64, h64 = _f64(o, p, half)
        # towards the collider from one unit further back
        o_back, d_in = (o - n).astype(np.float32), n.astype(np.float32)
        ref = _sweep64(o_back.astype(np.float64), d_in.astype(np.float64), Ra, h64, p64, Rb, h64)
        t, nn, hit = CAST.sweep_box_box(o_back, d_in, qa, half, p, qb, half)
        assert hit == ref[0], (k, ref)
        if hit and ref[3] != "start":
            towards += 1
            assert abs(t - ref[1]) <= 1e-5 * max(ref[1], 1.0) + 2e-6 * float(half[0]), (k, t, ref[1])
        # moving away, and sliding along the bars, from a start that is free by more than rounding
        if O.box_box(o, qa, half, p, qb, half) or _static64(o64, Ra, h64, p64, Rb, h64) or ref[1] < 1.0 + 1e-4:
            continue
        away += 1
        for d in ((-n).astype(np.float32), np.float32([1, 0, 0]), np.float32([-1, 0, 0])):
            ref = _sweep64(o64, d.astype(np.float64), Ra, h64, p64, Rb, h64)
            t, nn, hit = CAST.sweep_box_box(o, d, qa, half, p, qb, half)
            assert not (hit and t == 0.0), (k, d, gap, ref)
            assert hit == ref[0], (k, d, gap, ref)
    assert towards > 400 and away > 400, (towards, away)


def test_box_against_a_sphere_collider_against_float64():
    rng = np.random.default_rng(44)
    n = 3000
    o, d, qa, ha, c, _, _ = _poses(rng, n)
    R = rng.uniform(0.2, 2.0, size=n).astype(np.float32)
    compared, kinds = 0, {}
    for i in range(n):
        o64, d64, c64, ha64 = _f64(o[i], d[i], c[i], ha[i])
        Ra = _mat(qa[i])
        # the sphere swept by -d against the cast box at rest; the normal from the sphere to the box is the negated one
        ref = _sweep_box64(c64, -d64, float(R[i]), o64, Ra, ha64)
        lo = _sweep_box64(c64, -d64, float(R[i]) * (1 - EDGE), o64, Ra, ha64 * (1 - EDGE))
        hi = _sweep_box64(c64, -d64, float(R[i]) * (1 + EDGE), o64, Ra, ha64 * (1 + EDGE))
        if not (ref[0] == lo[0] == hi[0] and ref[3] == lo[3] == hi[3]):
            continue
        if ref[0] and max(abs(lo[1] - ref[1]), abs(hi[1] - ref[1])) > 1e-3 * max(ref[1], 1.0):
            continue
        t, nn, hit = CAST.sweep_box_sphere(o[i], d[i], qa[i], ha[i], c[i], R[i])
        compared += 1
        assert hit == ref[0], i
        if hit:
            kinds[ref[3]] = kinds.get(ref[3], 0) + 1
            n64 = -d64 / np.linalg.norm(d64) if ref[3] == "start" else -ref[2]
            lever = 1.0 if ref[3] in ("face", "start") else max(1.0, ref[1] * np.linalg.norm(d64) / float(R[i]))
            assert abs(t - ref[1]) <= 1e-5 * max(ref[1], 1.0) and np.abs(nn - n64).max() <= 1e-5 * lever, (i, ref[3], t, ref[1], nn, n64)
    assert compared > 0.97 * n, compared
    assert all(kinds.get(k, 0) > 30 for k in ("face", "edge", "corner")), kinds          # (start overlaps: the test after next)


def test_size_zero_is_the_ray_predicate_bit_for_bit():
    rng = np.random.default_rng(45)
    n = 3000
    o, d, _, _, p, qb, hb = _poses(rng, n)
    d[: n // 10, rng.integers(0, 3)] = 0.0          # (zero direction components, the slab's all-or-nothing rule)
    nanq = np.full(4, np.nan, np.float32)
    hits = 0
    for i in range(n):
        for z in ((0.0, 0.0, 0.0), (-0.0, 0.0, -0.0)):
            a, b = CAST.sweep_box_box(o[i], d[i], nanq, z, p[i], qb[i], hb[i]), Q.ray_box(o[i], d[i], p[i], qb[i], hb[i])
            assert a[2] == b[2] and np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes() and a[1].tobytes() == b[1].tobytes(), i
            a, b = CAST.sweep_box_sphere(o[i], d[i], nanq, z, p[i], hb[i, 0]), Q.ray_sphere(o[i], d[i], p[i], hb[i, 0])
            assert a[2] == b[2] and np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes() and a[1].tobytes() == b[1].tobytes(), i
            hits += a[2]
    assert hits > 0.2 * n
    # the same through the brute force: a cast of size 0 writes the ray cast's bytes, whatever its rotation
    rec, nbox = _world(boxes=[(tuple(p[i]), tuple(hb[i]), 1 + i % 5) for i in range(40)], spheres=[(tuple(p[40 + i]), float(hb[40 + i, 0]), 2) for i in range(20)])
    rays = np.zeros(n, dtype=E.RAY)
    rays["origin"], rays["direction"], rays["max_t"], rays["ignore_body"] = o, d, np.inf, NONE
    rays["max_t"][::3] = 6.0
    rays["ignore_body"][::7] = 3
    casts = np.zeros(n, dtype=E.BOX_CAST)
    for k in ("origin", "direction", "max_t", "ignore_body"):
        casts[k] = rays[k]
    casts["rotation"][::2] = np.nan
    assert CAST.cast(CAST.BOX, rec, nbox, casts).tobytes() == CAST.cast(CAST.RAY, rec, nbox, rays).tobytes()


def test_a_start_overlap_under_the_overlap_predicates_hits_at_zero():
    rng = np.random.default_rng(46)
    n = 4000
    ctr = rng.uniform(-2.0, 2.0, size=(n, 3)).astype(np.float32)
    qa, qb = _unit_quats(rng, n), _unit_quats(rng, n)
    ha = rng.uniform(0.05, 1.5, size=(n, 3)).astype(np.float32)
    hb = rng.uniform(0.2, 2.0, size=(n, 3)).astype(np.float32)
    o = rng.uniform(-4.0, 4.0, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    boxes = spheres = 0
    for i in range(n):
        inside = Q.ray_box(o[i], d[i], o[i], (0, 0, 0, 1), (1, 1, 1))[1]          # nh_q_inside(d): the ray's inside rule, bit for bit
        if O.box_box(o[i], qa[i], ha[i], ctr[i], qb[i], hb[i]):
            boxes += 1
            t, nn, hit = CAST.sweep_box_box(o[i], d[i], qa[i], ha[i], ctr[i], qb[i], hb[i])
            assert hit and t == 0.0 and nn.tobytes() == inside.tobytes(), i
        if O.sphere_box(ctr[i], hb[i, 0], o[i], qa[i], ha[i]):
            spheres += 1
            t, nn, hit = CAST.sweep_box_sphere(o[i], d[i], qa[i], ha[i], ctr[i], hb[i, 0])
            assert hit and t == 0.0 and nn.tobytes() == inside.tobytes(), i
    assert boxes > 300 and spheres > 300, (boxes, spheres)


# ---- named cases, through the brute force the GPU tests use as their oracle ---------------------------------------------------------------------
def _world(boxes=(), spheres=(), bodies=None, rotations=None):
    """boxes: (position, half extents, body), spheres: (position, radius, body); bodies at identity, collider transforms carry the positions."""
    nb = 1 + max([b for *_, b in list(boxes) + list(spheres)] + [0]) if bodies is None else bodies
    bt = np.zeros(nb, dtype=S.TRANSFORM)
    bt["rotation"][:, 3] = 1.0
    xt = np.zeros(len(boxes), dtype=S.TRANSFORM)
    xd = np.zeros(len(boxes), dtype=S.BOX)
    for i, (p, h, b) in enumerate(boxes):
        xt[i]["position"], xt[i]["body"], xt[i]["rotation"] = p, b, (0, 0, 0, 1) if rotations is None else rotations[i]
        xd[i]["size"] = h
    st = np.zeros(len(spheres), dtype=S.TRANSFORM)
    sd = np.zeros(len(spheres), dtype=S.SPHERE)
    for i, (p, r, b) in enumerate(spheres):
        st[i]["position"], st[i]["body"], st[i]["rotation"] = p, b, (0, 0, 0, 1)
        sd[i]["radius"] = r
    scene = dict(box_transforms=xt, box_data=xd, box_tags=np.arange(len(boxes), dtype=np.uint32) + 100,
                 sphere_transforms=st, sphere_data=sd, sphere_tags=np.arange(len(spheres), dtype=np.uint32) + 200)
    return Q.records(bt, scene), len(boxes)


def _cast(world, o, d, h, q=(0, 0, 0, 1), max_t=np.inf, ignore=NONE):
    rec, nbox = world
    c = np.zeros(1, dtype=E.BOX_CAST)
    c["origin"], c["direction"], c["size"], c["rotation"], c["max_t"], c["ignore_body"] = o, d, h, q, max_t, ignore
    return CAST.cast(CAST.BOX, rec, nbox, c)[0]


TOL = 1e-5       # the radii carry 2^-20 per term (nh_q_overlap_box_box's): a face-on hit comes a few 1e-6 early


def test_face_on_edge_first_and_corner_first():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 1)])
    h = _cast(w, (0, 0, -6), (0, 0, 1), (0.5, 0.5, 1.5))                 # faces: t = (6 - 1 - 1.5) / 1
    assert h["shape"] == E.NH_SHAPE_BOX and h["tag"] == 100 and abs(h["t"] - 3.5) <= TOL and np.allclose(h["normal"], (0, 0, -1), atol=1e-6)
    h = _cast(w, (0, 0, -6), (0, 0, 4), (0.5, 0.5, 1.5))                 # the same in units of a longer direction
    assert abs(h["t"] - 3.5 / 4) <= TOL and np.allclose(h["normal"], (0, 0, -1), atol=1e-6)
    s = np.float32(np.sqrt(0.5))
    q45 = (0.0, np.sin(np.pi / 8), 0.0, np.cos(np.pi / 8))               # 45 degrees about y: its edge along y leads
    h = _cast(w, (-6, 0, 0), (1, 0, 0), (0.5, 0.5, 0.5), q45)
    assert abs(h["t"] - (6 - 1 - 0.5 * np.sqrt(2))) <= TOL and np.allclose(h["normal"], (-1, 0, 0), atol=1e-6)      # an edge on a face: the face's normal
    # corner first: the cast box turned so that a corner points along -x (the diagonal (1, 1, 1) onto x)
    v = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    ax = np.cross(v, [-1.0, 0.0, 0.0])
    ang = np.arccos(v @ [-1.0, 0.0, 0.0])
    qc = _qaxis(ax, ang)
    h = _cast(w, (6, 0.2, -0.1), (-1, 0, 0), (0.5, 0.5, 0.5), qc)
    assert abs(h["t"] - (6 - 1 - 0.5 * np.sqrt(3))) <= TOL and np.allclose(h["normal"], (1, 0, 0), atol=1e-6)
    # edge against edge: both turned 45 degrees, about z and about x; the leading edges cross, the normal is their cross product
    qz, qx = _qaxis((0, 0, 1), np.pi / 4), _qaxis((1, 0, 0), np.pi / 4)
    w2 = _world(boxes=[((0, 0, 0), (1, 1, 1), 1)], rotations=[qz])
    h = _cast(w2, (0, -6, 0), (0, 1, 0), (1, 1, 1), qx)
    assert abs(h["t"] - (6 - 2 * np.sqrt(2))) <= TOL and np.allclose(h["normal"], (0, -1, 0), atol=1e-6)


def test_a_face_touching_at_exactly_the_gap():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 1)])
    h = _cast(w, (-6, 1.5, 0), (1, 0, 0), (0.5, 0.5, 0.5))               # sliding along the top face, touching it
    assert h["shape"] == E.NH_SHAPE_BOX and abs(h["t"] - 4.5) <= TOL and np.allclose(h["normal"], (-1, 0, 0), atol=1e-6)
    assert _cast(w, (-6, 1.5001, 0), (1, 0, 0), (0.5, 0.5, 0.5))["shape"] == E.NH_SHAPE_NONE


def test_a_slot_narrower_than_the_box_blocks_it_and_a_wider_one_lets_it_pass():
    w = _world(boxes=[((-2, 0, 0), (1, 1, 1), 1), ((2, 0, 0), (1, 1, 1), 2)])          # faces at x = -1 and x = +1: a slot of 2
    h = _cast(w, (0, 10, 0), (0, -1, 0), (1.1, 0.5, 0.5))
    assert h["shape"] == E.NH_SHAPE_BOX and abs(h["t"] - 8.5) <= TOL and np.allclose(h["normal"], (0, 1, 0), atol=1e-6)
    assert _cast(w, (0, 10, 0), (0, -1, 0), (0.9, 0.5, 0.5))["shape"] == E.NH_SHAPE_NONE
    h = _cast(w, (0, 10, 0), (0, -1, 0), (0.9, 0.5, 0.9), (0, np.sin(np.pi / 8), 0, np.cos(np.pi / 8)))      # turned 45 degrees about y: 0.9 sqrt(2) > 1
    assert h["shape"] == E.NH_SHAPE_BOX and abs(h["t"] - 8.5) <= TOL


def test_a_non_unit_direction_scales_t():
    rng = np.random.default_rng(47)
    s2 = np.float32(np.sqrt(0.5))
    w = _world(boxes=[((0.3, -0.2, 0.1), (1, 0.7, 1.3), 1), ((-3, 2, 1), (0.5, 0.5, 0.5), 3)], spheres=[((4, 1, 0), 1.1, 2)],
               rotations=[(0, 0, 0, 1), (s2, 0, 0, s2)])
    hits = 0
    for _ in range(300):
        o = rng.uniform(-6, 6, size=3).astype(np.float32)
        aim = np.asarray([(0.3, -0.2, 0.1), (4, 1, 0), (-3, 2, 1)][rng.integers(0, 3)])
        d = (aim + rng.normal(scale=0.8, size=3) - o).astype(np.float32)
        h = rng.uniform(0.05, 1.0, size=3).astype(np.float32)
        q = _unit_quats(rng, 1)[0]
        a, b = _cast(w, o, d, h, q), _cast(w, o, (d * np.float32(2)).astype(np.float32), h, q)
        assert a["shape"] == b["shape"] and a["collider"] == b["collider"]
        if a["shape"] != E.NH_SHAPE_NONE:
            hits += 1
            assert abs(b["t"] * 2 - a["t"]) <= 1e-5 * max(a["t"], 1.0) and np.allclose(a["normal"], b["normal"], atol=1e-5)
    assert hits > 50


def test_start_overlap_max_t_ignore_body_and_ties():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 1), ((0, 0, 6), (1, 1, 1), 2)], spheres=[((0, 0, 3), 0.5, 1)])
    h = _cast(w, (0, 0, -1.25), (0, 0, 2), (0.5, 0.5, 0.5))                             # overlapping at t = 0
    assert h["t"] == 0.0 and h["collider"] == 0 and np.array_equal(h["normal"], np.float32([0, 0, -1]))
    h = _cast(w, (0, 0, -5), (0, 0, 1), (0.5, 0.5, 0.5), max_t=0.0)
    assert h["shape"] == E.NH_SHAPE_NONE and h["t"] == 0.0 and h["body"] == NONE and np.array_equal(h["normal"], np.zeros(3, np.float32))
    t = _cast(w, (0, 0, -5), (0, 0, 1), (0.5, 0.5, 0.5))["t"]
    assert _cast(w, (0, 0, -5), (0, 0, 1), (0.5, 0.5, 0.5), max_t=t)["t"] == t                                            # t == max_t counts
    assert _cast(w, (0, 0, -5), (0, 0, 1), (0.5, 0.5, 0.5), max_t=np.nextafter(np.float32(t), np.float32(0)))["shape"] == E.NH_SHAPE_NONE
    assert _cast(w, (0, 0, -5), (0, 0, -1), (0.5, 0.5, 0.5))["t"] == np.inf                                              # moving away
    h = _cast(w, (0, 0, -5), (0, 0, 1), (0.5, 0.5, 0.5), ignore=1)                     # the first box and the sphere are body 1's
    assert h["body"] == 2 and h["collider"] == 1 and abs(h["t"] - 9.5) <= TOL
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 3), ((0, 0, 0), (1, 1, 1), 2), ((0, 0, 0), (1, 1, 1), 1)])
    h = _cast(w, (0.3, 0.2, -5), (0, 0, 1), (0.5, 0.5, 0.5))
    assert h["collider"] == 0 and h["body"] == 3
    assert _cast(w, (0.3, 0.2, -5), (0, 0, 1), (0.5, 0.5, 0.5), ignore=3)["collider"] == 1
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 2)], spheres=[((0, 0, 0), 1.0, 1)])       # a box and a sphere at the same t (the box by 3 ulp-ish first)
    h = _cast(w, (0, 0, -5), (0, 0, 1), (0.5, 0.5, 0.5))
    assert h["shape"] == E.NH_SHAPE_BOX
    assert _cast(w, (0, 0, -5), (0, 0, 1), (0.5, 0.5, 0.5), ignore=2)["shape"] == E.NH_SHAPE_SPHERE


def test_a_collider_of_a_missing_body_is_never_hit_and_invalid_casts_are_nan_misses():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 5)], spheres=[((0, 0, 3), 1.0, 5)], bodies=2)
    assert _cast(w, (0, 0, -5), (0, 0, 1), (0.5, 0.5, 0.5))["shape"] == E.NH_SHAPE_NONE
    assert _cast(w, (0, 0, -0.5), (0, 0, 1), (0.5, 0.5, 0.5))["shape"] == E.NH_SHAPE_NONE
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 1)])
    good = ((0, 0, -5), (0, 0, 1), (0.5, 0.5, 0.5), (0, 0, 0, 1))
    bad = [((np.nan, 0, -5),) + good[1:], (good[0], (0, np.inf, 1)) + good[2:], good[:2] + ((0.5, np.inf, 0.5), good[3]),
           good[:2] + ((0.5, 0.5, np.nan), good[3]), good[:2] + ((0.5, -0.25, 0.5), good[3]), good[:2] + ((-0.25, 0.0, 0.0), good[3]),
           good[:3] + ((0, np.nan, 0, 1),), good[:3] + ((np.inf, 0, 0, 1),)]
    for o, d, h, q in bad:
        r = _cast(w, o, d, h, q)
        assert r["shape"] == E.NH_SHAPE_NONE and np.isnan(r["t"]) and r["body"] == NONE and r["collider"] == NONE, (o, d, h, q)
    assert _cast(w, *good)["shape"] == E.NH_SHAPE_BOX
    assert _cast(w, good[0], good[1], (0, 0, 0), (np.nan, 0, 0, 1))["shape"] == E.NH_SHAPE_BOX           # size 0: the rotation is not read


def test_a_zero_direction_touches_at_zero_or_misses():
    w = _world(boxes=[((0, 0, 0), (1, 1, 1), 1)], spheres=[((5, 0, 0), 1.0, 2)])
    h = _cast(w, (0, 0, -1.25), (0, 0, 0), (0.5, 0.5, 0.5))
    assert h["t"] == 0.0 and h["shape"] == E.NH_SHAPE_BOX and np.isnan(h["normal"]).all()
    h = _cast(w, (5, 0, -1.25), (0, 0, 0), (0.5, 0.5, 0.5))
    assert h["t"] == 0.0 and h["shape"] == E.NH_SHAPE_SPHERE and np.isnan(h["normal"]).all()
    assert _cast(w, (0, 0, -3), (0, 0, 0), (0.5, 0.5, 0.5))["shape"] == E.NH_SHAPE_NONE
    assert _cast(w, (5, 1.4, -1.4), (0, 0, 0), (0.5, 0.5, 0.5))["shape"] == E.NH_SHAPE_NONE      # (the box's corner region, beyond the ball)
