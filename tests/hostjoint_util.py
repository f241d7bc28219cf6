"""The oracles of the joints (include/nudge_hip.h, "joints"), three of them:
tests/hostoracle/hostjoint.cpp, which runs the per-item functions of nudge_amd/csrc/nh_joint.h that the device's lanes run, serially and in the caller's
list order -- the specification; np_prepare, an independent numpy implementation of the level rule that shares no code with it; and Model, a float64
numpy model of the same algorithm (BALL and DISTANCE rows) for the sanity runs.

BODIES are dict(transforms=S.TRANSFORM, properties=S.PROPERTIES, momentum=S.MOMENTUM, idle=uint8) arrays of one length, the body count.  JOINTS are
E.JOINT records, IMPULSES E.JOINT_IMPULSE records of the same length."""
import ctypes as C

import numpy as np

import hostlib as H
from nudge_amd import engine as E
from nudge_amd import scenes as S

_U, _P, _F = C.c_uint32, C.c_void_p, C.c_float
_SIG = {
    "hj_solve_bytes": ([], _U),
    "hj_prepare": ([_P, _U, _P, _U, _U, _P, _P, _P], None),
    "hj_setup": ([_P, _P, _P, _U, _P, _U, _P, _U, _U, _P, _P, _P], None),
    "hj_apply": ([_P, _U, _U, _U, _P, _P, _U], None),
    "hj_connections": ([_P, _U, _U, _P], None),
    "hj_gravity": ([_P, _P, _U, _F, _F, _F, _F], None),
    "hj_advance": ([_P, _P, _P, _P, _U, _F], None),
}
lib = H.oracle(_SIG)
BALL, DISTANCE, HINGE = E.NH_JOINT_BALL, E.NH_JOINT_DISTANCE, E.NH_JOINT_HINGE
ERR_SIZE, ERR_SHARED, ERR_OFFSETS = E.NH_JOINT_ERR_ASSEMBLY_SIZE, E.NH_JOINT_ERR_SHARED_BODY, E.NH_JOINT_ERR_OFFSETS
PARAMS = dict(time_step=1.0 / 120.0, baumgarte=0.2, max_bias=4.0, warm=1.0)


def _ptr(a):
    return H.p(a) if a is not None and len(a) else None


# ---- records ------------------------------------------------------------------------------------------------------------------------------------------
def joints(n):
    return np.zeros(n, dtype=E.JOINT)


def ball(a, b, anchor_a=(0, 0, 0), anchor_b=(0, 0, 0)):
    j = joints(1)
    j["a"], j["b"], j["type"], j["anchor_a"], j["anchor_b"] = a, b, BALL, anchor_a, anchor_b
    return j


def distance(a, b, lo, hi, anchor_a=(0, 0, 0), anchor_b=(0, 0, 0)):
    j = ball(a, b, anchor_a, anchor_b)
    j["type"] = DISTANCE
    j["p"][0, :2] = (lo, hi)
    return j


def hinge(a, b, anchor_a=(0, 0, 0), anchor_b=(0, 0, 0), axis_a=(0, 1, 0), axis_b=(0, 1, 0)):
    j = ball(a, b, anchor_a, anchor_b)
    j["type"] = HINGE
    j["p"][0, :3], j["p"][0, 3:] = axis_a, axis_b
    return j


def params(**kw):
    p = dict(PARAMS)
    p.update(kw)
    return E.JointParams(p["time_step"], p["baumgarte"], p["max_bias"], p["warm"])


def bodies_of(scene):
    """The BODIES of a scene (copies)."""
    return dict(transforms=scene["body_transforms"].copy(), properties=scene["body_properties"].copy(), momentum=scene["body_momentum"].copy(),
                idle=scene["idle_counters"].copy())


def world(positions, half=0.25, spheres=False, rotations=None, seed=None, ground_y=-1000.0):
    """A scene of one dynamic box (or sphere) per position high above a ground slab at `ground_y`: bodies 1 .. n in the order given.  seed: random
    velocities and angular velocities in [-1, 1] (non-dyadic), None: at rest."""
    positions = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
    n = len(positions)
    bt = S._identity_transforms(n)
    bt["position"] = positions
    if rotations is not None:
        bt["rotation"] = rotations
    st = S._identity_transforms(1)
    st["position"][0] = (0.0, ground_y, 0.0)
    ssz = np.array([[500.0, 1.0, 500.0]], dtype=np.float32)
    none = (S._identity_transforms(0), np.zeros(0, np.float32), np.zeros(0, S.PROPERTIES))
    if spheres:
        r = np.full(n, half, dtype=np.float32)
        scene = S._assemble((st, ssz), (S._identity_transforms(0), np.zeros((0, 3), np.float32), np.zeros(0, S.PROPERTIES)), (bt, r, S._sphere_properties(r)),
                            S.DEFAULT_PARAMS, name="joints")
    else:
        sz = np.full((n, 3), half, dtype=np.float32)
        scene = S._assemble((st, ssz), (bt, sz, S._box_properties(sz[:, 0], sz[:, 1], sz[:, 2])), none, S.DEFAULT_PARAMS, name="joints")
    if seed is not None:
        rng = np.random.default_rng(seed)
        scene["body_momentum"]["velocity"][1:] = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
        scene["body_momentum"]["angular_velocity"][1:] = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    return scene


def random_rotations(n, seed):
    q = np.random.default_rng(seed).normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


# ---- the schedule -----------------------------------------------------------------------------------------------------------------------------------
def prepare(jnt, body_count, offsets=None):
    """hj_prepare: (status (4,), levels, order)."""
    jnt = np.ascontiguousarray(jnt, dtype=E.JOINT)
    n = len(jnt)
    status, levels, order = np.zeros(4, np.uint32), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint32)
    lib().hj_prepare(_ptr(jnt), n, None if off is None else H.p(off), 0 if off is None else len(off) - 1, body_count, H.p(status), H.p(levels), H.p(order))
    return status, levels[:n], order[:n]


def np_valid(jnt, body_count):
    a, b, t = jnt["a"].astype(np.int64), jnt["b"].astype(np.int64), jnt["type"]
    ok = np.isin(t, (BALL, DISTANCE, HINGE)) & (jnt["flags"] == 0) & (a != b) & (a < body_count) & (b < body_count)
    with np.errstate(invalid="ignore"):
        rope = (jnt["p"][:, 0] >= 0) & (jnt["p"][:, 0] <= jnt["p"][:, 1])
    return ok & ((t != DISTANCE) | rope)


def np_prepare(jnt, body_count, offsets=None):
    """The header's rules in numpy and dictionaries, written from the text: (status, levels, order)."""
    jnt = np.ascontiguousarray(jnt, dtype=E.JOINT)
    n = len(jnt)
    status, levels, order = np.zeros(4, np.uint32), np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32)
    if n == 0:
        return status, levels, order
    off = np.array([0, n], dtype=np.int64) if offsets is None else np.asarray(offsets, dtype=np.int64)
    valid = np_valid(jnt, body_count)
    status[1] = valid.sum()
    steps = np.diff(off)
    if off[0] != 0 or off[-1] != n or (steps < 0).any():
        status[0] |= ERR_OFFSETS
    if (steps[steps >= 0] > E.NH_JOINT_ASSEMBLY_MAX).any():
        status[0] |= ERR_SIZE
    if not status[0] & ERR_OFFSETS:
        bin_of = np.zeros(n, dtype=np.int64)
        for i in range(len(off) - 1):
            bin_of[off[i]:off[i + 1]] = off[i] // E.NH_JOINT_BIN
        bins_of_body = {}
        for j in np.flatnonzero(valid):
            for x in (int(jnt["a"][j]), int(jnt["b"][j])):
                if x:
                    bins_of_body.setdefault(x, set()).add(int(bin_of[j]))
        if any(len(s) > 1 for s in bins_of_body.values()):
            status[0] |= ERR_SHARED
    if status[0]:
        return status, levels, order
    for w in np.unique(bin_of):
        span = np.flatnonzero(bin_of == w)
        lev = {}
        names = [(int(jnt["a"][i]), int(jnt["b"][i])) if valid[i] else () for i in span]
        for pos, j in enumerate(span):
            if not valid[j]:
                continue
            best = 0
            for x in set(names[pos]) - {0}:
                for back in range(pos - 1, -1, -1):          # the LAST earlier valid joint of the bin that names x
                    if x in names[back]:
                        best = max(best, lev[span[back]])
                        break
            lev[j] = best + 1
            levels[j] = best + 1
        order[span[0]:span[0] + len(span)] = sorted(span, key=lambda j: (levels[j], j))
        status[3] += 1
    status[2] = levels.max()
    return status, levels, order


# ---- setup, sweeps and the rest of a sub-step through hostjoint.cpp ---------------------------------------------------------------------------------------
class Host:
    """The serial loop over one list: setup() and apply() change `bodies["momentum"]` and `impulses` in place."""

    def __init__(self, jnt, status0=0):
        self.joints = np.ascontiguousarray(jnt, dtype=E.JOINT)
        self.n = len(self.joints)
        self.status0 = int(status0)
        self.solve = np.zeros(max(self.n, 1) * int(lib().hj_solve_bytes()), dtype=np.uint8)
        self.impulses = np.zeros(max(self.n, 1), dtype=E.JOINT_IMPULSE)

    def setup(self, bodies, active, prm=None, **kw):
        prm = params(**kw) if prm is None else prm
        active = np.ascontiguousarray(active, dtype=np.uint32)
        nb = len(bodies["transforms"])
        lib().hj_setup(H.p(bodies["transforms"]), H.p(bodies["properties"]), H.p(bodies["momentum"]), nb, _ptr(active), len(active), _ptr(self.joints), self.n,
                       self.status0, C.byref(prm), H.p(self.impulses), H.p(self.solve))

    def apply(self, bodies, iterations=1):
        lib().hj_apply(H.p(bodies["momentum"]), len(bodies["momentum"]), self.n, self.status0, H.p(self.solve), H.p(self.impulses), iterations)


def connections(jnt, body_count):
    jnt = np.ascontiguousarray(jnt, dtype=E.JOINT)
    out = np.zeros((max(len(jnt), 1), 2), dtype=np.uint32)
    lib().hj_connections(_ptr(jnt), len(jnt), body_count, H.p(out))
    return out[:len(jnt)]


def gravity(bodies, active, time_step, g, damping_rate):
    """The sample's caller-side loop as nh_apply_gravity_damping computes it: g * dt and 1 - dt * rate in fp32."""
    f = np.float32
    active = np.ascontiguousarray(active, dtype=np.uint32)
    lib().hj_gravity(H.p(bodies["momentum"]), _ptr(active), len(active), f(0.0) * f(time_step), f(g) * f(time_step), f(0.0) * f(time_step),
                     f(1.0) - f(time_step) * f(damping_rate))


def advance(bodies, active, time_step):
    active = np.ascontiguousarray(active, dtype=np.uint32)
    lib().hj_advance(H.p(bodies["transforms"]), H.p(bodies["momentum"]), H.p(bodies["idle"]), _ptr(active), len(active), time_step)


def host_steps(bodies, host, steps, iterations, scene_params, prm=None, on_step=None, **kw):
    """`steps` sub-steps of a world WITHOUT contacts, everybody awake: gravity, joint setup, `iterations` sweeps, advance -- World.step_joints with
    every contact call a no-op."""
    active = np.arange(1, len(bodies["transforms"]), dtype=np.uint32)
    dt = scene_params["time_step"]
    for s in range(steps):
        gravity(bodies, active, dt, scene_params["gravity"], scene_params["damping_rate"])
        # (nh_setup_contact_constraints stashes mass_inverse in unused0 of every body, as the reference's does: nudge.cpp:4182-4199)
        bodies["momentum"]["unused0"] = bodies["properties"]["mass_inverse"]
        host.setup(bodies, active, prm, **({} if prm is not None else dict(time_step=dt, **kw)))
        for _ in range(iterations):
            host.apply(bodies, 1)
        advance(bodies, active, dt)
        if on_step:
            on_step(s)


# ---- anchor errors and the float64 model ------------------------------------------------------------------------------------------------------------
def _rot64(q, v):
    u = q[:3]
    t = 2.0 * np.cross(u, v)
    return v + q[3] * t + np.cross(u, t)


def anchor_errors(transforms, jnt):
    """Per joint, in float64: BALL / HINGE |d|, DISTANCE how far the length is outside [min, max]."""
    out = np.zeros(len(jnt))
    for k, j in enumerate(jnt):
        ta, tb = transforms[j["a"]], transforms[j["b"]]
        pa = ta["position"].astype(np.float64) + _rot64(ta["rotation"].astype(np.float64), j["anchor_a"].astype(np.float64))
        pb = tb["position"].astype(np.float64) + _rot64(tb["rotation"].astype(np.float64), j["anchor_b"].astype(np.float64))
        ln = np.linalg.norm(pb - pa)
        out[k] = max(0.0, ln - float(j["p"][1]), float(j["p"][0]) - ln) if j["type"] == DISTANCE else ln
    return out


class Model:
    """The same algorithm in float64 (BALL and DISTANCE rows): gravity, setup with warm start, sweeps in list order, advance."""

    def __init__(self, bodies, jnt, scene_params, **kw):
        self.x = bodies["transforms"]["position"].astype(np.float64)
        self.q = bodies["transforms"]["rotation"].astype(np.float64)
        self.v = bodies["momentum"]["velocity"].astype(np.float64)
        self.w = bodies["momentum"]["angular_velocity"].astype(np.float64)
        self.mi = bodies["properties"]["mass_inverse"].astype(np.float64)
        self.ii = bodies["properties"]["inertia_inverse"].astype(np.float64)
        self.mi[0], self.ii[0] = 0.0, 0.0
        self.joints = jnt
        self.acc = np.zeros((len(jnt), 3))
        self.sp = scene_params
        self.p = dict(PARAMS, time_step=scene_params["time_step"])
        self.p.update(kw)

    def _W(self, b):
        x, y, z, s = self.q[b]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - s * z), 2 * (x * z + s * y)],
                      [2 * (x * y + s * z), 1 - 2 * (x * x + z * z), 2 * (y * z - s * x)],
                      [2 * (x * z - s * y), 2 * (y * z + s * x), 1 - 2 * (x * x + y * y)]])
        return R @ np.diag(self.ii[b]) @ R.T

    def _rows(self, j):
        a, b = int(j["a"]), int(j["b"])
        ra, rb = _rot64(self.q[a], j["anchor_a"].astype(np.float64)), _rot64(self.q[b], j["anchor_b"].astype(np.float64))
        d = (self.x[b] + rb) - (self.x[a] + ra)
        Wa, Wb = self._W(a), self._W(b)
        beta = self.p["baumgarte"] / self.p["time_step"]
        rows = []
        if j["type"] == BALL:
            specs = [(np.eye(3)[k], d[k], -np.inf, np.inf, False) for k in range(3)]
        else:
            ln = np.linalg.norm(d)
            n = d / ln if ln > 0 else np.array([0.0, 1.0, 0.0])
            mn, mx = float(j["p"][0]), float(j["p"][1])
            if mn == mx:
                specs = [(n, ln - mn, -np.inf, np.inf, False)]
            elif ln > mx:
                specs = [(n, ln - mx, -np.inf, 0.0, False)]
            elif ln < mn:
                specs = [(n, ln - mn, 0.0, np.inf, False)]
            else:
                specs = [(n, 0.0, 0.0, 0.0, True)]
        for n, Cc, lo, hi, dead in specs:
            ja, jb = -np.cross(ra, n), np.cross(rb, n)
            wa, wb = Wa @ ja, Wb @ jb
            k = (self.mi[a] + self.mi[b]) + ja @ wa + jb @ wb
            m = 0.0 if dead or not k > 0 else 1.0 / k
            bias = 0.0 if dead else min(max(beta * Cc, -self.p["max_bias"]), self.p["max_bias"])
            rows.append(dict(n=n, ja=ja, jb=jb, wa=wa, wb=wb, m=m, bias=bias, lo=lo, hi=hi, dead=dead))
        return rows

    def _push(self, j, r, delta):
        a, b = int(j["a"]), int(j["b"])
        if a:
            self.v[a] -= r["n"] * (delta * self.mi[a])
            self.w[a] += r["wa"] * delta
        if b:
            self.v[b] += r["n"] * (delta * self.mi[b])
            self.w[b] += r["wb"] * delta

    def step(self, iterations):
        dt, n = self.sp["time_step"], len(self.x)
        damping = 1.0 - dt * self.sp["damping_rate"]
        self.v[1:, 1] -= self.sp["gravity"] * dt
        self.v[1:] *= damping
        self.w[1:] *= damping
        rows = []
        for k, j in enumerate(self.joints):
            rs = self._rows(j)
            for i, r in enumerate(rs):
                self.acc[k, i] = 0.0 if r["dead"] else self.p["warm"] * self.acc[k, i]
                self._push(j, r, self.acc[k, i])
            rows.append(rs)
        for _ in range(iterations):
            for k, j in enumerate(self.joints):
                a, b = int(j["a"]), int(j["b"])
                for i, r in enumerate(rows[k]):
                    jv = r["n"] @ (self.v[b] * (b != 0) - self.v[a] * (a != 0)) + r["ja"] @ (self.w[a] * (a != 0)) + r["jb"] @ (self.w[b] * (b != 0))
                    new = min(max(self.acc[k, i] - (jv + r["bias"]) * r["m"], r["lo"]), r["hi"])
                    self._push(j, r, new - self.acc[k, i])
                    self.acc[k, i] = new
        for b in range(1, n):
            wq = np.array([*self.w[b], 0.0])
            u, s = wq[:3], wq[3]
            qv, qs = self.q[b][:3], self.q[b][3]
            dq = np.array([*(qv * s + u * qs + np.cross(u, qv)), s * qs - u @ qv]) * (0.5 * dt)
            self.x[b] += self.v[b] * dt
            qn = self.q[b] + dq
            self.q[b] = qn / np.linalg.norm(qn)

    def transforms(self):
        t = np.zeros(len(self.x), dtype=[("position", "<f8", 3), ("body", "<u4"), ("rotation", "<f8", 4)])
        t["position"], t["rotation"] = self.x, self.q
        return t
