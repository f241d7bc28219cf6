"""Crafted joint lists and jointed worlds, shared by tests/test_cpu_joints.py (the serial oracle against an independent numpy implementation and against
closed forms) and tests/test_gpu_joints.py (the device against the serial oracle, byte for byte), so that the GPU tests cannot pass on lists that miss a
rule.  A SCHEDULE case is (joints, offsets or None, body_count); a WORLD is (scene, joints, offsets or None)."""
import numpy as np

import hostjoint_util as HJ
from nudge_amd import engine as E

NAN = float("nan")


def pairs(ab, kind=HJ.BALL):
    """Joints of one type over (a, b) pairs, anchors half a unit apart so that nothing is degenerate."""
    ab = np.asarray(ab, dtype=np.uint32).reshape(-1, 2)
    j = HJ.joints(len(ab))
    j["a"], j["b"], j["type"] = ab[:, 0], ab[:, 1], kind
    j["anchor_a"], j["anchor_b"] = (0.0, -0.5, 0.0), (0.0, 0.5, 0.0)
    if kind == HJ.DISTANCE:
        j["p"][:, 0], j["p"][:, 1] = 0.5, 1.5
    if kind == HJ.HINGE:
        j["p"][:, 2], j["p"][:, 5] = 1.0, 1.0
    return j


def chain(first, n, kind=HJ.BALL):
    """n links over the bodies first .. first + n, in order."""
    b = np.arange(first, first + n, dtype=np.uint32)
    return pairs(np.stack([b, b + 1], axis=1), kind)


def even_odd(j):
    return np.concatenate([j[0::2], j[1::2]])


def invalid_kinds(body_count):
    """One joint of each invalid kind between two valid ones that share body 1: the invalid ones must not count as predecessors."""
    j = pairs([(1, 2)] + [(1, 3)] * 10 + [(1, 4)])
    j["type"][1], j["type"][2] = 0, 7
    j["flags"][3] = 1
    j["b"][4] = 1
    j["a"][5] = body_count
    j["b"][6] = 0xFFFFFFFF
    for k, (lo, hi) in zip((7, 8, 9, 10), ((2.0, 1.0), (-1.0, 1.0), (NAN, 1.0), (0.0, NAN))):
        j["type"][k] = HJ.DISTANCE
        j["p"][k, :2] = (lo, hi)
    return j


def assemblies(sizes, seed=3, share_body0=True):
    """One assembly per size over bodies of its own: a random graph (every joint between two of the assembly's bodies, or with body 0), types mixed.
    Returns (joints, offsets, body_count)."""
    rng = np.random.default_rng(seed)
    out, off, first = [], [0], 1
    for n in sizes:
        nb = max(2, n // 2 + 1)
        a = rng.integers(first, first + nb, n)
        b = first + (a - first + rng.integers(1, nb, n)) % nb
        if share_body0:
            a = np.where(rng.random(n) < 0.1, 0, a)
        j = pairs(np.stack([a, b], axis=1))
        j["type"] = rng.choice([HJ.BALL, HJ.DISTANCE, HJ.HINGE], n)
        j["p"][:, :2] = np.where((j["type"] == HJ.DISTANCE)[:, None], (0.5, 1.5), j["p"][:, :2])
        out.append(j)
        off.append(off[-1] + n)
        first += nb
    return np.concatenate(out), np.array(off, dtype=np.uint32), first


def schedule_cases():
    cases = {}
    cases["chain in order"] = (chain(1, 12), None, 14)
    cases["chain even then odd"] = (even_odd(chain(1, 12)), None, 14)
    cases["star"] = (pairs([(1, k) for k in range(2, 11)]), None, 11)
    cases["body 0 only"] = (pairs([(0, k) for k in range(1, 8)] + [(k, 0) for k in range(8, 15)]), None, 15)
    cases["invalid kinds"] = (invalid_kinds(5), None, 5)
    cases["empty"] = (HJ.joints(0), None, 4)
    cases["windows"] = assemblies([1, 255, 256, 257, 1024, 3, 0, 700, 600, 11])
    j = chain(1, 1025)
    cases["1025 without offsets"] = (j, None, 1027)
    cases["1025 in one assembly"] = (np.concatenate([chain(1, 5), chain(10, 1025)]), np.array([0, 5, 1030], dtype=np.uint32), 1040)
    two = np.concatenate([chain(1, 256), chain(300, 256)])
    two_shared = two.copy()
    two_shared["b"][300] = 7                      # bin 1 names a body of bin 0
    cases["two bins"] = (two, np.array([0, 256, 512], dtype=np.uint32), 600)
    cases["shared across two bins"] = (two_shared, np.array([0, 256, 512], dtype=np.uint32), 600)
    near = np.concatenate([chain(1, 10), chain(20, 10)])
    near["a"][15] = 4                             # the second assembly of bin 0 names a body of the first
    cases["shared inside one bin"] = (near, np.array([0, 10, 20], dtype=np.uint32), 40)
    base = chain(1, 20)
    cases["offsets descend"] = (base, np.array([0, 12, 8, 20], dtype=np.uint32), 22)
    cases["offsets start late"] = (base, np.array([1, 8, 20], dtype=np.uint32), 22)
    cases["offsets end early"] = (base, np.array([0, 8, 19], dtype=np.uint32), 22)
    cases["offsets end late"] = (base, np.array([0, 8, 21], dtype=np.uint32), 22)
    cases["no assembly"] = (base, np.array([0], dtype=np.uint32), 22)
    return cases


# ---- worlds ------------------------------------------------------------------------------------------------------------------------------------------
def _scatter(n, seed, spacing=3.0):
    """n positions on a grid high above the ground, jittered by non-dyadic amounts."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** 0.5))
    g = np.stack([(np.arange(n) % side) * spacing, np.full(n, 50.0), (np.arange(n) // side) * spacing], axis=1)
    return (g + rng.uniform(-0.3, 0.3, (n, 3))).astype(np.float32)


def _random_joint_fields(j, seed):
    rng = np.random.default_rng(seed)
    n = len(j)
    j["anchor_a"], j["anchor_b"] = rng.uniform(-0.6, 0.6, (n, 3)), rng.uniform(-0.6, 0.6, (n, 3))
    ax = rng.normal(size=(n, 2, 3))
    ax /= np.linalg.norm(ax, axis=2, keepdims=True)
    hinge, rope = j["type"] == HJ.HINGE, j["type"] == HJ.DISTANCE
    j["p"][hinge] = ax.reshape(n, 6)[hinge].astype(np.float32)
    lo = rng.uniform(0.1, 2.0, n).astype(np.float32)
    hi = np.where(rng.random(n) < 0.3, lo, lo + rng.uniform(0.0, 2.0, n).astype(np.float32))
    j["p"][rope, 0], j["p"][rope, 1] = lo[rope], hi[rope]
    return j


def each_type_world(seed=11):
    """Each type against body 0 (both ways round) and between two dynamic bodies; random rotations, velocities and anchors."""
    kinds = (HJ.BALL, HJ.DISTANCE, HJ.HINGE)
    ab = []
    for k in range(3):
        b = 1 + 4 * k
        ab += [(0, b), (b + 1, 0), (b + 2, b + 3)]
    j = pairs(ab)
    j["type"] = np.repeat(kinds, 3)
    nb = 12
    scene = HJ.world(_scatter(nb, seed), rotations=HJ.random_rotations(nb, seed), seed=seed)
    return scene, _random_joint_fields(j, seed), None


def copies_world(copies=300, seed=12):
    """`copies` copies of a 15-joint assembly over 8 bodies each, BALL, HINGE and DISTANCE mixed, some joints to body 0, bodies shared inside an assembly
    only: 4,500 joints in 18 bins whose spans merge about 17 assemblies each."""
    rng = np.random.default_rng(seed)
    local = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (1, 5), (2, 6), (3, 7), (8, 0), (4, 8), (1, 3), (6, 8)]
    kinds = rng.choice([HJ.BALL, HJ.DISTANCE, HJ.HINGE], len(local))
    out = []
    for c in range(copies):
        ab = [(a + 8 * c if a else 0, b + 8 * c if b else 0) for a, b in local]
        j = pairs(ab)
        j["type"] = kinds
        out.append(j)
    j = _random_joint_fields(np.concatenate(out), seed)
    nb = 8 * copies
    scene = HJ.world(_scatter(nb, seed), rotations=HJ.random_rotations(nb, seed), seed=seed, spheres=True)
    return scene, j, np.arange(copies + 1, dtype=np.uint32) * len(local)


def rope_world(links=1024, seed=13, split=False, kind=None):
    """One rope of `links` joints hung from body 0, listed link by link (levels = links) or even links first (two levels)."""
    nb = links
    pos = np.stack([np.arange(nb) * 0.5, np.full(nb, 50.0), np.zeros(nb)], axis=1).astype(np.float32)
    scene = HJ.world(pos, half=0.2, rotations=HJ.random_rotations(nb, seed), seed=seed, spheres=True)
    b = np.arange(links, dtype=np.uint32)
    j = pairs(np.stack([b, b + 1], axis=1))
    rng = np.random.default_rng(seed)
    j["type"] = rng.choice([HJ.BALL, HJ.DISTANCE, HJ.HINGE], links) if kind is None else kind
    j = _random_joint_fields(j, seed)
    return scene, (even_odd(j) if split else j), None


def hanging_world(seed=14):
    """Bodies hung from body 0 by ropes, rods and hinges, high above the ground, anchors met at the start: pendulums that swing for 240 sub-steps."""
    n = 24
    pos = _scatter(n, seed, spacing=4.0)
    scene = HJ.world(pos, half=0.25)
    j = HJ.joints(n)
    j["a"], j["b"] = 0, np.arange(1, n + 1)
    j["type"] = np.resize([HJ.DISTANCE, HJ.DISTANCE, HJ.HINGE, HJ.BALL], n)
    arm = np.array([1.0, 0.75, 0.0], dtype=np.float32)          # the pivot sits up and to the side of the body: it swings
    j["anchor_a"] = pos + arm
    j["anchor_b"] = (0.0, 0.25, 0.0)
    j["anchor_a"][j["type"] != HJ.DISTANCE] = pos[j["type"] != HJ.DISTANCE] + np.array([0.5, 0.25, 0.0], dtype=np.float32)
    j["anchor_b"][j["type"] != HJ.DISTANCE] = (0.5, 0.25, 0.0)
    ln = np.linalg.norm(arm - np.array([0.0, 0.25, 0.0])).astype(np.float32)
    rope = j["type"] == HJ.DISTANCE
    j["p"][rope, 0] = np.where(np.arange(n)[rope] % 8 == 0, ln, 0.0)          # rods and ropes
    j["p"][rope, 1] = ln
    hinge = j["type"] == HJ.HINGE
    j["p"][hinge] = (0.0, 0.0, 1.0, 0.0, 0.0, 1.0)
    return scene, j, None


def chains_world(crates=6, links=5):
    """Crates on chains, resting partly on the ground: per crate `links` small spheres in a chain from body 0 down to a box that stands on the slab."""
    per = links + 1
    n = crates * per
    pos = np.zeros((n, 3), dtype=np.float32)
    half = np.zeros(n, dtype=np.float32)
    ab, anchors = [], []
    top = 1.0 + 0.6 * links          # the pivot: the chain hangs straight and ends at the crate's top face
    for c in range(crates):
        x = 4.0 * c
        crate = 1 + c * per
        pos[c * per] = (x, 0.5, 0.0)
        prev, prev_anchor = 0, (x, top, 0.0)
        for k in range(links):
            b = crate + 1 + k
            pos[b - 1] = (x, top - 0.3 - 0.6 * k, 0.0)
            ab.append((prev, b))
            anchors.append((prev_anchor, (0.0, 0.3, 0.0)))
            prev, prev_anchor = b, (0.0, -0.3, 0.0)
        ab.append((prev, crate))
        anchors.append((prev_anchor, (0.0, 0.5, 0.0)))
    scene = chains_scene(pos, crates, per)
    j = pairs(ab)
    j["anchor_a"] = [a for a, _ in anchors]
    j["anchor_b"] = [b for _, b in anchors]
    j["a"], j["b"] = scene["joint_body"][j["a"]], scene["joint_body"][j["b"]]
    return scene, j, np.arange(crates + 1, dtype=np.uint32) * per


def chains_scene(pos, crates, per):
    """Boxes (the crates, half extent 0.5) and spheres (the links, radius 0.1) in the body order of chains_world, the slab's top at y = 0."""
    from nudge_amd import scenes as S
    n = len(pos)
    is_crate = (np.arange(n) % per) == 0
    bt = S._identity_transforms(n)
    bt["position"] = pos
    st = S._identity_transforms(1)
    st["position"][0] = (0.0, -1.0, 0.0)
    ssz = np.array([[500.0, 1.0, 500.0]], dtype=np.float32)
    sz = np.full((int(is_crate.sum()), 3), 0.5, dtype=np.float32)
    r = np.full(int((~is_crate).sum()), 0.1, dtype=np.float32)
    scene = S._assemble((st, ssz), (bt[is_crate], sz, S._box_properties(sz[:, 0], sz[:, 1], sz[:, 2])), (bt[~is_crate], r, S._sphere_properties(r)),
                        S.DEFAULT_PARAMS, name="chains")
    # _assemble numbers the boxes before the spheres: map the joints' body order onto it
    order = np.concatenate([[0], 1 + np.flatnonzero(is_crate), 1 + np.flatnonzero(~is_crate)])
    scene["joint_body"] = np.argsort(order).astype(np.uint32)          # body index of chains_world's body k
    return scene
