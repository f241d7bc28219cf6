"""Joint rates on the landed config-2 world (include/nudge_hip.h, "joints"): nh_joints_prepare, nh_joint_connections, nh_joints_setup and
nh_joints_apply on chains of rods and ropes laid over the landed boxes, beside the call-by-call step of the same world without and with them.

    the list   the dynamic bodies in index order, cut into assemblies of --links bodies; inside an assembly body k is tied to body k + 1 by a DISTANCE
               joint between the centres: every third a rod of the landed distance, the others ropes with 5 % slack (dead rows).  Listed link by
               link (levels = links - 1) or, with --split, even links first (two levels).  --joints bounds the list (0: every body).
    the world  the landed world's state in a second World without NH_FLAG_FUSED_STEP (joints follow every contact apply there), stepped through the
               eight calls; rates.landed's own world is the fused one that lands it.
    timed      ms per call as the best (and median) of --reps blocks of --inner calls after a warm-up, by device events around the block: prepare,
               connections, setup, apply(1), apply(8); step(1) through the eight calls and step_joints(1), for scale.  Setup and apply change the
               momentum they read: the world is not stepped between them and the figures are those of a list at work, not of one trajectory.
    checked    momentum and accumulated impulses after one setup and one sweep against the host oracle (tests/hostjoint_util.py), byte for byte.

(On rates.py; not a *_rates.py: it also times the step beside its series.)

    python tools/joints.py [--steps 70] [--links 15] [--split] [--reps 5] [--inner 5] [--out profiles/joint_rates.log]
    (on a GPU box; prints the table, one JSON line at the end, and writes both to --out)
"""
import json

import numpy as np

import rates
from nudge_amd import engine as E           # noqa: E402


def chains(positions, links, limit, split):
    """(joints, offsets) over the bodies 1 .. len(positions)."""
    nb = len(positions)
    first = np.arange(1, nb + 1 - (links - 1), links)
    if limit:
        first = first[:max(1, limit // (links - 1))]
    a = (first[:, None] + np.arange(links - 1)[None, :])
    if split:
        a = np.concatenate([a[:, 0::2], a[:, 1::2]], axis=1)
    a = a.reshape(-1)
    j = np.zeros(len(a), dtype=E.JOINT)
    j["a"], j["b"], j["type"] = a, a + 1, E.NH_JOINT_DISTANCE
    ln = np.linalg.norm(positions[a] - positions[a - 1], axis=1).astype(np.float32)
    rod = np.arange(len(a)) % 3 == 0
    j["p"][:, 0] = np.where(rod, ln, 0.0)
    j["p"][:, 1] = np.where(rod, ln, ln * np.float32(1.05))
    return j, (np.arange(len(first) + 1) * (links - 1)).astype(np.uint32)


def main():
    ap = rates.parser("joint_rates")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--links", type=int, default=15)
    ap.add_argument("--joints", type=int, default=0)
    ap.add_argument("--split", action="store_true")
    a = ap.parse_args()
    import hostjoint_util as HJ
    land = rates.landed(a, build=False)
    log = rates.Log()
    state = land.world.get_bodies()
    land.world.close()
    w = E.World(land.scene, flags=0, max_contacts=6 * land.bodies)
    w.eight_calls = True
    w.set_bodies(transforms=state["transforms"], momentum=state["momentum"], idle=state["idle"])
    jnt, offsets = chains(state["transforms"]["position"][1:].astype(np.float64), a.links, a.joints, a.split)

    def timed(fn):
        return rates.best_median(rates.blocks(w, fn, a.reps, a.inner))

    log.say(f"landed {land.name} world: {land.bodies:,} bodies after {a.steps} steps; {len(jnt):,} joints in {len(offsets) - 1:,} assemblies of {a.links - 1}"
            f"{', even links first' if a.split else ''}; GPU {rates.gpu_name(w)}")
    log.say(f"ms per call: the best (median) of {a.reps} blocks of {a.inner} calls after a warm-up, device events around the block; one box, one run.")
    r = {}
    r["step"] = timed(lambda: w.step(1))
    r["prepare"] = timed(lambda: w.joints_prepare(jnt, offsets))
    status = w.joint_status()
    assert status[0] == 0 and status[1] == len(jnt), status
    w.step_joints(1)
    r["step_joints"] = timed(lambda: w.step_joints(1))
    w.collide()
    r["setup"] = timed(lambda: w.joints_setup())
    r["apply(1)"] = timed(lambda: w.joints_apply(1))
    r["apply(8)"] = timed(lambda: w.joints_apply(8))
    # one setup and one sweep against the serial loop
    w.collide()
    active = w.get_active()
    b = w.get_bodies()
    bd = dict(transforms=b["transforms"], properties=land.scene["body_properties"].copy(), momentum=b["momentum"], idle=b["idle"])
    host = HJ.Host(jnt)
    host.impulses[:] = rates.download(w.joint_impulses[:32 * len(jnt)], E.JOINT_IMPULSE)
    w.joints_setup()
    w.joints_apply(1)
    host.setup(bd, active, time_step=land.scene["params"]["time_step"], **w._joints["params"])
    host.apply(bd, 1)
    assert w.get_bodies()["momentum"].tobytes() == bd["momentum"].tobytes(), "momentum differs from the host oracle"
    assert rates.download(w.joint_impulses[:32 * len(jnt)], E.JOINT_IMPULSE).tobytes() == host.impulses[:len(jnt)].tobytes(), "impulses differ from the host oracle"
    for key, v in r.items():
        log.say(f"  {key:14s} {v[0]:8.3f} ({v[1]:8.3f})")
    log.say(f"  levels {status[2]}, bins {status[3]:,}; momentum and impulses after one setup and one sweep equal the host oracle byte for byte")
    log.say()
    log.say(json.dumps(dict(bodies=land.bodies, joints=len(jnt), levels=status[2], bins=status[3], steps=a.steps, checked=len(jnt),
                            **{key: dict(best_ms=v[0], median_ms=v[1]) for key, v in r.items()})))
    log.write(a.out)
    w.close()


if __name__ == "__main__":
    main()
