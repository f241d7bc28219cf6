"""Spatial partition of one world across ranks: x-slabs, ghost-body halo exchange, migration.

Every rank steps an ordinary world through the C ABI (nudge_amd.engine.World) that holds
    slot 0            the static body with ALL static colliders (replicated: ground slabs / walls are few),
    slots 1..n_owned  the dynamic bodies whose centre lies in the rank's slab [lo, hi)  -- authoritative here,
    the tail          GHOSTS: read-only copies of neighbour-owned bodies that may touch something owned here.
A step is  [halo exchange]  ->  collide .. advance on the local world.  Nothing else crosses ranks: there is no
collective on the data path, only neighbour point-to-point messages (RCCL send/recv over xGMI when the tensors are
on the GPU, gloo on the CPU tests).

The exchange is epoch based so that the per-step cost is three gathers, one message per neighbour and three
contiguous copies:
  * every `epoch` steps (and at step 0) -- REFRESH: bodies whose centre left the slab migrate to the neighbour
    (full record: transform, properties, momentum, idle counter, collider shape / local transform / tag); then every
    rank lists the owned bodies that can reach across a cut within the coming epoch,
        distance to the cut  <  reach(body) + max reach of any body + epoch * dt * speed bound,
    and sends their full records once; both sides remember the list;
  * every step: the dynamic part (position, rotation, momentum, idle counter; 64 B) of the listed bodies is sent, the
    receiver overwrites its ghost slots.  Ghosts are integrated locally as well (they are ordinary bodies to the
    engine) and corrected by the owner's state at the next step.
Contacts between an owned body and a ghost are solved on BOTH ranks, each against its own picture of the other
body's island; the owner's result is the one that survives.  With no cross-cut contacts (drop scenes: config 5)
the partitioned world reproduces the single world exactly up to the broadphase frame; with cross-cut contacts it is
an overlapping-subdomain (Schwarz) Gauss-Seidel -- a valid solver whose result differs from the single-world sweep
in the chaotic regime.  The warm-start cache follows a body for free: it is keyed by collider
tags, and a body is a ghost on the new owner before it migrates there.

`Partition(..., per_iteration=True)` -- for worlds whose contacts DO cross the cuts (piles, pits): the solver runs one sweep at a
time (`apply_impulses(…, 1)`, the reference's own loop, example/main.cpp:314-317) and after every sweep each rank sends the
MOMENTUM (32 B) of the listed bodies again and overwrites its ghosts' momentum with the owner's: both ranks solve a contact that
crosses the cut, but every sweep starts from the owners' values on both sides instead of drifting apart for a whole step
(the per-iteration ghost exchange).  Costs I extra neighbour messages per step; off by default.

`Partition(..., per_iteration=True, single_owner=True)` -- SURVEY 8(e)'s determinism rule: ONE owner per contact.  A contact with the static world belongs to the
rank of its dynamic body; a contact of two dynamic bodies to the rank owning the body whose collider has the LARGER tag (the a > b canonicalisation of
nudge.cpp:2074-2087 / 2131-2132); the engine makes no contact for a pair it does not own (include/nudge_hip.h: nh_set_first_ghost_body; on the reference engine of the
CPU tests the list is filtered between collide and read_cached_impulses).  So the contact lists of the ranks are disjoint and together are the single world's list.
A ghost is then moved only by the contacts owned here, and what they did to it -- momentum now minus momentum at the last exchange, 32 B per ghost -- goes back to
the ghost's owner, which adds it; after that the owners' momentum goes out to the ghosts as before.  Even ranks sweep first, their results travel, then odd ranks
sweep (two exchanges per solver iteration): every contact of the world is then visited once per iteration with everything before it applied, i.e. one Gauss-Seidel
sweep in rank-parity order -- like the engine's colour order a different order than the reference's, same fixed point.  (Both parities sweeping at once would be a
Jacobi step between ranks: a plank held from both sides of a cut gets both supports' full correction and overshoots.)  The warm-start cache of a contact lives on
its owner; when a migration changes the owner the contact starts cold once.

Re-balancing ("move cuts when |count_r - mean| > 5 %"): at every refresh the two ranks on either side of a cut tell each other how many
bodies they own; when the two counts differ by more than 5 % of their sum the HEAVIER one picks the new cut -- the x that hands half the difference (at most
5 % of its bodies per refresh: the capacity slack) to its neighbour -- and sends it over; the bodies between the old cut and the new one then migrate through the
ordinary migration of that same refresh.  Neighbour messages only (two more tiny ones per refresh, one of them only when a cut moves); a cut never moves further
from where it started than the static colliders a rank keeps allow (`split_scene(static_margin=...)`).

A dynamic body carries up to MAX_COLLIDERS colliders (compound bodies: nudge.cpp:3023-3025, 3058-3060), any local transforms; they travel with it in its
record, boxes first, then spheres.  Static colliders are unrestricted.

WHERE THE WORK IS DONE.  `Partition(...)` makes one of two classes that share the arguments, the counters and the step in phases (_PartitionBase).  On the HIP
engine it is a `HipPartition`: every operation -- migration, ghost listing and installation, the collider rebuild, the per-step records, the choice of a new cut --
is a call into the C ABI (include/nudge_hip.h "multi-GPU": nh_partition_*, kernels with device-side counts in nudge_amd/csrc/nh_partition.hip), and the class only
carries message buffers between the library and the transport, exactly like the C++ host examples/partition_rccl.cpp.  `TorchPartition` is the torch implementation
of the same operations on any engine: what the CPU tests run (the compiled reference as the engine, gloo as the transport) and what the GPU tests check the kernels
against (`Partition(..., force_torch=True)`).

Transport is pluggable.  The step protocol -- refresh phases, per-step exchange, per-iteration loop -- is written once (_Cluster) over two primitives, one round of
messages and one vote: `LocalCluster` moves tensors between partitions living in one process (tests, one GPU), `DistCluster` uses torch.distributed point-to-point
ops and a one-word all-reduce (one process per GPU).  The same partition code runs in both.
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

from . import engine as E
from . import scenes as S

MAX_COLLIDERS = 4                                 # colliders a dynamic body may carry across ranks (include/nudge_hip.h: NH_PARTITION_MAX_COLLIDERS)
COLLIDER_BYTES = 16 + 32 + 4 + 4                  # shape, collider transform, tag, pad
FULL_BYTES = 32 + 16 + 32 + MAX_COLLIDERS * COLLIDER_BYTES + 4      # transform, properties, momentum, the colliders (boxes first, then spheres), (boxes, spheres, idle, pad)
STEP_BYTES = 64                                   # position 12, rotation 16, momentum 32, idle 1 + pad (nh_halo_pack's record)


def body_colliders(scene):
    """Per dynamic body its colliders, boxes first (scene order), then spheres: (nbx[B], nsp[B], index[B, 4] into the scene's box / sphere arrays, reach[B]) with
    reach = distance from the body origin to the farthest point of any of its colliders.  Raises when a body carries more than MAX_COLLIDERS."""
    nb = len(scene["body_transforms"])
    counts, index = [], np.zeros((nb, MAX_COLLIDERS), dtype=np.int64)
    reach = np.zeros(nb, dtype=np.float32)
    base = np.zeros(nb, dtype=np.int64)
    for k, (xf, data) in enumerate(((scene["box_transforms"], scene["box_data"]), (scene["sphere_transforms"], scene["sphere_data"]))):
        body = xf["body"].astype(np.int64)
        dyn = np.flatnonzero(body > 0)
        order = dyn[np.argsort(body[dyn], kind="stable")]               # grouped by body, scene order inside a body
        b = body[order]
        cnt = np.bincount(b, minlength=nb)
        first = np.cumsum(cnt) - cnt
        within = np.arange(len(order)) - first[b]
        if len(order) and (base[b] + within >= MAX_COLLIDERS).any():
            raise ValueError(f"partitioned worlds: a dynamic body carries at most {MAX_COLLIDERS} colliders")
        index[b, base[b] + within] = order
        off = np.linalg.norm(xf["position"][order].astype(np.float64), axis=1)
        ext = np.linalg.norm(data["size"][order].astype(np.float64), axis=1) if k == 0 else data["radius"][order].astype(np.float64)
        np.maximum.at(reach, b, (off + ext).astype(np.float32) * np.float32(1.0001))
        counts.append(cnt.astype(np.uint8))
        base = base + cnt
    return counts[0], counts[1], index, reach


def split_scene(scene, cuts, rank, slack=0.15, min_extra=4096, static_margin=None):
    """Rank `rank`'s initial local scene for slabs bounded by `cuts` (ascending x, len = ranks - 1).
    Returns (local_scene, info) where info holds what `Partition` needs besides the engine arrays.
    `static_margin`: keep only the static colliders whose x-extent comes within this distance of the rank's slab or of a
    neighbour's (bodies only ever arrive from a neighbour, and they bring the ground they stand on into reach one slab at a
    time) -- None keeps all of them (small scenes); a rank of the 16 M-box world holds ~500 of the 1984 ground slabs."""
    nbx, nsp, cidx, reach = body_colliders(scene)
    x = scene["body_transforms"]["position"][:, 0]
    lo = -np.inf if rank == 0 else cuts[rank - 1]
    hi = np.inf if rank == len(cuts) else cuts[rank]
    owned = np.flatnonzero((x >= lo) & (x < hi) & (np.arange(len(x)) > 0))
    body_map = np.concatenate([[0], owned]).astype(np.int64)
    n = len(body_map)

    local = dict(name=f"{scene.get('name', 'scene')}/rank{rank}", params=dict(scene["params"]))
    for k in ("body_transforms", "body_properties", "body_momentum", "idle_counters"):
        local[k] = scene[k][body_map].copy()
    local["body_transforms"]["body"] = body_map.astype(np.uint32)          # global id rides in the unused field (nudge.h:36)

    def pick(prefix, k):
        xf = scene[prefix + "_transforms"]
        static = np.flatnonzero(xf["body"] == 0)
        if static_margin is not None and len(static):
            # conservative x-extent of a static collider: centre +- |half extents| (any rotation) or radius
            data = scene[prefix + "_data"][static]
            ext = np.linalg.norm(data["size"].astype(np.float64), axis=1) if k == 0 else data["radius"].astype(np.float64)
            cx = xf["position"][static, 0].astype(np.float64)
            # this slab and both neighbours' (a ghost or migrant arriving from next door may rest on ground beyond the cut)
            lo2 = -np.inf if rank <= 1 else cuts[rank - 2]
            hi2 = np.inf if rank + 1 >= len(cuts) else cuts[rank + 1]
            static = static[(cx + ext >= lo2 - static_margin) & (cx - ext <= hi2 + static_margin)]
        # the dynamic bodies' colliders of this kind in local slot order, a body's own adjacent (what nh_partition_create and the collider rebuild expect / produce)
        cnt = (nbx if k == 0 else nsp)[body_map].astype(np.int64)
        cnt[0] = 0
        slot = np.repeat(np.arange(n), cnt)
        within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + (0 if k == 0 else nbx[body_map].astype(np.int64)[slot])
        sel = np.concatenate([static, cidx[body_map[slot], within]]).astype(np.int64)
        t = xf[sel].copy()
        t["body"][len(static):] = slot.astype(np.uint32)
        return scene[prefix + "_tags"][sel].astype(np.uint32), scene[prefix + "_data"][sel].copy(), t, len(static)

    local["box_tags"], local["box_data"], local["box_transforms"], n_static_box = pick("box", 0)
    local["sphere_tags"], local["sphere_data"], local["sphere_transforms"], n_static_sph = pick("sphere", 1)

    # body-parallel collider description (what travels with a body): per body MAX_COLLIDERS slots, its boxes first, then its spheres
    shape = np.zeros((n, MAX_COLLIDERS, 4), dtype=np.float32)
    cxf = np.zeros((n, MAX_COLLIDERS), dtype=S.TRANSFORM)
    tag = np.zeros((n, MAX_COLLIDERS), dtype=np.uint32)
    lb, ls = nbx[body_map].copy(), nsp[body_map].copy()
    lb[0] = ls[0] = 0
    for c in range(MAX_COLLIDERS):
        isb = np.flatnonzero(c < lb)
        ci = cidx[body_map[isb], c]
        shape[isb, c, :3] = scene["box_data"]["size"][ci]; shape[isb, c, 3] = scene["box_data"]["unused"][ci]
        cxf[isb, c] = scene["box_transforms"][ci]; tag[isb, c] = scene["box_tags"][ci]
        iss = np.flatnonzero((c >= lb) & (c < lb.astype(np.int64) + ls))
        ci = cidx[body_map[iss], c]
        shape[iss, c, 0] = scene["sphere_data"]["radius"][ci]
        cxf[iss, c] = scene["sphere_transforms"][ci]; tag[iss, c] = scene["sphere_tags"][ci]
    extra = max(min_extra, int(slack * n))
    info = dict(rank=rank, ranks=len(cuts) + 1, lo=float(lo), hi=float(hi), n_owned=n - 1, cut_slack=(float("inf") if static_margin is None else 0.5 * float(static_margin)), nbx=lb, nsp=ls, shape=shape, cxf=cxf, tag=tag,
                reach=reach[body_map].copy(), max_reach=float(reach.max()) if len(reach) else 0.0,
                n_static_box=n_static_box, n_static_sph=n_static_sph,
                # (room for `extra` more bodies, with as many colliders each as the world's busiest body carries)
                capacity=dict(bodies=n + extra, boxes=len(local["box_tags"]) + extra * max(1, int(nbx.max()) if len(nbx) else 1),
                              spheres=len(local["sphere_tags"]) + extra * max(1, int(nsp.max()) if len(nsp) else 1)),
                tag_bits=max(8, int(max(int(scene["box_tags"].max()) if len(scene["box_tags"]) else 1,
                                        int(scene["sphere_tags"].max()) if len(scene["sphere_tags"]) else 1)).bit_length()))
    return local, info


class _PartitionBase:
    """What does not depend on who does the work: the arguments and their checks, the engine's record tensors, the counters, the re-balancing rule, the step in phases,
    the 8-byte scalar message and the 64-byte step record.  A subclass brings the refresh_* / step_* / delta_* / momentum_* pack and unpack methods, delta_mark, and what
    the shared messages are made from: _choose_cut(d), _top_speed(), _peer_speeds(peers), _nothing_would_change()."""

    def __init__(self, engine, info, epoch, speed_floor, per_iteration, rebalance, balance_tolerance, single_owner):
        import torch
        self.per_iteration = per_iteration
        # one owner per contact that crosses a cut (module docstring): needs the per-iteration exchange, and an engine that can drop the contacts it does not own
        if single_owner and not per_iteration:
            raise ValueError("single_owner=True needs per_iteration=True")
        if single_owner and not hasattr(engine, "set_first_ghost"):
            raise ValueError("single_owner=True needs an engine with set_first_ghost()")
        self.single_owner = single_owner
        self.hip = None                       # the nh_partition handle (HipPartition only)
        # per-iteration exchange = one apply call per sweep with ghost momentum written in between: the engine must keep its solver states and
        # re-read momentum every call, which NH_FLAG_SINGLE_APPLY (4) / NH_FLAG_FUSED_STEP (8) promise away
        if per_iteration and (getattr(engine, "flags", 0) & (4 | 8)):
            raise ValueError("per_iteration=True needs an engine without NH_FLAG_SINGLE_APPLY / NH_FLAG_FUSED_STEP")
        self.rebalance, self.balance_tolerance = rebalance, balance_tolerance
        self.cut0 = {-1: info["lo"], +1: info["hi"]}            # where the cuts started: they may move by at most cut_slack
        self.cut_slack = info.get("cut_slack", float("inf"))
        self._nb_count = {}
        self.torch = torch
        self.e = engine
        # the engine's optional members, probed once: the HIP kernels for the per-step records, the stream, the per-step book-keeping
        self._halo_pack, self._halo_unpack = getattr(engine, "halo_pack", None), getattr(engine, "halo_unpack", None)
        self._synchronize, self._step_done = getattr(engine, "synchronize", None), getattr(engine, "step_done", None)
        self.rank, self.ranks = info["rank"], info["ranks"]
        self.lo, self.hi = info["lo"], info["hi"]
        self.n_owned = info["n_owned"]
        self.n_static_box, self.n_static_sph = info["n_static_box"], info["n_static_sph"]
        self.max_reach = info["max_reach"]
        self.epoch, self.speed_floor = epoch, speed_floor
        self.quiet_refresh = True             # (switch for A/B and tests: False = every epoch boundary is a refresh, as in rounds 3-5)
        self.dt = float(engine.params["time_step"])
        self.gravity = abs(float(engine.params["gravity"]))
        r = engine.records
        self.bt, self.bp, self.bm, self.bi = r("bt", 32), r("bp", 16), r("bm", 32), r("bi", 1)
        self.xt, self.xd, self.xx = r("xt", 4), r("xd", 16), r("xx", 32)
        self.st, self.sd, self.sx = r("st", 4), r("sd", 4), r("sx", 32)
        self.ghost_in = {-1: 0, +1: 0}             # ghost records received from the left / right neighbour
        self.steps = 0
        # steps_total: every step ever taken (`steps` is the epoch clock, which bench.py rewinds before each timed block -- it cannot be the divisor of step_bytes)
        self.stats = dict(refreshes=0, migrated_out=0, migrated_in=0, ghosts=0, late_bodies=0, step_bytes=0, refresh_bytes=0, cut_moves=0, steps_total=0)

    def close(self):
        pass

    # ---- helpers -------------------------------------------------------------------------------------------------
    def neighbours(self):
        return [d for d in (-1, +1) if 0 <= self.rank + d < self.ranks]

    def _scalar(self, value, dtype):
        """The 8-byte message: one int64 / float64 as a [1, 8] uint8 record."""
        t = self.torch
        return t.tensor([value], dtype=dtype, device=self.bt.device).view(t.uint8).reshape(1, 8)

    def _scalars(self, incoming, dtype):
        """... and what the neighbours sent in that form: {d: value} for every neighbour whose message is not empty."""
        return {d: incoming[d].reshape(-1).view(dtype)[0].item() for d in self.neighbours() if incoming.get(d) is not None and incoming[d].numel()}

    # the 64-byte per-step record (nh_halo_pack's): position 12, rotation 16, momentum 32, idle 1 + pad -- the engine's HIP kernels when it has them, else torch ops
    def _step_records(self, idx, idx32=None):
        """Per-step records [len, 64] of the given body slots."""
        if self._halo_pack is not None:
            return self._halo_pack(idx32 if idx32 is not None else idx.to(self.torch.int32))
        t = self.torch
        pad = t.zeros((len(idx), 4), dtype=t.uint8, device=idx.device)
        pad[:, 0] = self.bi[idx, 0]
        return t.cat([self.bt[idx][:, :12], self.bt[idx][:, 16:], self.bm[idx], pad], dim=1)

    def _step_install(self, at, rec):
        """... written over the bodies in slots [at, at + len): the same bodies as before (the lists only change at a refresh, which announces itself: set_counts)."""
        if self._halo_unpack is not None:
            self._halo_unpack(at, rec.contiguous(), same_bodies=True)
            return
        s = slice(at, at + rec.shape[0])
        self.bt[s, :12] = rec[:, :12]                 # position
        self.bt[s, 16:] = rec[:, 12:28]               # rotation (the `body` field keeps the global id)
        self.bm[s] = rec[:, 28:60]
        self.bi[s, 0] = rec[:, 60]

    # ---- refresh: phase 0 (re-balancing the cuts) ------------------------------------------------------------------
    def balance_pack_counts(self):
        """One 8-byte message per neighbour: how many bodies I own."""
        return {d: self._scalar(self.n_owned, self.torch.int64) for d in self.neighbours()}

    def _moves(self, d):
        """Does the cut towards neighbour d move this refresh, and who picks the new place?  Both sides evaluate the same rule on the same two counts."""
        if not self.rebalance or d not in self._nb_count:
            return None
        mine, theirs = self.n_owned, self._nb_count[d]
        if abs(mine - theirs) <= self.balance_tolerance * max(1, mine + theirs):
            return None
        return "me" if mine > theirs else "neighbour"

    def balance_unpack_counts(self, incoming):
        self._nb_count = self._scalars(incoming, self.torch.int64)

    def balance_expected(self):
        """Rows of the second message I expect from each neighbour (1 when the neighbour is the heavier side of a cut that moves)."""
        return {d: (1 if self._moves(d) == "neighbour" else 0) for d in self.neighbours()}

    def balance_pack_cuts(self):
        """The heavier side of an unbalanced cut picks the x that hands half the difference -- at most 5 % of its bodies -- to the neighbour (_choose_cut)."""
        t = self.torch
        # (the neighbour expects exactly one row from the side that picks, whatever comes out)
        return {d: (self._scalar(self._choose_cut(d), t.float64) if self._moves(d) == "me" else t.zeros((0, 8), dtype=t.uint8, device=self.bt.device)) for d in self.neighbours()}

    def balance_unpack_cuts(self, incoming):
        for d, cut in self._scalars(incoming, self.torch.float64).items():
            self._move_cut(d, cut)

    def _move_cut(self, d, cut):
        if cut != (self.lo if d < 0 else self.hi):
            if d < 0: self.lo = cut
            else: self.hi = cut
            self.stats["cut_moves"] += 1

    # ---- refresh: top speeds across the cuts ---------------------------------------------------------------------
    # A cut's ghost margin is reach + 2 x drift: the two bodies of a cross-cut pair approach each other from BOTH sides, so the drift must come from the top speed on
    # both sides of that cut -- mine (now: before this refresh's migration) and the neighbour's.  One 8-byte message per neighbour, like the body counts.
    # (Round-4 advisor finding: with a rank's own top speed only, a fast body owned by the neighbour reached slow bodies here that this rank had never listed for it and
    # tunnelled through them until the next refresh.  tests/test_partition_cpu.py::test_a_fast_body_from_the_neighbour_finds_its_ghosts)
    def speed_pack(self):
        v = self._top_speed()
        return {d: self._scalar(v, self.torch.float64) for d in self.neighbours()}

    def speed_unpack(self, incoming):
        self._peer_speeds(self._scalars(incoming, self.torch.float64))

    # ---- refresh: is it needed at all?  (round 6) ---------------------------------------------------------------
    def refresh_is_quiet(self):
        """Would a refresh change nothing on this rank?  No owned body beyond a cut, and the bodies within reach of a cut -- at the speeds just exchanged (speed_pack /
        speed_unpack first; nothing is consumed) -- exactly the ones listed for the neighbours at the last refresh, in the same order.  The clusters skip the refresh only
        when EVERY rank says so: the epoch boundary is then a per-step exchange like any other sub-step, and a world at rest stays in its still steps."""
        if not self.quiet_refresh or self.steps == 0 or self.per_iteration:
            return False
        return self._nothing_would_change()

    # ---- every step ---------------------------------------------------------------------------------------------------
    def local_step(self):
        self.e.step(1)
        self.steps += 1
        self.stats["steps_total"] += 1

    # ---- per-iteration mode: the step in phases, ghost momentum refreshed after every sweep ---------------------------
    def step_begin(self):
        e = self.e
        if self.single_owner:
            e.set_first_ghost(self.n_owned + 1)
        e.collide(); e.gravity(); e.read_cache()
        if self.single_owner:
            self.delta_mark()                     # (the warm start inside setup() already moves the ghosts of the contacts owned here)
        e.setup()
        if self.single_owner and self._synchronize is not None:
            self._synchronize()                   # (the HIP engine may defer the warm start into the first apply call, header note 7: it has to be in the momentum the deltas are taken from)

    def sweep(self):
        self.e.apply(1)

    def step_end(self):
        e = self.e
        e.update(); e.write_cache(); e.advance()
        if self._step_done is not None:
            self._step_done()
        self.steps += 1
        self.stats["steps_total"] += 1

    def iterations(self):
        return int(self.e.params["iterations"])

    def needs_refresh(self):
        return self.steps % self.epoch == 0

    # ---- results ------------------------------------------------------------------------------------------------------------
    def owned_state(self):
        """(global ids, transforms, momentum, idle) of the owned bodies, as numpy arrays."""
        n = self.n_owned + 1
        if self._synchronize is not None:
            self._synchronize()
        bt = np.frombuffer(self.bt[1:n].cpu().numpy().tobytes(), dtype=S.TRANSFORM).copy()
        bm = np.frombuffer(self.bm[1:n].cpu().numpy().tobytes(), dtype=S.MOMENTUM).copy()
        bi = self.bi[1:n, 0].cpu().numpy().copy()
        return bt["body"].astype(np.int64), bt, bm, bi


class HipPartition(_PartitionBase):
    """The HIP engine: every operation is ONE call into the C ABI (include/nudge_hip.h "multi-GPU"); this class holds the handle and the message buffers and carries
    them between the library and the transport, exactly like examples/partition_rccl.cpp.  The ghost lists and the body-parallel collider description live in the library."""

    def __init__(self, engine, info, epoch, speed_floor, per_iteration, rebalance, balance_tolerance, single_owner):
        super().__init__(engine, info, epoch, speed_floor, per_iteration, rebalance, balance_tolerance, single_owner)
        t, e = self.torch, self.e
        cap = e.capacity
        inf = float("inf")
        cfg = E.PartitionConfig(self.rank, self.ranks, self.lo if self.lo > -inf else -1e308 * 10, self.hi if self.hi < inf else 1e308 * 10, self.n_owned, self.n_static_box, self.n_static_sph,
                                cap["bodies"], cap["boxes"], cap["spheres"], self.epoch, self.dt, self.gravity, self.speed_floor, self.max_reach,
                                self.cut_slack if self.cut_slack < inf else 1e308 * 10)
        h = C.c_void_p()
        E._check(e.L, e.L.nh_partition_create(C.byref(h), e.ctx, C.byref(cfg), C.byref(e.bodies), C.byref(e.colliders)), "nh_partition_create")
        self.hip = h
        dev = self.bt.device
        self._msg_cap = max(4096, cap["bodies"] // 4)
        self._fullbuf = {d: t.empty((self._msg_cap, FULL_BYTES), dtype=t.uint8, device=dev) for d in (-1, +1)}      # migrants / ghosts out
        self._stepbuf = {d: t.empty((0, STEP_BYTES), dtype=t.uint8, device=dev) for d in (-1, +1)}                  # per-step records out, sized at every refresh
        self._ghost_out_total = 0             # how many of my bodies are listed for the two neighbours together
        self._iter_keep = None                # the last per-iteration message buffers (_call_pair)

    def close(self):
        if self.hip is not None:
            self.e.L.nh_partition_destroy(self.hip)
            self.hip = None

    def _call(self, name, *args):
        E._check(self.e.L, getattr(self.e.L, name)(self.hip, *args), name)

    def _hip_info(self):
        i = E.PartitionInfo()
        self._call("nh_partition_info", C.byref(i))
        self.n_owned = int(i.n_owned)
        self.lo, self.hi = (float(i.lo) if self.rank > 0 else self.lo), (float(i.hi) if self.rank + 1 < self.ranks else self.hi)
        self.stats.update(refreshes=int(i.refreshes), migrated_out=int(i.migrated_out), migrated_in=int(i.migrated_in), cut_moves=int(i.cut_moves),
                          ghosts=int(i.ghost_in[0]) + int(i.ghost_in[1]))
        return i

    def _ghost_out_n(self, d):
        """How many of my bodies are listed for neighbour d (the lists are on the device: nh_partition_info)."""
        return int(self._hip_info().ghost_out[0 if d < 0 else 1])

    def _pack_full(self, name):
        counts = (C.c_uint32 * 2)()
        ptr = lambda d: C.c_void_p(self._fullbuf[d].data_ptr()) if d in self.neighbours() else C.c_void_p(0)      # noqa: E731
        self._call(name, C.byref(self.e.bodies), ptr(-1), ptr(+1), self._msg_cap, C.byref(counts))
        return {d: self._fullbuf[d][:int(counts[0 if d < 0 else 1])] for d in self.neighbours()}

    def _unpack_full_args(self, incoming):
        args = []
        for d in (-1, +1):
            rec = incoming.get(d) if d in self.neighbours() else None
            m = 0 if rec is None else int(rec.shape[0])
            if m:
                rec = rec.contiguous()
                incoming[d] = rec              # (keeps the buffer alive until the kernels have been enqueued behind it)
            args += [C.c_void_p(rec.data_ptr() if m else 0), m]
        return args

    # ---- refresh ------------------------------------------------------------------------------------------------------------
    def _choose_cut(self, d):
        cut = C.c_double(0.0)
        self._call("nh_partition_choose_cut", C.byref(self.e.bodies), d, int(self._nb_count[d]), C.byref(cut))
        if d < 0: self.lo = cut.value
        else: self.hi = cut.value
        self._hip_info()
        return cut.value

    def _move_cut(self, d, cut):
        self._call("nh_partition_set_cut", d, cut)
        super()._move_cut(d, cut)

    def _top_speed(self):
        v = C.c_double(0.0)
        self._call("nh_partition_top_speed", C.byref(self.e.bodies), C.byref(v))
        return float(v.value)

    def _peer_speeds(self, peers):
        self._call("nh_partition_set_peer_speeds", peers.get(-1, 0.0), peers.get(+1, 0.0))

    def _nothing_would_change(self):
        q = C.c_int(0)
        self._call("nh_partition_refresh_is_quiet", C.byref(self.e.bodies), C.byref(q))
        return bool(q.value)

    def refresh_pack_migrants(self):
        return self._pack_full("nh_partition_pack_migrants")

    def refresh_unpack_migrants(self, incoming):
        self._call("nh_partition_unpack_migrants", C.byref(self.e.bodies), *self._unpack_full_args(incoming))
        self._hip_info()

    def refresh_pack_ghosts(self):
        out = self._pack_full("nh_partition_pack_ghosts")
        t = self.torch
        for d in self.neighbours():
            self._stepbuf[d] = t.empty((out[d].shape[0], STEP_BYTES), dtype=t.uint8, device=self.bt.device)
        self._ghost_out_total = sum(int(out[d].shape[0]) for d in self.neighbours())
        return out

    def refresh_unpack_ghosts(self, incoming):
        e = self.e
        self._call("nh_partition_unpack_ghosts", C.byref(e.bodies), C.byref(e.colliders), *self._unpack_full_args(incoming))
        i = self._hip_info()
        self.ghost_in = {-1: int(i.ghost_in[0]), +1: int(i.ghost_in[1])}
        e.nb, e.nbox, e.nsph = int(i.n_bodies), int(i.n_boxes), int(i.n_spheres)         # (the C call has set the counts of the engine's structs and told the context)

    # ---- every step ---------------------------------------------------------------------------------------------------
    def step_pack(self):
        ptr = lambda d: C.c_void_p(self._stepbuf[d].data_ptr()) if d in self.neighbours() and self._stepbuf[d].shape[0] else C.c_void_p(0)      # noqa: E731
        self._call("nh_partition_pack_step", C.byref(self.e.bodies), ptr(-1), ptr(+1))
        out = {d: self._stepbuf[d] for d in self.neighbours()}
        self.stats["step_bytes"] += sum(int(r.numel()) for r in out.values())
        return out

    def step_unpack(self, incoming):
        recs = {d: (incoming[d].contiguous() if self.ghost_in[d] else None) for d in (-1, +1)}
        ptr = lambda d: C.c_void_p(recs[d].data_ptr()) if recs[d] is not None else C.c_void_p(0)      # noqa: E731
        self._call("nh_partition_unpack_step", C.byref(self.e.bodies), ptr(-1), ptr(+1))

    def exchange_step(self):
        """Pack, send / receive, unpack of the per-step records in ONE library call, over the library's own transport (nh_partition_set_transport)."""
        self._call("nh_partition_exchange_step", C.byref(self.e.bodies))
        self.stats["step_bytes"] += STEP_BYTES * self._ghost_out_total

    def library_steps(self, n, exchange_first, loopback_records=0):
        """n sub-steps in ONE library call (nh_partition_step): per-step halo exchanges enqueued by the library over its own transport between them.  Must not reach past
        the next refresh (the caller's business)."""
        self.e.partition_step(self.hip, n, exchange_first, loopback_records)
        self.stats["step_bytes"] += STEP_BYTES * self._ghost_out_total * (n if exchange_first else n - 1)
        self.steps += n
        self.stats["steps_total"] += n

    # ---- per-iteration mode (round 5: nh_partition_mark_ghosts / pack_deltas / unpack_deltas / pack_momentum / unpack_momentum) ----------------------------------
    def _call_pair(self, name, sizes, incoming=None):
        """One of the four pack / unpack entry points: `sizes` records of 32 bytes per side; returns {d: tensor} for a pack."""
        t = self.torch
        dev = self.bt.device
        bufs = {}
        for d in (-1, +1):
            if incoming is None:
                bufs[d] = t.empty((sizes[d], 32), dtype=t.uint8, device=dev) if d in self.neighbours() else None
            else:
                r = incoming.get(d) if d in self.neighbours() else None
                bufs[d] = r.contiguous().to(dev) if (r is not None and sizes[d]) else None
                if bufs[d] is not None:
                    assert bufs[d].numel() == 32 * sizes[d], (name, d, bufs[d].shape, sizes[d])
        ptr = lambda d: C.c_void_p(bufs[d].data_ptr() if (bufs[d] is not None and bufs[d].numel()) else 0)      # noqa: E731
        self._call(name, C.byref(self.e.bodies), ptr(-1), ptr(+1))
        self._iter_keep = bufs                   # (the kernels are enqueued: keep the message tensors alive until the next call)
        if incoming is not None:
            return None
        out = {d: b for d, b in bufs.items() if b is not None}
        self.stats["step_bytes"] += sum(int(v.numel()) for v in out.values())
        return out

    def delta_mark(self):
        self._call("nh_partition_mark_ghosts", C.byref(self.e.bodies))

    def delta_pack(self):
        return self._call_pair("nh_partition_pack_deltas", self.ghost_in)

    def delta_unpack(self, incoming):
        self._call_pair("nh_partition_unpack_deltas", {d: self._ghost_out_n(d) for d in (-1, +1)}, incoming)

    def momentum_pack(self):
        return self._call_pair("nh_partition_pack_momentum", {d: self._ghost_out_n(d) for d in (-1, +1)})

    def momentum_unpack(self, incoming):
        self._call_pair("nh_partition_unpack_momentum", self.ghost_in, incoming)


class TorchPartition(_PartitionBase):
    """The same operations in torch, on any engine: what the CPU tests run (the compiled reference as the engine) and the independent check of the kernels on the GPU
    (`Partition(..., force_torch=True)`).  It keeps the body-parallel collider description and the ghost lists itself."""

    def __init__(self, engine, info, epoch, speed_floor, per_iteration, rebalance, balance_tolerance, single_owner):
        super().__init__(engine, info, epoch, speed_floor, per_iteration, rebalance, balance_tolerance, single_owner)
        torch = self.torch
        dev = self.bt.device
        cap = self.bt.shape[0]
        n = self.n_owned + 1

        def dev_rec(a, width):
            t = torch.zeros((cap, width), dtype=torch.uint8, device=dev)
            raw = np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)
            t[:n] = torch.from_numpy(raw.copy()).to(dev)
            return t

        # body-parallel collider description + reach: MAX_COLLIDERS slots per body (its boxes first, then its spheres)
        self.shape = dev_rec(info["shape"], MAX_COLLIDERS * 16).view(cap, MAX_COLLIDERS, 16)
        self.cxf = dev_rec(info["cxf"], MAX_COLLIDERS * 32).view(cap, MAX_COLLIDERS, 32)
        self.tag = dev_rec(info["tag"], MAX_COLLIDERS * 4).view(cap, MAX_COLLIDERS, 4)
        self.nbx = torch.zeros(cap, dtype=torch.uint8, device=dev)
        self.nbx[:n] = torch.from_numpy(info["nbx"].astype(np.uint8).copy()).to(dev)
        self.nsp = torch.zeros(cap, dtype=torch.uint8, device=dev)
        self.nsp[:n] = torch.from_numpy(info["nsp"].astype(np.uint8).copy()).to(dev)
        self.reach = torch.zeros(cap, dtype=torch.float32, device=dev)
        self.reach[:n] = torch.from_numpy(info["reach"].copy()).to(dev)
        self.n_bodies = n                          # owned + ghosts (+ slot 0)
        self.ghost_out = {-1: None, +1: None}      # owned slots sent to the left / right neighbour every step
        self.ghost_out32 = {-1: None, +1: None}
        self._speed_pre, self._peer_speed = 0.0, {}     # top speeds on my side / the neighbours' side of the cuts, from speed_pack to the next refresh_pack_ghosts
        self._leave = None                         # who migrates away, from refresh_pack_migrants to refresh_unpack_migrants
        self._ghost_ref = None                     # the ghosts' momentum at the last delta_mark()

    # ---- helpers -------------------------------------------------------------------------------------------------
    def _f32(self, rec):
        return rec.view(self.torch.float32)

    def _owned_x(self):
        """(x of slots [0, n_owned], the mask of the owned ones: everything but slot 0)"""
        x = self._f32(self.bt[:self.n_owned + 1])[:, 0]
        return x, self.torch.arange(self.n_owned + 1, device=x.device) > 0

    def _ghost_out_n(self, d):
        """How many of my bodies are listed for neighbour d."""
        return int(len(self.ghost_out[d])) if self.ghost_out.get(d) is not None else 0

    def _full(self, idx):
        """Full records of the given body slots: [len, FULL_BYTES] uint8 (the layout of nh_FullRecord, nudge_amd/csrc/nh_partition.hip)."""
        t = self.torch
        m = len(idx)
        pad = t.zeros((m, 4), dtype=t.uint8, device=idx.device)
        tail = t.zeros((m, 4), dtype=t.uint8, device=idx.device)
        tail[:, 0] = self.nbx[idx]
        tail[:, 1] = self.nsp[idx]
        tail[:, 2] = self.bi[idx, 0]
        parts = [self.bt[idx], self.bp[idx], self.bm[idx]]
        for c in range(MAX_COLLIDERS):
            parts += [self.shape[idx, c], self.cxf[idx, c], self.tag[idx, c], pad]
        return t.cat(parts + [tail], dim=1)

    def _install_full(self, rec, at):
        """Writes full records into body slots [at, at + len)."""
        t = self.torch
        m = rec.shape[0]
        s = slice(at, at + m)
        o = 0
        for dst, w in ((self.bt, 32), (self.bp, 16), (self.bm, 32)):
            dst[s] = rec[:, o:o + w]
            o += w
        for c in range(MAX_COLLIDERS):
            self.shape[s, c] = rec[:, o:o + 16]
            self.cxf[s, c] = rec[:, o + 16:o + 48]
            self.tag[s, c] = rec[:, o + 48:o + 52]
            o += COLLIDER_BYTES
        self.nbx[s] = rec[:, o]
        self.nsp[s] = rec[:, o + 1]
        self.bi[s, 0] = rec[:, o + 2]
        # reach is a function of the colliders: the largest |local offset| + extent
        nb, ns = self.nbx[s].to(t.int64), self.nsp[s].to(t.int64)
        reach = t.zeros(m, dtype=t.float32, device=rec.device)
        for c in range(MAX_COLLIDERS):
            off = self._f32(self.cxf[s, c].contiguous())[:, :3].norm(dim=1)
            sh = self._f32(self.shape[s, c].contiguous())
            ext = t.where(c < nb, sh[:, :3].norm(dim=1), sh[:, 0])
            reach = t.where(c < nb + ns, t.maximum(reach, (off + ext) * 1.0001), reach)
        self.reach[s] = reach

    # ---- refresh ------------------------------------------------------------------------------------------------------------
    def _choose_cut(self, d):
        t = self.torch
        n = self.n_owned
        old = self.lo if d < 0 else self.hi
        cut = old
        if n > 1:
            x = self._owned_x()[0][1:]
            k = max(1, min((n - self._nb_count[d]) // 2, int(0.05 * n), n - 1))
            if d < 0:          # bodies with x < new lo leave: between the k-th and the (k+1)-th smallest x
                a, b = t.kthvalue(x, k).values, t.kthvalue(x, k + 1).values
            else:              # bodies with x >= new hi leave: between the k-th and the (k+1)-th largest x
                a, b = t.kthvalue(x, n - k + 1).values, t.kthvalue(x, n - k).values
            cut = 0.5 * (float(a) + float(b))
            # never further from where the cut started than the static colliders this rank kept allow
            cut = min(max(cut, self.cut0[d] - self.cut_slack), self.cut0[d] + self.cut_slack)
            if not np.isfinite(cut):
                cut = old
        self._move_cut(d, cut)
        return cut

    def _top_speed(self):
        n = self.n_owned + 1
        self._speed_pre = float(self._f32(self.bm[:n])[1:, :3].norm(dim=1).max()) if n > 1 else 0.0
        return self._speed_pre

    def _peer_speeds(self, peers):
        self._peer_speed = peers

    def _leavers(self):
        """(d, mask over slots [0, n_owned]) per neighbour: the owned bodies whose centre is beyond the cut towards d."""
        x, own = self._owned_x()
        for d in self.neighbours():
            yield d, own & ((x < self.lo) if d < 0 else (x >= self.hi))

    def _reaching(self):
        """(d, slots) per neighbour: the owned bodies that can reach across the cut towards d within the coming epoch (module docstring)."""
        t = self.torch
        n = self.n_owned + 1
        x, own = self._owned_x()
        v = self._f32(self.bm[:n])[:, :3].norm(dim=1)
        vmax = float(v[1:].max()) if n > 1 else 0.0
        # how far anything can travel in one epoch: top speed on BOTH sides of the cut (speed_pack / speed_unpack) + free-fall gain, never below the floor
        own_speed = max(vmax, self._speed_pre, self.speed_floor)
        for d in self.neighbours():
            drift = self.epoch * self.dt * (max(own_speed, self._peer_speed.get(d, 0.0)) + self.gravity * self.epoch * self.dt)
            margin = self.reach[:n] + (self.max_reach + 2.0 * drift)
            yield d, t.nonzero(own & ((x - margin < self.lo) if d < 0 else (x + margin >= self.hi))).flatten()

    def _nothing_would_change(self):
        if any(bool(m.any()) for _, m in self._leavers()):
            return False
        for d, idx in self._reaching():
            old = self.ghost_out.get(d)
            if old is None or idx.shape != old.shape or not bool((idx == old).all()):
                return False
        return True

    # phase 1 (migration)
    def refresh_pack_migrants(self):
        out = {}
        self._leave = self.torch.zeros(self.n_owned + 1, dtype=self.torch.bool, device=self.bt.device)
        for d, m in self._leavers():
            idx = self.torch.nonzero(m).flatten()
            out[d] = self._full(idx)
            self._leave |= m
            self.stats["migrated_out"] += int(idx.numel())
        return out

    def refresh_unpack_migrants(self, incoming):
        """Drops the bodies that left, appends the ones that arrived (owned region stays contiguous from slot 1)."""
        t = self.torch
        n = self.n_owned + 1
        keep = t.nonzero(~self._leave).flatten()          # includes slot 0
        if keep.numel() != n:
            for arr in (self.bt, self.bp, self.bm, self.bi, self.shape, self.cxf, self.tag, self.nbx, self.nsp, self.reach):
                arr[:keep.numel()] = arr[keep]
        at = int(keep.numel())
        for d in self.neighbours():
            rec = incoming.get(d)
            if rec is not None and rec.shape[0]:
                if at + rec.shape[0] > self.bt.shape[0]:
                    raise RuntimeError("partition: body capacity exceeded by migration")
                self._install_full(rec, at)
                at += rec.shape[0]
                self.stats["migrated_in"] += int(rec.shape[0])
        self.n_owned = at - 1

    # phase 2 (ghost lists)
    def refresh_pack_ghosts(self):
        out = {}
        for d, idx in self._reaching():
            self.ghost_out[d] = idx
            self.ghost_out32[d] = idx.to(self.torch.int32)
            out[d] = self._full(idx)
        self._speed_pre, self._peer_speed = 0.0, {}
        return out

    def refresh_unpack_ghosts(self, incoming):
        at = self.n_owned + 1
        for d in (-1, +1):
            rec = incoming.get(d) if d in self.neighbours() else None
            m = 0 if rec is None else int(rec.shape[0])
            if at + m > self.bt.shape[0]:
                raise RuntimeError("partition: body capacity exceeded by ghosts")
            if m:
                self._install_full(rec, at)
            self.ghost_in[d] = m
            at += m
        self.n_bodies = at
        self._rebuild_colliders()
        self.stats["refreshes"] += 1
        self.stats["ghosts"] = self.ghost_in[-1] + self.ghost_in[+1]

    def _rebuild_colliders(self):
        """Collider arrays = static colliders, then the dynamic bodies' in slot order (owned, then ghosts), a body's own adjacent."""
        t = self.torch
        n = self.n_bodies
        dev = self.bt.device
        nb, ns = self.nbx[:n].to(t.int64).clone(), self.nsp[:n].to(t.int64).clone()
        nb[0] = 0; ns[0] = 0
        counts = []
        for k, (tags, data, xf, n_static, width, cnt, base) in enumerate(((self.xt, self.xd, self.xx, self.n_static_box, 16, nb, t.zeros_like(nb)),
                                                                          (self.st, self.sd, self.sx, self.n_static_sph, 4, ns, nb))):
            m = int(cnt.sum())
            if n_static + m > tags.shape[0]:
                raise RuntimeError("partition: collider capacity exceeded")
            slot = t.repeat_interleave(t.arange(n, device=dev), cnt)
            within = t.arange(m, device=dev) - t.repeat_interleave(t.cumsum(cnt, 0) - cnt, cnt) + base[slot]
            s = slice(n_static, n_static + m)
            tags[s] = self.tag[slot, within]
            data[s] = self.shape[slot, within][:, :width]
            xf[s] = self.cxf[slot, within]
            xf[s].view(t.int32)[:, 3] = slot.to(t.int32)               # Transform.body = local body slot (nudge.h:36)
            counts.append(n_static + m)
        self.e.set_counts(n, counts[0], counts[1])

    # ---- every step ---------------------------------------------------------------------------------------------------
    def _ghost_slots(self):
        """(d, first slot, count) of the ghosts received from each side: the left neighbour's first."""
        at = self.n_owned + 1
        for d in (-1, +1):
            yield d, at, self.ghost_in[d]
            at += self.ghost_in[d]

    def step_pack(self):
        out = {d: self._step_records(self.ghost_out[d], self.ghost_out32[d]) for d in self.neighbours()}
        self.stats["step_bytes"] += sum(int(rec.numel()) for rec in out.values())
        return out

    def step_unpack(self, incoming):
        for d, at, m in self._ghost_slots():
            if m:
                self._step_install(at, incoming[d])

    # ---- single ownership: what the solver did to a ghost goes back to the ghost's owner ----------------------------------------------
    def _ghost_momentum(self):
        at = self.n_owned + 1
        return self.bm[at:at + self.ghost_in[-1] + self.ghost_in[+1]]

    def delta_mark(self):
        self._ghost_ref = self._ghost_momentum().clone()

    def delta_pack(self):
        """Per neighbour: momentum of its bodies' ghosts here now minus at the last delta_mark() (8 floats per ghost, in the order of the neighbour's list)."""
        t = self.torch
        d = self._ghost_momentum().contiguous().view(t.float32) - self._ghost_ref.contiguous().view(t.float32)
        d[:, 3] = 0.0; d[:, 7] = 0.0              # (the two spare words of a momentum record are the engine's: the inverse mass rides there during a solve, nudge.cpp:4358)
        out, m = {}, self.ghost_in[-1]
        for dirn, part in ((-1, d[:m]), (+1, d[m:])):
            if dirn in self.neighbours():
                out[dirn] = part.contiguous().view(t.uint8)
                self.stats["step_bytes"] += int(out[dirn].numel())
        return out

    def delta_unpack(self, incoming):
        """Adds the neighbours' deltas to the bodies listed for them (ghost_out[d] is the order the neighbour holds their ghosts in)."""
        t = self.torch
        bmf = self.bm.view(t.float32)
        for d in self.neighbours():
            idx = self.ghost_out[d]
            if idx is not None and len(idx):
                bmf.index_add_(0, idx.long(), incoming[d].contiguous().view(t.float32).to(bmf.device))

    def momentum_pack(self):
        out = {d: self.bm[self.ghost_out[d]] for d in self.neighbours()}
        self.stats["step_bytes"] += sum(int(rec.numel()) for rec in out.values())
        return out

    def momentum_unpack(self, incoming):
        for d, at, m in self._ghost_slots():
            if m:
                self.bm[at:at + m] = incoming[d]


def Partition(engine, info, epoch=16, speed_floor=1.0, per_iteration=False, rebalance=True, balance_tolerance=0.05, force_torch=False, single_owner=False):
    """One rank's share of the world.  `engine` exposes the caller-owned arrays as [capacity, record] uint8 torch
    tensors (`records(name, bytes)`), `set_counts(bodies, boxes, spheres)`, `step(n)` and `params` -- nudge_amd.engine.World
    does; the CPU tests plug the oracle in behind the same four members.
    (Round 5: the per-iteration exchange of single ownership is behind the C ABI too, so the HIP engine gets a HipPartition in every mode; force_torch=True keeps the
    torch implementation, the independent check.)"""
    on_the_abi = not force_torch and hasattr(engine, "L") and hasattr(engine, "ctx") and hasattr(engine.L, "nh_partition_create")
    return (HipPartition if on_the_abi else TorchPartition)(engine, info, epoch, speed_floor, per_iteration, rebalance, balance_tolerance, single_owner)


def _merge(states):
    """owned_state() of several partitions merged by global id: dict(ids, transforms, momentum, idle), sorted by id."""
    ids = np.concatenate([q[0] for q in states])
    order = np.argsort(ids, kind="stable")
    return dict(ids=ids[order], transforms=np.concatenate([q[1] for q in states])[order],
                momentum=np.concatenate([q[2] for q in states])[order], idle=np.concatenate([q[3] for q in states])[order])


class _Cluster:
    """The step protocol, once, over the partitions this process holds (`parts`: all of them in a LocalCluster, one in a DistCluster).  A transport brings two
    primitives: _round(name, width, counts) -- `name.format("pack")` on every local partition, deliver, `name.format("unpack")` (the methods are looked up on the
    partition at call time; `width` the record bytes, `counts(p)` the rows expected per neighbour when they are known in advance) -- and _vote(answers): does
    every rank of the job say yes?"""

    def __init__(self, parts):
        self.parts = parts
        self.quiet_refreshes = 0

    def _refresh(self):
        """Counts and cuts (re-balancing), top speeds, the quiet vote, migrants, ghosts.  False: a QUIET refresh -- nobody has crossed a cut, every ghost list would come
        out as it is, on EVERY partition -- and the epoch boundary is a per-step exchange."""
        parts, lead = self.parts, self.parts[0]
        one_row = lambda p: dict.fromkeys(p.neighbours(), 1)      # noqa: E731
        if lead.rebalance and lead.steps > 0:
            self._round("balance_{}_counts", 8, one_row)
            self._round("balance_{}_cuts", 8, lambda p: p.balance_expected())
        self._round("speed_{}", 8, one_row)
        # (the vote is taken whenever a partition here could say yes -- at step 0 too, where every refresh_is_quiet() says no: all ranks of a job must vote or none)
        if any(p.quiet_refresh and not p.per_iteration for p in parts) and self._vote([p.refresh_is_quiet() for p in parts]):
            self.quiet_refreshes += 1
            return False
        self._round("refresh_{}_migrants", FULL_BYTES)
        self._round("refresh_{}_ghosts", FULL_BYTES)
        return True

    def _boundary(self):
        """The start of a step: (is it an epoch boundary, was a refresh made).  Without a refresh the caller owes the ghosts a per-step exchange."""
        boundary = self.parts[0].needs_refresh()
        return boundary, boundary and self._refresh()

    def _step_exchange(self):
        self._round("step_{}", STEP_BYTES, lambda p: p.ghost_in)

    def _iteration_exchange(self):
        single_owner = self.parts[0].single_owner
        if single_owner:                          # ghost deltas to their owners first: the momentum sent back below includes them
            self._round("delta_{}", 32, lambda p: {d: p._ghost_out_n(d) for d in p.neighbours()})
        self._round("momentum_{}", 32, lambda p: p.ghost_in)
        if single_owner:
            for p in self.parts:
                p.delta_mark()

    def _solve(self):
        """Collide .. advance on every local partition: one engine step, or (per_iteration) the step in phases with an exchange after every sweep."""
        parts, lead = self.parts, self.parts[0]
        if not lead.per_iteration:
            for p in parts:
                p.local_step()
            return
        for p in parts:
            p.step_begin()
        if lead.single_owner:
            self._iteration_exchange()            # (the warm start)
        for _it in range(lead.iterations()):
            if lead.single_owner:
                # even ranks sweep, their results travel, odd ranks sweep: with one owner per contact that IS one Gauss-Seidel sweep over all contacts of the
                # world (module docstring); sweeping both parities at once would be a Jacobi step between the ranks, which overshoots on a body held from both sides
                for phase in (0, 1):
                    for p in parts:
                        if p.rank % 2 == phase:
                            p.sweep()
                    self._iteration_exchange()
            else:
                for p in parts:
                    p.sweep()
                self._iteration_exchange()
        for p in parts:
            p.step_end()


class LocalCluster(_Cluster):
    """All partitions in one process (one GPU or the CPU): messages are tensor hand-overs."""

    def _route(self, outs):
        ins = [dict() for _ in self.parts]
        for r, out in enumerate(outs):
            for d, rec in out.items():
                ins[r + d][-d] = rec.clone()
        return ins

    def _round(self, name, width=None, counts=None):
        ins = self._route([getattr(p, name.format("pack"))() for p in self.parts])
        for p, i in zip(self.parts, ins):
            getattr(p, name.format("unpack"))(i)

    def _vote(self, answers):
        return all(answers)

    def step(self, steps=1):
        for _ in range(steps):
            if not self._boundary()[1]:
                self._step_exchange()
            self._solve()

    def gather(self):
        """Owned bodies of all partitions merged by global id: dict(ids, transforms, momentum, idle), sorted by id."""
        return _merge([p.owned_state() for p in self.parts])


class RcclDirect:
    """An RCCL communicator of this job's ranks created through ctypes on the RCCL library the process has ALREADY loaded (torch's), for the library-driven per-step
    halo (include/nudge_hip.h: nh_partition_set_transport / nh_partition_exchange_step): the unique id travels over torch.distributed, the four entry points the
    library calls are handed to it as plain addresses.  Everything here may fail (no RCCL library found, a rank that does not answer): `ok` then stays False and the
    caller keeps the torch.distributed transport."""

    def __init__(self, dist, group, device, timeout_s=60.0):
        self.ok, self.why, self.comm, self.lib = False, "", None, None
        try:
            import torch
            path = None
            try:
                for line in open("/proc/self/maps"):
                    if "librccl" in line:
                        path = line.split()[-1]
                        break
            except OSError:
                pass
            self.lib = C.CDLL(path or "librccl.so")
            self.path = path or "librccl.so"

            class UniqueId(C.Structure):
                _fields_ = [("internal", C.c_char * 128)]
            self.lib.ncclGetUniqueId.argtypes = [C.POINTER(UniqueId)]
            self.lib.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, UniqueId, C.c_int]
            rank, world = dist.get_rank(group), dist.get_world_size(group)
            uid = UniqueId()
            if rank == 0:
                rc = self.lib.ncclGetUniqueId(C.byref(uid))
                if rc:
                    raise RuntimeError(f"ncclGetUniqueId: {rc}")
            red = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
            t = torch.frombuffer(bytearray(bytes(uid)), dtype=torch.uint8).clone().to(red)
            dist.broadcast(t, src=0, group=group)
            C.memmove(C.byref(uid), bytes(t.cpu().numpy().tobytes()), 128)
            torch.cuda.set_device(device)
            comm = C.c_void_p()
            rc = self.lib.ncclCommInitRank(C.byref(comm), world, uid, rank)
            if rc:
                raise RuntimeError(f"ncclCommInitRank: {rc}")
            self.comm, self.rank, self.world = comm, rank, world
            self.fn = [C.cast(getattr(self.lib, n), C.c_void_p) for n in ("ncclGroupStart", "ncclGroupEnd", "ncclSend", "ncclRecv")]
            self.ok = True
        except Exception as e:          # noqa: BLE001 -- any failure means "use the torch transport"
            self.why = repr(e)

    def attach(self, partition, loopback=False, timeout_s=60.0):
        """Hands communicator and entry points to the partition's library object and checks both neighbours with a pattern exchange, polled with a time-out so that a
        neighbour that never answers cannot hang the job.  Returns True when the library-driven exchange may be used."""
        p = partition
        if not self.ok or p.hip is None:
            return False
        left = p.rank - 1 if p.rank > 0 else -1
        right = p.rank + 1 if p.rank + 1 < p.ranks else (self.rank if loopback else -1)
        L = p.e.L
        if L.nh_partition_set_transport(p.hip, self.comm, *self.fn, left, right):
            return False
        if left < 0 and right < 0:
            return True
        if L.nh_partition_transport_check(p.hip, 1 << 16, 1):
            L.nh_partition_set_transport(p.hip, None, None, None, None, None, -1, -1)
            return False
        stream = p.torch.cuda.current_stream(p.bt.device)
        t0 = time.time()
        while not stream.query():
            if time.time() - t0 > timeout_s:
                self.why = "transport check timed out"
                L.nh_partition_set_transport(p.hip, None, None, None, None, None, -1, -1)
                return False
            time.sleep(0.001)
        if L.nh_partition_transport_result(p.hip):
            self.why = "transport check: wrong data"
            L.nh_partition_set_transport(p.hip, None, None, None, None, None, -1, -1)
            return False
        return True


class DistCluster(_Cluster):
    """One partition per process; neighbour messages over torch.distributed point-to-point ops
    (backend "nccl" = RCCL over xGMI for GPU tensors, "gloo" for the CPU tests)."""

    def __init__(self, partition, group=None, host_staging=False, loopback=0):
        """`host_staging`: move messages through host memory (for backends without device p2p, e.g. gloo with GPU worlds).
        `loopback` = m > 0: every step this rank also sends the per-step records of its first m owned bodies to ITSELF through the same
        point-to-point ops and writes them back onto those bodies (a no-op for the simulation) -- what a ONE-GPU box can execute of the RCCL path."""
        import torch.distributed as dist
        super().__init__([partition])
        self.dist = dist
        self.p = partition
        self.group = group
        self.torch = partition.torch
        self.host_staging = host_staging
        self.loopback = int(loopback)
        self.loopback_records = 0
        self.loopback_steps = 0
        self._loop_plan = None              # the loopback's buffers and P2P ops, built once
        self._step_plan = None              # per-step exchange of a HIP partition: send / receive buffers and the P2P ops, built once per refresh
        self.direct = False                 # the per-step halo is driven by the library over its own RCCL communicator (use_rccl_direct)
        self.direct_why = ""
        self._rccl = None
        self.multi_step = True              # with the library-driven transport: the sub-steps between two refreshes in ONE call (nh_partition_step); False: one call per sub-step (round 5)
        self._can_multi_step = partition.hip is not None and hasattr(partition.e, "partition_step")
        self._on_the_abi = hasattr(partition.e, "L") and hasattr(partition.e, "ctx")
        # host-side accounting for bench.py (wall time of the refreshes, their own synchronisations included; host time to ENQUEUE a per-step halo)
        self.t_refresh, self.n_refresh, self.t_halo, self.n_halo = 0.0, 0, 0.0, 0

    def _vote(self, answers):
        """Every rank of the job must say yes: one all-reduce of one word."""
        t, dist = self.torch, self.dist
        red = "cuda" if dist.get_backend(self.group) == "nccl" else "cpu"
        flag = t.tensor([1.0 if all(answers) else 0.0], device=red)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.group)
        return bool(flag.item() > 0.5)

    def use_rccl_direct(self, device, loopback=False):
        """Per-step halo through nh_partition_exchange_step (pack, ncclSend / ncclRecv, unpack in ONE library call) instead of torch.distributed point-to-point ops: the
        host's share of a step shrinks to two C calls.  Every rank must end up with the same answer, so the outcome is agreed on with an all-reduce; any doubt -> False."""
        p = self.p
        r = RcclDirect(self.dist, self.group, device)
        ok = r.attach(p, loopback=loopback)
        self.direct = self._vote([ok])
        self.direct_why = r.why
        self._rccl = r                      # (keeps library and communicator alive)
        if not self.direct and ok:
            p.e.L.nh_partition_set_transport(p.hip, None, None, None, None, None, -1, -1)
        return self.direct

    def _fast_step_exchange(self):
        """The per-step halo of a partition on the C ABI, device tensors, lengths fixed since the last refresh: the message buffers and the list of point-to-point ops
        are built once per refresh; a step is pack (one C call), batch_isend_irecv on the prepared ops, unpack (one C call)."""
        t, dist, p = self.torch, self.dist, self.p
        if self._step_plan is None or self._step_plan[0] != p.stats["refreshes"]:
            home = p.bt.device
            ins = {d: t.empty((p.ghost_in[d], STEP_BYTES), dtype=t.uint8, device=home) for d in p.neighbours()}
            ops = []
            for d in p.neighbours():
                if p._stepbuf[d].shape[0]:
                    ops.append(dist.P2POp(dist.isend, p._stepbuf[d], p.rank + d, self.group))
                if p.ghost_in[d]:
                    ops.append(dist.P2POp(dist.irecv, ins[d], p.rank + d, self.group))
            self._step_plan = (p.stats["refreshes"], ins, ops)
        _, ins, ops = self._step_plan
        p.step_pack()
        if ops:
            for w in dist.batch_isend_irecv(ops):
                w.wait()
        p.step_unpack(ins)

    def _loopback(self):
        t, dist, p = self.torch, self.dist, self.p
        m = min(self.loopback, p.n_owned)
        if m <= 0:
            return
        home = p.bt.device
        if self._loop_plan is None or self._loop_plan[0] != m:
            # (buffers and ops built once, like the per-step exchange with real neighbours: _fast_step_exchange)
            idx = t.arange(1, 1 + m, dtype=t.int32, device=home)
            dev = t.device("cpu") if self.host_staging else home
            out = t.empty((m, STEP_BYTES), dtype=t.uint8, device=home)
            back = t.empty((m, STEP_BYTES), dtype=t.uint8, device=dev)
            me = dist.get_rank(self.group)
            stage = out if not self.host_staging else t.empty((m, STEP_BYTES), dtype=t.uint8, device=dev)
            ops = [dist.P2POp(dist.isend, stage, me, self.group), dist.P2POp(dist.irecv, back, me, self.group)]
            self._loop_plan = (m, idx, out, stage, back, ops)
        _, idx, out, stage, back, ops = self._loop_plan
        if self._on_the_abi:                # (nh_halo_pack straight into the prepared buffer)
            E._check(p.e.L, p.e.L.nh_halo_pack(p.e.ctx, C.byref(p.e.bodies), C.c_void_p(idx.data_ptr()), m, C.c_void_p(out.data_ptr())), "halo_pack")
        else:
            out.copy_(p._step_records(idx.to(t.int64), idx))
        if self.host_staging:
            stage.copy_(out)
        for w in dist.batch_isend_irecv(ops):
            w.wait()
        p._step_install(1, back.to(home) if self.host_staging else back)
        self.loopback_records += m
        self.loopback_steps += 1

    def _exchange(self, out, widths=None, known_counts=None):
        """Sends out[d] to rank+d and returns what the neighbours sent.  Counts are exchanged first unless known."""
        t, dist, p = self.torch, self.dist, self.p
        nb = p.neighbours()
        home = p.bt.device
        dev = t.device("cpu") if self.host_staging else home
        if self.host_staging:
            out = {d: r.cpu() for d, r in out.items()}
        if known_counts is None:
            ops, cin = [], {}
            for d in nb:
                cout = t.tensor([out[d].shape[0]], dtype=t.int64, device=dev)
                cin[d] = t.zeros(1, dtype=t.int64, device=dev)
                ops.append(dist.P2POp(dist.isend, cout, p.rank + d, self.group))
                ops.append(dist.P2POp(dist.irecv, cin[d], p.rank + d, self.group))
            if ops:
                for w in dist.batch_isend_irecv(ops):
                    w.wait()
            known_counts = {d: int(cin[d].item()) for d in nb}
        ops, ins = [], {}
        for d in nb:
            ins[d] = t.empty((known_counts[d], widths), dtype=t.uint8, device=dev)
            if out[d].shape[0]:
                ops.append(dist.P2POp(dist.isend, out[d].contiguous(), p.rank + d, self.group))
            if known_counts[d]:
                ops.append(dist.P2POp(dist.irecv, ins[d], p.rank + d, self.group))
        if ops:
            for w in dist.batch_isend_irecv(ops):
                w.wait()
        if self.host_staging:
            ins = {d: r.to(home) for d, r in ins.items()}
        return ins

    def _round(self, name, width, counts=None):
        p = self.p
        out = getattr(p, name.format("pack"))()
        getattr(p, name.format("unpack"))(self._exchange(out, width, known_counts=None if counts is None else counts(p)))

    def _step_exchange(self):
        p = self.p
        if self.direct:
            p.exchange_step()
        elif p.hip is not None and not self.host_staging:
            self._fast_step_exchange()
        else:
            super()._step_exchange()

    def _clock(self, boundary, t_0, n=1):
        """Books the host time since t_0 on the refreshes (an epoch boundary, quiet or not) or on the per-step halo of n sub-steps."""
        if boundary:
            self.t_refresh += time.perf_counter() - t_0; self.n_refresh += 1
        else:
            self.t_halo += time.perf_counter() - t_0; self.n_halo += n

    def step(self, steps=1):
        p = self.p
        # the library drives the sub-steps between two refreshes itself (nh_partition_step): refresh (host), then one call for the steps up to the next one
        library = self.direct and self.multi_step and not p.per_iteration and self._can_multi_step
        left = steps
        while left > 0:
            t_0 = time.perf_counter()
            boundary, refreshed = self._boundary()          # (refreshed False at a boundary: a quiet one)
            if library:
                if boundary:
                    self._clock(True, t_0)
                n = min(left, p.epoch - (p.steps % p.epoch))
                t_0 = time.perf_counter()
                lb = min(self.loopback, p.n_owned) if self.loopback else 0
                p.library_steps(n, exchange_first=not refreshed, loopback_records=lb)          # (no refresh: the first sub-step's exchange is the library's as well)
                self._clock(False, t_0, n)
                if lb:
                    self.loopback_records += lb * (n if not refreshed else n - 1)
                    self.loopback_steps += n
            else:
                n = 1
                if not refreshed:
                    self._step_exchange()
                self._clock(boundary, t_0)
                if self.loopback:
                    self._loopback()
                self._solve()
            left -= n

    def gather(self, dst=0):
        """Owned bodies of all ranks merged by global id on rank `dst` (None elsewhere)."""
        dist = self.dist
        mine = self.p.owned_state()
        world = dist.get_world_size(self.group)
        objs = [None] * world if dist.get_rank(self.group) == dst else None
        dist.gather_object(mine, objs, dst=dst, group=self.group)
        return None if objs is None else _merge(objs)
