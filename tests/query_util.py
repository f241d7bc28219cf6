"""What the scene-query tests share: the small scenes, the bounds of a world's colliders, random unit quaternions."""
import numpy as np

from nudge_amd import scenes as S

SMALL = {
    "pile": lambda: S.pile(256, 64, seed=1),
    "compound": lambda: S.compound(150, seed=6),
    "stacks": lambda: S.stacks(64, 3, seed=5),
    "grid_tiles": lambda: S.grid_tiles(4, side=16, sphere_fraction=0.5, seed=2),
    "ball_pit": lambda: S.ball_pit(6, 6, 6, seed=4),
}


def bounds(rec):
    """(lowest, highest) centre of the colliders with a finite pose (float64)."""
    p = rec["p"][np.isfinite(rec["p"]).all(axis=1)].astype(np.float64)
    return p.min(axis=0), p.max(axis=0)


def unit_quats(rng, n):
    """n unit quaternions (float32): one rng.normal(size=(n, 4)) draw, normalised in float64."""
    q = rng.normal(size=(n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
