"""Scenes for the potential field's statistics split (tests/test_field_stats_split_cpu.py and _gpu.py): each is the
smallest input at which one part of the split -- cost-only statistics and far flags in the sweep kernels, near-cell
statistics over the obstacles' windows in k_field_near, the fold in k_field_batch -- can go wrong.

scene(name) -> (obst [k][16][2], tgt [k][2]) float32, k = 1 or 2 envs that belong to one batch."""
import numpy as np

PARK = 999.0
NAMES = ("ring", "cluster", "edges", "empty", "occupied_target", "detour", "inside_pair")


def _parked(k=1):
    return np.full((k, 16, 2), PARK, np.float32)


def scene(name):
    if name == "ring":
        # (a) a closed ring of radius 2.25 m about (5, 5): the cells at its centre are unreachable (infinite cost)
        # and farther than far_d from every obstacle -- infinite far cells that are not border cells
        a = 2 * np.pi * np.arange(16) / 16
        obst = np.stack([5 + 2.25 * np.cos(a), 5 + 2.25 * np.sin(a)], 1)[None].astype(np.float32)
        return obst, np.array([[-5.0, -5.0]], np.float32)
    if name == "cluster":
        # (b) all sixteen obstacles within 1 m of each other, next to the target: windows overlap fully, and the
        # target itself is a near cell
        gx, gy = np.meshgrid(np.arange(4) * 0.2, np.arange(4) * 0.2)
        obst = np.stack([2.0 + 0.7 + gx.ravel(), -3.0 - 0.3 + gy.ravel()], 1)[None].astype(np.float32)
        return obst, np.array([[2.0, -3.0]], np.float32)
    if name == "edges":
        # (c) windows clipped by the grid edge, in the four corners and on one side
        obst = _parked()
        obst[0, :5] = [[14.9, 14.9], [-14.9, 14.9], [14.9, -14.9], [-14.9, -14.9], [14.9, 0.0]]
        return obst, np.array([[0.0, 0.0]], np.float32)
    if name == "empty":
        # (d) every obstacle parked: no window at all, only the cost-only row
        return _parked(), np.array([[1.3, -2.1]], np.float32)
    if name == "occupied_target":
        # (e) an obstacle on the target cell: the cost field is its seeds' only
        rng = np.random.default_rng(5)
        obst = rng.uniform(-12, 12, (1, 16, 2)).astype(np.float32)
        obst[0, 0] = [0.1, 0.2]
        return obst, np.array([[0.1, 0.2]], np.float32)
    if name == "detour":
        # (f) the long-detour wall of test_env_gpu.py (finite costs above 224: the env takes the reference's 225
        # literal sweeps) in a batch with an ordinary env
        k = np.arange(16) - 7.5
        wall = np.stack([-8.0 - k * 0.9 / np.sqrt(2), -8.0 + k * 0.9 / np.sqrt(2)], 1)
        rng = np.random.default_rng(11)
        obst = np.stack([wall, rng.uniform(-12, 12, (16, 2))]).astype(np.float32)
        return obst, np.array([[-14.3, -14.3], [0.4, -0.3]], np.float32)
    if name == "inside_pair":
        # (g) one env with an obstacle that contains grid cells, one whose only obstacle lies off the grid: it
        # has near cells with J > 0 but none inside (the nearest cell centres are 1.05 m > 2 r_obs away), so the
        # batch's any-inside flag and `high` come from the other env alone
        obst = _parked(2)
        obst[0, 0] = [3.0, 4.0]
        obst[1, 0] = [15.95, 0.1]
        return obst, np.array([[-2.0, 1.0], [-6.0, -6.0]], np.float32)
    raise KeyError(name)


def random_scene(rng):
    """One env: sixteen obstacles uniform over the spawn square, the target near the middle."""
    obst = rng.uniform(-12, 12, (1, 16, 2)).astype(np.float32)
    return obst, rng.uniform(-3, 3, (1, 2)).astype(np.float32)


def batch(name, k, seed):
    """A batch of k envs in shuffled order that holds scene `name` (its first env only when k = 1) and random
    scenes for the rest: (obst [k][16][2], tgt [k][2], env ids [k] drawn from 64 envs)."""
    rng = np.random.default_rng(seed)
    obst, tgt = scene(name)
    obst, tgt = obst[:k], tgt[:k]
    while obst.shape[0] < k:
        o, t = random_scene(rng)
        obst, tgt = np.concatenate([obst, o]), np.concatenate([tgt, t])
    order = rng.permutation(k)
    ids = rng.choice(64, k, replace=False).astype(np.int32)
    return obst[order].copy(), tgt[order].copy(), ids
