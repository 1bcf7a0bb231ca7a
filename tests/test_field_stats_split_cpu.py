"""The cover argument behind the potential field's statistics split, restated in NumPy over the oracle's cost field.

The field's per-env statistics (csrc/usv_field.hip SS_*) are minima, maxima and ORs of per-cell values, so any cover
of the grid gives the same value.  The kernels split the grid in two:
  * the sweep kernels fold the cost statistics over every cell, and two flags over the cells outside every
    obstacle window: "some finite-cost cell" and "some infinite-cost cell" lies out there (such a cell has J = +0
    and is not inside, so only its existence matters);
  * k_field_near applies the full per-cell statistic to the cells of each obstacle's window (a cell of two
    windows twice).
Here both rows and their fold are formed as the kernels form them and compared with one pass over all cells."""
import numpy as np
import pytest

from oracle import oracle as O
from omniisaacgymenvs_loop_amd.tasks.usv_config import build_usv_cfg, load_yaml
from tests import field_split_scenes as S
from tests.test_oracle_golden import TEST_YAML

G = 150
F32 = np.float32
INF = F32(np.inf)
# (statistic, is a minimum): the ten statistics a slot's row holds
STATS = (("gmin_f", True), ("gmax_f", False), ("any_inf", False), ("jmin_f_ni", True), ("jmax_f_ni", False),
         ("jmax_f_all", False), ("jrmin_i_ni", True), ("jrmax_i_ni", False), ("jrmax_i_all", False), ("inside", False))


@pytest.fixture(scope="module")
def cfg():
    return build_usv_cfg(load_yaml(TEST_YAML))


def _far_d(cfg, cell):
    return F32(F32(F32(cfg.influence_radius) + F32(2.0) * F32(cfg.obstacle_radius)) + F32(0.01) * cell) + F32(1e-3)


def _cells(cfg, cost, obst, lin):
    """Per-cell values of one env: squared distance to the nearest obstacle, inside, raw J, masked J, infinite."""
    cell = F32(np.float64(cfg.map_size) / G)
    dx = lin[None, :, None] - obst[None, None, :, 0]
    dy = lin[:, None, None] - obst[None, None, :, 1]
    d2 = (dy * dy + dx * dx).astype(F32).min(-1)
    dte = (np.sqrt(d2) - F32(cfg.obstacle_radius)) - F32(cfg.obstacle_radius)
    ins = dte <= 0
    inv_r = F32(1.0 / np.float64(cfg.influence_radius))
    t = F32(1.0) / np.maximum(dte, F32(1e-3)) - inv_r
    jr = np.where(dte < F32(cfg.influence_radius), F32(cfg.eta) * (t * t), F32(0)).astype(F32)
    gi = np.isinf(cost)
    with np.errstate(invalid="ignore"):
        j = (jr * np.clip(np.where(gi, F32(0), cost) * cell / F32(cfg.safe_radius), F32(0), F32(1))).astype(F32)
    return d2, ins, jr, j, gi


def _neutral():
    return {k: (INF if is_min else (-INF if k in ("gmax_f", "jmax_f_ni", "jrmax_i_ni") else F32(0))) for k, is_min in STATS}


def _stat(acc, cost, ins, jr, j, gi, sel):
    """k_field_near's stat() over the selected cells (every statistic takes the cell's value or its neutral)."""
    def lo(key, vals, where):
        v = vals[sel & where]
        if v.size:
            acc[key] = min(acc[key], v.min())

    def hi(key, vals, where):
        v = vals[sel & where]
        if v.size:
            acc[key] = max(acc[key], v.max())
    lo("gmin_f", cost, ~gi); hi("gmax_f", cost, ~gi)
    hi("any_inf", gi.astype(F32), np.ones_like(gi))
    lo("jmin_f_ni", j, ~gi & ~ins); hi("jmax_f_ni", j, ~gi & ~ins); hi("jmax_f_all", j, ~gi)
    lo("jrmin_i_ni", jr, gi & ~ins); hi("jrmax_i_ni", jr, gi & ~ins); hi("jrmax_i_all", jr, gi)
    hi("inside", ins.astype(F32), np.ones_like(ins))


def _windows(cfg, obst):
    """near_window of every obstacle: (cl, ch, rl, rh) index ranges, none for a parked obstacle."""
    cell = F32(np.float64(cfg.map_size) / G)
    half = F32(np.float64(cfg.map_size) / 2)
    wc = (_far_d(cfg, cell) + cell) / cell
    out = []
    for ox, oy in obst:
        ic, jc = (F32(ox) + half) / cell - F32(0.5), (F32(oy) + half) / cell - F32(0.5)
        if not (abs(ic) < 4 * G and abs(jc) < 4 * G):
            continue
        cl, ch = max(int(np.ceil(ic - wc)), 0), min(int(np.floor(ic + wc)), G - 1)
        rl, rh = max(int(np.ceil(jc - wc)), 0), min(int(np.floor(jc + wc)), G - 1)
        if cl <= ch and rl <= rh:
            out.append((cl, ch, rl, rh))
    return out


def _check_env(cfg, cost, obst, lin):
    cell = F32(np.float64(cfg.map_size) / G)
    cost = cost.reshape(G, G)
    d2, ins, jr, j, gi = _cells(cfg, cost, obst, lin)
    every = np.ones((G, G), bool)
    # one pass over all cells
    direct = _neutral()
    _stat(direct, cost, ins, jr, j, gi, every)
    # the windows and the near map (their union)
    wins = _windows(cfg, obst)
    near = np.zeros((G, G), bool)
    for cl, ch, rl, rh in wins:
        near[rl:rh + 1, cl:ch + 1] = True
    # premise: a cell outside every window meets the far criterion, has raw J = +0 and is not inside
    far_d = _far_d(cfg, cell)
    assert (d2[~near] >= far_d * far_d).all()
    assert not ins[~near].any() and (jr[~near] == 0).all() and not np.signbit(jr[~near]).any()
    # premise: the window is the issue's -- it holds every cell with |x - ox| <= far_d + cell, |y - oy| <= far_d + cell
    for ox, oy in obst:
        box = (np.abs(lin[None, :] - ox) <= far_d + cell) & (np.abs(lin[:, None] - oy) <= far_d + cell)
        assert not (box & ~near).any()
    # the sweep kernels' row: cost statistics over every cell, the far flags as min(., +0) / max(., +0)
    row_c = _neutral()
    fin = cost[~gi]
    if fin.size:
        row_c["gmin_f"], row_c["gmax_f"] = fin.min(), fin.max()
    row_c["any_inf"] = F32(gi.any())
    if (~near & ~gi).any():
        row_c["jmin_f_ni"], row_c["jmax_f_ni"] = F32(0), F32(0)
    if (~near & gi).any():
        row_c["jrmin_i_ni"], row_c["jrmax_i_ni"] = F32(0), F32(0)
    # k_field_near's row: stat() over each window's cells
    row_n = _neutral()
    for cl, ch, rl, rh in wins:
        sel = np.zeros((G, G), bool)
        sel[rl:rh + 1, cl:ch + 1] = True
        _stat(row_n, cost, ins, jr, j, gi, sel)
    row_n["gmin_f"], row_n["gmax_f"], row_n["any_inf"] = INF, -INF, F32(0)
    # k_field_batch's fold of the two rows
    for key, is_min in STATS:
        folded = min(row_c[key], row_n[key]) if is_min else max(row_c[key], row_n[key])
        np.testing.assert_array_equal(np.asarray(folded, F32), np.asarray(direct[key], F32), err_msg=key)
    return near, d2, gi, far_d


@pytest.mark.parametrize("name", S.NAMES)
def test_split_statistics_equal_full_grid_pass(cfg, name):
    obst, tgt = S.scene(name)
    _, cost = O.potential_field(cfg, obst, tgt, want_cost=True)
    lin = O.grid_lin(cfg.map_size)
    for k in range(obst.shape[0]):
        near, d2, gi, far_d = _check_env(cfg, cost[k], obst[k], lin)
        far = d2 >= far_d * far_d
        border = np.ones((G, G), bool)
        border[1:-1, 1:-1] = False
        if name == "ring":
            # 620 infinite far cells: the 596 border cells and 24 cells enclosed by the ring
            assert int((far & gi).sum()) == 620 and int((far & gi & ~border).sum()) == 24
        if name == "empty":
            assert not near.any()
        if name == "detour" and k == 0:
            assert cost[k][np.isfinite(cost[k])].max() > 224.0


def test_split_statistics_random_scenes(cfg):
    rng = np.random.default_rng(17)
    scenes = [S.random_scene(rng) for _ in range(20)]
    obst = np.concatenate([s[0] for s in scenes])
    tgt = np.concatenate([s[1] for s in scenes])
    _, cost = O.potential_field(cfg, obst, tgt, want_cost=True)
    lin = O.grid_lin(cfg.map_size)
    for k in range(20):
        _check_env(cfg, cost[k], obst[k], lin)
