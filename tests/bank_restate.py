"""Numpy restatement of the policy-bank evaluation (usv_bank_* of include/usv_hip.h): the motion sums behind the
reference's ALV / AAV / AAC (scripts/multi_model_eval.py:107-113, on the USV's columns) as streaming double sums,
and the per-group summary as tests/task_eval_restate.summarize on each group's columns.  tests/test_bank_cpu.py
holds it against the reference's own numbers (tests/golden/bank_eval_golden.npz, written by
tests/golden/make_bank_eval_golden.py); the GPU tests hold the kernels against it."""
from __future__ import annotations

import os

import numpy as np

from tests import task_eval_restate as R

F = np.float32
SPEED_SUM, YAWRATE_SUM, ACT_SUM, STEPS, ROWS = 0, 1, 2, 3, 4     # USV_BEV_*
S_SPEED_SUM, S_YAWRATE_SUM, S_ACT_SUM, S_PAIRS, S_N = 23, 24, 25, 26, 27   # USV_BEVS_*
T, N, GROUP = 24, 70, 35   # the fixture's synthetic sets: two groups of 35


def speed(obs):
    """float32 norm(obs[0], obs[1]): float32 products, a float32 sum, the correctly rounded root."""
    obs = np.asarray(obs, F)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = obs[..., 0], obs[..., 1]
        return np.sqrt(a * a + b * b).astype(F)


def motion(obs, act, horizon, steps=None):
    """usv_bank_step over obs [T][n][>= 3], act [T][n][2]: the [USV_BEV_ROWS][n] table, every term added in
    double in step order; a step past horizon counts in STEPS only."""
    obs, act = np.asarray(obs, F), np.asarray(act, F)
    tab = np.zeros((ROWS, obs.shape[1]), np.float64)
    for t in range(obs.shape[0] if steps is None else steps):
        tab[STEPS] += 1
        if t >= horizon:
            continue
        tab[SPEED_SUM] = tab[SPEED_SUM] + speed(obs[t]).astype(np.float64)
        tab[YAWRATE_SUM] = tab[YAWRATE_SUM] + np.abs(obs[t, :, 2]).astype(np.float64)
        tab[ACT_SUM] = tab[ACT_SUM] + (act[t, :, 0].astype(np.float64) + act[t, :, 1].astype(np.float64))
    return tab


def summarize(tab, mo, models, group, nch, horizon):
    """usv_bank_summary's [models][USV_BEVS_N] with numpy."""
    out = np.zeros((models, S_N), np.float64)
    for m in range(models):
        sl = slice(m * group, (m + 1) * group)
        out[m, :R.S_N] = R.summarize(tab[:, sl], nch)
        out[m, S_SPEED_SUM:S_SPEED_SUM + 3] = mo[:3, sl].sum(1)
        out[m, S_PAIRS] = np.minimum(mo[STEPS, sl], horizon).sum()
    return out


def figures(row):
    """(ALV, AAV, AAC) of a summary row."""
    p = row[S_PAIRS]
    return row[S_SPEED_SUM] / p, row[S_YAWRATE_SUM] / p, row[S_ACT_SUM] / (2.0 * p)


def write_checkpoint(path, seed, obs_dim=33, epoch=1, hidden=None, mu_gain=1.0):
    """A checkpoint (<path>, ending in .pth) of the default-initialised network of `seed` written with
    save_checkpoint; its observation mean is 0.01 seed and its variance 1 + 0.1 seed, so no two seeds normalise
    alike.  mu_gain scales the mu head (so that some actions leave +-1); hidden: another hidden width, for the
    refusal tests."""
    import torch

    from omniisaacgymenvs_loop_amd._abi import DEFINES as D
    from omniisaacgymenvs_loop_amd.rl_games import checkpoint as ckpt
    from omniisaacgymenvs_loop_amd.rl_games.a2c_continuous import default_linear_init
    nin = ckpt.NIN
    obs_rms = torch.zeros(2 * nin + 1, dtype=torch.float64)
    obs_rms[:nin], obs_rms[nin:2 * nin], obs_rms[2 * nin] = 0.01 * seed, 1.0 + 0.1 * seed, 1.0
    params = default_linear_init(seed, obs_dim).cpu()
    params[D["PPO_OFF_WMU"]:] *= mu_gain
    sd = ckpt.model_state_dict(params, obs_rms, torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64), obs_dim)
    if hidden is not None:
        sd["a2c_network.actor_mlp.2.weight"] = torch.zeros(hidden, hidden)
    path = str(path)
    assert path.endswith(".pth")
    ckpt.save_checkpoint(path[:-len(".pth")], {"model": sd, "epoch": epoch})
    return path


def load_golden():
    return dict(np.load(os.path.join(R.GOLDEN, "bank_eval_golden.npz"), allow_pickle=False))


def synthetic(bg, tg, name):
    """Synthetic set `name` of the task-eval fixture tg with the bank fixture's motion columns and actions:
    (kind, obs [T][n][33], rew, reset, thr, levels, act [T][n][2])."""
    kind, obs, rew, reset, thr, levels = R.synthetic(tg, name)
    obs = obs.copy()
    obs[..., 0:3] = bg[f"{name}_vel"]
    return kind, obs, rew, reset, thr, levels, bg[f"{name}_act"]
