"""Policy banks on the GPU (ppo_policy_bank_step, usv_bank_* of libusv_hip.so, rl_games.ModelBank,
eval.BankTraceEvaluator / rollout_bank, scripts/multi_model_eval.py).

The main oracle is bit equality: a group of a bank run is the stand-alone run of that model.  The motion and
summary kernels are held against the reference-derived fixture tests/golden/bank_eval_golden.npz (ALV / AAV / AAC
within 32 x 2^-24 x mean|v| of the reference's float32 numbers, the bound its generator asserts) and against the
numpy restatement tests/bank_restate.py (count x 2^-52 x max|v| on the double sums, integers exactly)."""
import copy
import csv
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import bank_restate as B
from tests import task_eval_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "omniisaacgymenvs_loop_amd", "cfg", "task", "USV")
YAML_OF = {"pose": "GoToPose", "track": "TrackXYOVelocity"}
NIN, NPARAM = 33, 21253


def _yaml(name):
    from omniisaacgymenvs_loop_amd.tasks.usv_config import load_yaml
    return load_yaml(os.path.join(CFG, f"USV_Virtual_{name}.yaml"))


def _task(cfg_d, n, seed=7):
    from omniisaacgymenvs_loop_amd.tasks.usv_virtual import USVVirtual
    return USVVirtual(cfg_d, num_envs=n, device=DEV, seed=seed)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _same_bits(a, b, msg=""):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), msg


# ---- 1, 2: the forward ------------------------------------------------------------------------------------------
def _models(M):
    """M weight sets whose mu head is scaled so that some mu leave +-1, and a different obs_rms per model."""
    from omniisaacgymenvs_loop_amd._abi import DEFINES as D
    from omniisaacgymenvs_loop_amd.rl_games.a2c_continuous import default_linear_init
    g = torch.Generator().manual_seed(5)
    params = torch.stack([default_linear_init(11 + m) for m in range(M)])
    params[:, D["PPO_OFF_WMU"]:] *= 12.0
    params[:, D["PPO_OFF_BMU"]:] = torch.rand((M, 2), generator=g) - 0.5
    rms = torch.zeros((M, 2 * NIN + 1), dtype=torch.float64)
    rms[:, :NIN] = torch.randn((M, NIN), generator=g, dtype=torch.float64) * 0.5
    rms[:, NIN:2 * NIN] = torch.rand((M, NIN), generator=g, dtype=torch.float64) * 3.0 + 0.25
    rms[:, 2 * NIN] = 100.0
    return params.to(DEV), rms.to(DEV)


def _obs(n, nan_row=None):
    g = torch.Generator().manual_seed(9)
    obs = (torch.randn((n, NIN), generator=g) * 3.0).clamp(-12.0, 12.0)
    obs[1], obs[n - 2, ::2], obs[n - 2, 1::2] = 12.0, -12.0, 12.0
    if nan_row is not None:
        obs[nan_row, 7] = float("nan")
    return obs.to(DEV)


def _bank_step(params, rms, obs, M, G, grid_cap=0):
    from omniisaacgymenvs_loop_amd import _capi as c
    from omniisaacgymenvs_loop_amd._abi import PpoCfg
    cfg = PpoCfg()
    cfg.horizon, cfg.n_envs, cfg.minibatch, cfg.normalize_input, cfg.rms_eps = 1, M * G, 64, 1, 1e-5
    out = torch.full((M * G, 2), 7.0, device=DEV)
    c.call("ppo_policy_bank_step", c.byref(cfg), c.ptr(params), c.ptr(rms), c.ptr(obs), M, G, c.ptr(out), grid_cap,
           c.stream_ptr())
    return out


def _single_mu(params, rms, obs):
    """ppo_policy_step with one model on its rows (as PpoPlayerContinuous.get_action calls it): the mu it stores."""
    from omniisaacgymenvs_loop_amd import _capi as c
    from omniisaacgymenvs_loop_amd._abi import PpoCfg
    n = obs.shape[0]
    cfg = PpoCfg()
    cfg.horizon, cfg.n_envs, cfg.minibatch, cfg.normalize_input, cfg.rms_eps = 1, n, 64, 1, 1e-5
    f = lambda *s: torch.zeros(s, device=DEV)
    sc = {"obs": f(n, NIN), "act": f(n, 2), "nlp": f(n), "val": f(n), "mu": f(n, 2), "sigma": f(n, 2)}
    done8, dones = torch.zeros(n, device=DEV, dtype=torch.uint8), torch.zeros(n, device=DEV, dtype=torch.int64)
    actions = f(n, 2)
    val_rms = torch.tensor([0.0, 1.0, 1.0], device=DEV, dtype=torch.float64)
    c.call("ppo_policy_step", c.byref(cfg), c.ptr(params), c.ptr(rms), c.ptr(val_rms), c.ptr(obs.contiguous()), 0,
           c.ptr(sc["obs"]), c.ptr(sc["act"]), c.ptr(sc["nlp"]), c.ptr(sc["val"]), c.ptr(sc["mu"]), c.ptr(sc["sigma"]),
           c.ptr(done8), c.ptr(dones), c.ptr(actions), 42, 0, None, None, c.stream_ptr())
    return sc["mu"]


@pytest.mark.parametrize("M,G", [(3, 32), (2, 96), (1, 64)])
def test_forward_equals_the_single_model_step_bit_for_bit(M, G):
    """Every group is clamp(mu) of ppo_policy_step with that model alone on its G rows; rows at +-12, some mu past
    +-1, normalisation on with the model's own statistics; a NaN observation stays in its row."""
    params, rms = _models(M)
    nan_row = G + 3 if M > 1 else 3
    obs = _obs(M * G, nan_row)
    got = _bank_step(params, rms, obs, M, G)
    torch.cuda.synchronize()
    want = torch.cat([_single_mu(params[m].contiguous(), rms[m].contiguous(), obs[m * G:(m + 1) * G])
                      for m in range(M)])
    assert torch.isnan(want[nan_row]).all() and torch.isnan(got[nan_row]).all()
    keep = torch.ones(M * G, dtype=torch.bool, device=DEV)
    keep[nan_row] = False
    assert torch.isfinite(got[keep]).all() and torch.isfinite(want[keep]).all()
    assert (want[keep].abs() > 1).any() and (want[keep].abs() < 1).any()   # the clamp acts, and not everywhere
    _same_bits(got[keep], want[keep].clamp(-1.0, 1.0))
    if M > 1:   # the models matter: group 0's weights on group 1's rows give other actions
        other = _single_mu(params[0].contiguous(), rms[0].contiguous(), obs[G:2 * G]).clamp(-1.0, 1.0)
        assert not torch.equal(other[:3], got[G:G + 3])


def test_model_boundaries_inside_a_workgroup():
    """M = 5, G = 32: one workgroup walks all five models (grid_cap 1), two split them 2 + 3, the default grid has
    one tile each: identical bits."""
    params, rms = _models(5)
    obs = _obs(160)
    outs = [_bank_step(params, rms, obs, 5, 32, grid_cap=g) for g in (1, 2, 0)]
    _same_bits(outs[0], outs[2], "grid_cap 1")
    _same_bits(outs[1], outs[2], "grid_cap 2")
    want = torch.cat([_single_mu(params[m].contiguous(), rms[m].contiguous(), obs[m * 32:(m + 1) * 32])
                      for m in range(5)]).clamp(-1.0, 1.0)
    _same_bits(outs[0], want)


# ---- 3: the uniforms --------------------------------------------------------------------------------------------
def _noisy(cfg_d):
    cfg_d = copy.deepcopy(cfg_d)
    cfg_d["env"]["disturbances"]["observations"]["add_noise_on_pos"] = True
    cfg_d["env"]["disturbances"]["actions"]["add_noise_on_act"] = True
    return cfg_d


def _uniforms(task, group):
    from omniisaacgymenvs_loop_amd import _capi as c
    from omniisaacgymenvs_loop_amd._abi import DEFINES as D
    n = task.num_envs
    us = torch.full((n, D["USV_NU_STEP"]), -1.0, device=DEV)
    ur = torch.full((n, D["USV_NU_RESET"]), -1.0, device=DEV)
    c.call("usv_bank_uniforms", c.byref(task.cfg), c.byref(task._bufs), group, task.seed, task._step_index,
           c.ptr(us), c.ptr(ur), c.stream_ptr())
    return us, ur


def test_uniforms_repeat_per_group_and_equal_the_in_kernel_draws():
    """Rows e and e + G are equal; only the resetting envs' reset rows are written; a G-env task stepped 12 times
    (the spawn included, position and action noise on, episodes of 5 steps so that envs reset again) on the
    injected words equals the same task on its in-kernel Philox draws bit for bit."""
    G, T = 64, 12
    cfg_d = _noisy(_yaml("GoToPose"))
    cfg_d["env"]["maxEpisodeLength"] = 5
    big = _task(copy.deepcopy(cfg_d), 2 * G, seed=13)
    big.reset()
    big.ibuf[2][5] = 0
    big.ibuf[2][G + 9] = 0
    us, ur = _uniforms(big, G)
    _same_bits(us[:G], us[G:])
    assert (us >= 0).all() and (us < 1).all() and us[:, 4:].std() > 0.1   # the second Philox block is drawn
    assert (ur[5] == -1).all() and (ur[G + 9] == -1).all()                # rows of envs not in reset: left alone
    rows = torch.ones(2 * G, dtype=torch.bool)
    rows[[5, 9, G + 5, G + 9]] = False
    rows = rows.to(DEV)
    _same_bits(ur[:G][rows[:G]], ur[G:][rows[G:]])
    assert (ur[rows] >= 0).all() and (ur[rows] < 1).all()
    quiet = _task(_yaml("GoToPose"), G, seed=13)   # no position / action noise: words 4..7 are the kernel's zeros
    assert (_uniforms(quiet, G)[0][:, 4:] == 0).all()

    inj, own = _task(copy.deepcopy(cfg_d), G, seed=13), _task(copy.deepcopy(cfg_d), G, seed=13)
    g = torch.Generator().manual_seed(3)
    acts = (torch.rand((T, G, 2), generator=g) * 2 - 1).to(DEV)
    resets = 0
    for t in range(T):
        us, ur = _uniforms(inj, G)
        a = inj.env_step(acts[t], u_step=us, u_reset=ur)
        b = own.env_step(acts[t])
        for x, y, what in zip(a + (inj.state,), b + (own.state,), ("obs", "rew", "dones", "state")):
            _same_bits(x, y, f"{what} differs at step {t}")
        resets += int(a[2].sum())
    assert resets > G   # every env reset again after its spawn


# ---- 4, 5, 7: bank runs -----------------------------------------------------------------------------------------
def _obs_dim(yaml_name):
    from omniisaacgymenvs_loop_amd._abi import DEFINES as D
    from omniisaacgymenvs_loop_amd.tasks.usv_config import build_usv_cfg
    return D["USV_NOBS_BASE"] + int(build_usv_cfg(_yaml(yaml_name)).priv_dim)


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    """Three checkpoints per observation width, written once."""
    root = tmp_path_factory.mktemp("bank_ckpts")
    made = {}

    def get(obs_dim):
        if obs_dim not in made:
            nn = [root / f"w{obs_dim}" / f"exp{m}" / "nn" for m in range(3)]
            made[obs_dim] = [B.write_checkpoint(nn[m] / f"last_exp{m}_ep_{10 + m}_rew_0.pth", 21 + m, obs_dim=obs_dim,
                                                epoch=10 + m, mu_gain=10.0) for m in range(3)]
        return made[obs_dim]
    return get


def _bank_run(cfg_d, paths, G, H, paired, seed=17):
    from omniisaacgymenvs_loop_amd.eval import BankTraceEvaluator, rollout_bank
    from omniisaacgymenvs_loop_amd.rl_games.model_bank import ModelBank
    M = len(paths)
    task = _task(copy.deepcopy(cfg_d), M * G, seed=seed)
    bank = ModelBank(paths, task.num_observations, DEV)
    ev = BankTraceEvaluator(task, H, M, G, paired=paired)
    assert rollout_bank(task, bank, ev) == H
    torch.cuda.synchronize()
    return task, ev


def _group_equals_alone(yaml_name, cfg_d, ckpts, skip_return=False, want_resets=False):
    G, H = 64, 24
    paths = ckpts(_obs_dim(yaml_name))
    task, ev = _bank_run(cfg_d, paths, G, H, paired=True)
    tab, mo, summ = ev.table.cpu().numpy(), ev.motion.cpu().numpy(), ev.summary_raw().cpu().numpy().copy()
    assert (tab[R.STEPS] == H).all() and (mo[B.STEPS] == H).all() and (summ[:, B.S_PAIRS] == H * G).all()
    ret_rows = [R.RETURN]
    ret_slots = [R.S_RETURN + 1, R.S_RETURN + 2]
    for m in range(3):
        alone_task, alone = _bank_run(cfg_d, paths[m:m + 1], G, H, paired=False)
        sl = slice(m * G, (m + 1) * G)
        a_tab, a_mo = alone.table.cpu().numpy(), alone.motion.cpu().numpy()
        a_sum = alone.summary_raw().cpu().numpy()[0]
        rows = [r for r in range(R.ROWS) if not (skip_return and r in ret_rows)]
        slots = [s for s in range(B.S_N) if not (skip_return and s in ret_slots)]
        np.testing.assert_array_equal(tab[rows][:, sl].view(np.int64), a_tab[rows].view(np.int64), err_msg=f"table {m}")
        np.testing.assert_array_equal(mo[:, sl].view(np.int64), a_mo.view(np.int64), err_msg=f"motion {m}")
        np.testing.assert_array_equal(summ[m][slots].view(np.int64), a_sum[slots].view(np.int64),
                                      err_msg=f"summary {m}")
        _same_bits(task.state[:, sl], alone_task.state, f"state {m}")
        if want_resets:
            assert a_sum[R.S_RESETS] > 0
    assert len({summ[m, B.S_ACT_SUM] for m in range(3)}) == 3   # three models, three behaviours
    return summ


@pytest.mark.parametrize("yaml_name", ["GoToPose", "TrackXYVelocity"])
@pytest.mark.parametrize("resetting", [False, True])
def test_group_equals_the_stand_alone_run(ckpts, yaml_name, resetting):
    """M = 3, G = 64, horizon 24: each group's table columns, motion rows, summary row and final state equal a
    stand-alone run of that model on 64 envs with the same seed (a one-model bank, unpaired: in-kernel draws and
    the 64-env origins) bit for bit.  resetting: episodes of 9 steps with the kill rules on, so envs reset inside
    the horizon and the reset rows are injected mid-run."""
    cfg_d = _yaml(yaml_name)
    if resetting:
        cfg_d["env"]["maxEpisodeLength"] = 9
    else:
        cfg_d["env"]["maxEpisodeLength"], cfg_d["env"]["fixed_horizon_eval"] = 26, True
    summ = _group_equals_alone(yaml_name, cfg_d, ckpts, want_resets=resetting)
    assert (summ[:, R.S_RESETS] > 0).all() == resetting


def test_track_xyo_group_equals_the_stand_alone_run_but_for_the_return(ckpts):
    """TrackXYOVelocity's reward holds a sum over all envs of the run (3 x 64 here, 64 alone): everything but the
    RETURN row and the return's mean / std equals the stand-alone run."""
    cfg_d = _yaml("TrackXYOVelocity")
    cfg_d["env"]["maxEpisodeLength"], cfg_d["env"]["fixed_horizon_eval"] = 26, True
    _group_equals_alone("TrackXYOVelocity", cfg_d, ckpts, skip_return=True)


def test_pairing(ckpts):
    """The same checkpoint in all three groups: paired, three identical summary rows; unpaired (each env on the
    draws of its own index and its own origin), the rows differ."""
    cfg_d = _yaml("GoToPose")
    cfg_d["env"]["maxEpisodeLength"], cfg_d["env"]["fixed_horizon_eval"] = 26, True
    path = ckpts(_obs_dim("GoToPose"))[0]
    _, ev = _bank_run(cfg_d, [path] * 3, 64, 24, paired=True)
    s = ev.summary_raw().cpu().numpy()
    np.testing.assert_array_equal(s[0].view(np.int64), s[1].view(np.int64))
    np.testing.assert_array_equal(s[0].view(np.int64), s[2].view(np.int64))
    rows = ev.summaries()
    assert rows[0] == rows[1] == rows[2] and np.isfinite([rows[0][k] for k in ("ALV", "AAV", "AAC")]).all()
    assert (ev.records()["model"] == np.repeat(np.arange(3), 64)).all()
    _, ev = _bank_run(cfg_d, [path] * 3, 64, 24, paired=False)
    u = ev.summary_raw().cpu().numpy()
    assert u[0, B.S_SPEED_SUM] != u[1, B.S_SPEED_SUM] != u[2, B.S_SPEED_SUM] and u[0, B.S_ACT_SUM] != u[1, B.S_ACT_SUM]


@pytest.mark.parametrize("paired", [False, True])
def test_evaluator_has_no_side_effect(ckpts, paired):
    """The env's state, observation, reward and dones after a run with the evaluator hooked in equal a run of the
    same bank without it (on the same draws)."""
    from omniisaacgymenvs_loop_amd.eval import BankTraceEvaluator
    from omniisaacgymenvs_loop_amd.rl_games.model_bank import ModelBank
    cfg_d = _yaml("GoToPose")
    cfg_d["env"]["maxEpisodeLength"] = 9
    G, H = 32, 20
    paths = ckpts(_obs_dim("GoToPose"))
    hooked, ev = _bank_run(cfg_d, paths, G, H, paired=paired)
    plain = _task(copy.deepcopy(cfg_d), 3 * G, seed=17)
    bank = ModelBank(paths, plain.num_observations, DEV)
    draws = BankTraceEvaluator(plain, H, 3, G, paired=paired).draws   # the words only: never hooked into a step
    plain.reset()
    obs, _, _ = plain.env_step(torch.zeros((3 * G, 2), device=DEV), **draws())
    plain.reset()
    for _ in range(H):
        obs, rew, dones = plain.env_step(bank.get_action(obs), **draws())
    torch.cuda.synchronize()
    for x, y, what in ((hooked.state, plain.state, "state"), (hooked.obs_buf_t, plain.obs_buf_t, "obs"),
                       (hooked.rew_buf, plain.rew_buf, "rew"), (hooked.dones, plain.dones, "dones")):
        _same_bits(x, y, what)
    assert ev.table.cpu().numpy()[R.RESETS].sum() > 0


# ---- 6: the motion and summary kernels on written buffers ---------------------------------------------------
def _kernel_level(data, name, models, group, horizon=None, steps=None):
    """usv_teval_step + usv_bank_step driven from a trace written into the task's buffers (no env step)."""
    from omniisaacgymenvs_loop_amd.eval import BankTraceEvaluator
    kind, obs, rew, reset, thr, levels, act = data
    T, n = obs.shape[:2]
    task = _task(_yaml(YAML_OF[name]), n)
    ev = BankTraceEvaluator(task, T if horizon is None else horizon, models, group, paired=False,
                            thresholds=[float(v) for v in thr], levels=[[float(v) for v in row] for row in levels])
    for t in range(T if steps is None else steps):
        task.obs_buf_t.copy_(torch.tensor(np.ascontiguousarray(obs[t]), device=DEV))
        task.rew_buf.copy_(torch.tensor(np.ascontiguousarray(rew[t]), device=DEV))
        task.ibuf[2] = torch.tensor(np.ascontiguousarray(reset[t]), device=DEV, dtype=torch.int32)
        ev.step(torch.tensor(np.ascontiguousarray(act[t]), device=DEV))
    torch.cuda.synchronize()
    return ev


def _tiled(data, envs):
    kind, obs, rew, reset, thr, levels, act = data
    return kind, obs[:, envs], rew[:, envs], reset[:, envs], thr, levels, act[:, envs]


def _check_kernels(ev, data, name, models, group, horizon):
    """Motion rows and summary against the restatement; the first USV_TEVS_N entries of every row are the bits of
    usv_teval_summary on a table holding that group alone; two summary calls agree bitwise."""
    from omniisaacgymenvs_loop_amd.eval import TaskTraceEvaluator
    kind, obs, rew, reset, thr, levels, act = data
    mo, tab = ev.motion.cpu().numpy(), ev.table.cpu().numpy()
    want_mo = B.motion(obs, act, horizon)
    np.testing.assert_array_equal(mo[B.STEPS], want_mo[B.STEPS])
    vmax = [np.nanmax(B.speed(obs)), np.nanmax(np.abs(obs[..., 2])), 2.0]
    for r in range(3):
        np.testing.assert_array_equal(np.isnan(mo[r]), np.isnan(want_mo[r]))
        ok = ~np.isnan(want_mo[r])
        assert (np.abs(mo[r] - want_mo[r])[ok] <= horizon * 2.0 ** -52 * vmax[r]).all(), f"motion row {r}"
    a = ev.summary_raw().cpu().numpy().copy()
    b = ev.summary_raw().cpu().numpy().copy()
    np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))
    want = B.summarize(tab, mo, models, group, 2, horizon)
    counts = [R.S_ENVS, R.S_CHANNELS, R.S_STEPS_MIN, R.S_STEPS_MAX, R.S_RESETS, R.S_RESET_ENVS, R.S_RETURN, B.S_PAIRS]
    for c in range(2):
        counts += [R.S_CH + R.S_CH_STRIDE * c + q for q in range(6)]
    np.testing.assert_array_equal(a[:, counts], want[:, counts])
    for q, r in ((B.S_SPEED_SUM, 0), (B.S_YAWRATE_SUM, 1), (B.S_ACT_SUM, 2)):
        np.testing.assert_array_equal(np.isnan(a[:, q]), np.isnan(want[:, q]))
        ok = ~np.isnan(want[:, q])
        assert (np.abs(a[:, q] - want[:, q])[ok] <= horizon * group * 2.0 ** -52 * vmax[r]).all(), f"summary slot {q}"
    rest = [i for i in range(R.S_N) if i not in counts]
    np.testing.assert_allclose(a[:, rest], want[:, rest], rtol=1e-12, atol=0, equal_nan=True)
    alone = TaskTraceEvaluator(_task(_yaml(YAML_OF[name]), group), horizon, thresholds=[float(v) for v in thr],
                               levels=[[float(v) for v in row] for row in levels])
    for m in range(models):
        alone.table.copy_(ev.table[:, m * group:(m + 1) * group])
        np.testing.assert_array_equal(a[m, :R.S_N].view(np.int64), alone.summary_raw().cpu().numpy().view(np.int64),
                                      err_msg=f"group {m} vs usv_teval_summary alone")
    return a


@pytest.mark.parametrize("name", ["pose", "track"])
def test_motion_and_summary_kernels_reproduce_the_reference(name):
    """n = 70 in two groups of 35 (a group boundary inside a wave): the per-group success tables are the
    reference's exactly, ALV / AAV / AAC within 32 x 2^-24 x mean|v| of its float32 numbers; group 1's NaN step
    gives NaN as it does there; the env with all-zero actions sums to 0."""
    from omniisaacgymenvs_loop_amd.eval.bank_evaluator import motion_figures
    bg, tg = B.load_golden(), R.load_golden()
    data = B.synthetic(bg, tg, name)
    kind, obs, rew, reset, thr, levels, act = data
    ev = _kernel_level(data, name, 2, B.GROUP)
    a = _check_kernels(ev, data, name, 2, B.GROUP, B.T)
    assert ev.motion[B.ACT_SUM, 3] == 0 and int(torch.isnan(ev.motion[B.SPEED_SUM]).sum()) == 1
    rows = ev.summaries()
    for g in range(2):
        sl = slice(g * B.GROUP, (g + 1) * B.GROUP)
        for c, ch in enumerate(ev.channels):
            want = bg[f"{name}_rates"][g, c]
            assert list(rows[g][ch]["table"].values()) == [want[0], want[1], want[2] * 100]
            np.testing.assert_allclose(np.array(list(rows[g][ch]["time_under"].values())),
                                       bg[f"{name}_time_under"][g, c] * 100, rtol=1e-12)
        got = np.array([motion_figures(a[g])[k] for k in ("ALV", "AAV", "AAC")])
        assert [rows[g][k] for k in ("ALV", "AAV", "AAC")] == list(got) or g == 1
        ref = bg[f"{name}_figures_f32"][g]
        mean_abs = np.array([np.nanmean(B.speed(obs[:, sl]).astype(np.float64)),
                             np.nanmean(np.abs(obs[:, sl, 2]).astype(np.float64)),
                             np.mean(np.abs(act[:, sl].astype(np.float64)))])
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
        ok = ~np.isnan(ref)
        assert (np.abs(got - ref)[ok] <= 32 * 2.0 ** -24 * mean_abs[ok]).all(), (got, ref)
        assert np.isnan(got[:2]).all() == (g == 1)


def test_summary_with_more_than_one_env_per_thread():
    """Groups of 2,080 (threads 0..31 of a group's workgroup fold a third env, the others two)."""
    bg, tg = B.load_golden(), R.load_golden()
    data = _tiled(B.synthetic(bg, tg, "track"), np.arange(2 * 2080) % 70)
    a = _check_kernels(_kernel_level(data, "track", 2, 2080), data, "track", 2, 2080, B.T)
    assert (a[:, R.S_ENVS] == 2080).all() and (a[:, B.S_PAIRS] == 2080 * B.T).all()


def test_a_step_past_the_horizon_changes_steps_only():
    bg, tg = B.load_golden(), R.load_golden()
    data = B.synthetic(bg, tg, "pose")
    a = _kernel_level(data, "pose", 2, B.GROUP, horizon=20, steps=20)
    b = _kernel_level(data, "pose", 2, B.GROUP, horizon=20)
    ma, mb = a.motion.cpu().numpy(), b.motion.cpu().numpy()
    assert (ma[B.STEPS] == 20).all() and (mb[B.STEPS] == 24).all()
    np.testing.assert_array_equal(ma[:3].view(np.int64), mb[:3].view(np.int64))
    sa, sb = a.summary_raw().cpu().numpy(), b.summary_raw().cpu().numpy()
    keep = [i for i in range(B.S_N) if i not in (R.S_STEPS_MIN, R.S_STEPS_MAX)]
    np.testing.assert_array_equal(sa[:, keep].view(np.int64), sb[:, keep].view(np.int64))
    assert (sb[:, B.S_PAIRS] == 20 * B.GROUP).all() and (sb[:, R.S_STEPS_MAX] == 24).all()


# ---- 8: the script ----------------------------------------------------------------------------------------------
def test_script_end_to_end(ckpts, tmp_path):
    """Three checkpoints in a tree of experiments, 32 envs each, horizon 16: three CSV rows with `model` first, the
    JSON, the per-env CSV; two passes (bank.models_per_pass=2) give the same rows; CaptureXY is refused."""
    from omniisaacgymenvs_loop_amd.eval.bank_report import bank_csv_columns
    from omniisaacgymenvs_loop_amd.scripts import multi_model_eval
    paths = ckpts(_obs_dim("GoToPose"))
    load_dir = os.path.dirname(os.path.dirname(os.path.dirname(paths[0])))
    out_csv, out_json, env_csv = (str(tmp_path / f) for f in ("bank.csv", "bank.json", "bank_envs.csv"))
    common = ["task=USV/USV_Virtual_GoToPose", "num_envs=32", "eval.horizon=16", f"bank.load_dir={load_dir}"]
    names, summaries, report = multi_model_eval.main(common + [
        f"eval.output_csv={out_csv}", f"eval.summary_json={out_json}", f"eval.per_env_csv={env_csv}"])
    assert names == ["exp0", "exp1", "exp2"]
    rows = list(csv.reader(open(out_csv)))
    s0 = summaries[0]
    assert tuple(rows[0]) == bank_csv_columns(s0["channels"], [s0[c]["threshold"] for c in s0["channels"]],
                                              [s0[c]["levels"] for c in s0["channels"]])
    assert rows[0][0] == "model" and [r[0] for r in rows[1:]] == names and len(rows) == 4
    assert len({r[rows[0].index("AAC")] for r in rows[1:]}) == 3
    assert all(r[rows[0].index("resets")] == "0" for r in rows[1:])
    j = json.load(open(out_json))
    assert list(j["models"]) == names and j["envs_per_model"] == 32 and j["horizon"] == 16 and j["paired"] is True
    assert j["models"]["exp1"]["checkpoint"] == paths[1] and j["models"]["exp1"]["envs"] == 32
    assert j["models"]["exp2"]["steps_min"] == j["models"]["exp2"]["steps_max"] == 16
    per_env = list(csv.reader(open(env_csv)))
    assert per_env[0][:2] == ["model", "env"] and len(per_env) == 1 + 96 and per_env[33][:2] == ["exp1", "0"]
    _, two_pass, _ = multi_model_eval.main(common + ["bank.models_per_pass=2"])
    assert two_pass == summaries
    _, listed, _ = multi_model_eval.main(["task=USV/USV_Virtual_GoToPose", "num_envs=32", "eval.horizon=16",
                                          f"bank.checkpoints=[{paths[2]},{paths[0]}]"])
    assert listed == [summaries[2], summaries[0]]
    with pytest.raises(SystemExit, match="evaluate_policy.py eval.episodes_per_env"):
        multi_model_eval.main([f"bank.load_dir={load_dir}", "num_envs=32"])
    with pytest.raises(SystemExit, match="multiple of 32"):
        multi_model_eval.main(common[:1] + ["num_envs=40", f"bank.load_dir={load_dir}"])
