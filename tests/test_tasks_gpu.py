"""GoToXY / KeepXY / TrackXYVelocity on the device (k_env_step_task<GO_TO_XY | KEEP_XY | TRACK_XY>, the k_reset
branches) against the reference's recorded episodes X / K / V and against tests/task_restate.py.

* fixture replay in the three legs of test_env_gpu.test_fixture_replay_on_gpu, at its bounds (e2e state bit for
  bit, obs / reward / extras at rtol = atol = 1e-5, dones and goal counters exactly, targets at 1e-6; the
  own-trig leg's reward recorded);
* in-kernel draws at n = 1, 33, 1000 against the restatement on the device's own states;
* the shared path (integrator, DR, spawns, targets, reset masks) bit for bit across kinds;
* penalize_action_variation on GoToPose; two trainers' epochs per new task, graph replay = eager;
* k_env_step (CaptureXY) against k_env_step_task<GO_TO_XY> on the same inputs: the step they share, bit for bit.
"""
import copy
import ctypes
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from omniisaacgymenvs_loop_amd.tasks.usv_config import stat_names
from tests import errtab as ET
from tests import task_restate as R
from tests.test_tasks_cpu import CFG, FIXTURE, _yaml

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STATE_KEYS = ("px", "py", "yaw", "vx", "vy", "wz", "fl", "fr")
NU_RESET = 718


def _task(cfg_d, n, seed=7):
    from omniisaacgymenvs_loop_amd.tasks.usv_virtual import USVVirtual
    return USVVirtual(cfg_d, num_envs=n, device=DEV, seed=seed)


def _cfg_of(d):
    return json.loads(bytes(d["config_json"]).decode())


@pytest.mark.parametrize("variant", sorted(FIXTURE))
def test_fixture_replay_on_gpu(golden, variant):
    d = golden(f"episode_{variant}.npz")
    cfg_d = _cfg_of(d)
    T, n = d["obs"].shape[:2]
    tasks = {}
    for mode in ("e2e", "post", "own"):
        task = _task(cfg_d, n)
        assert task.tgt_h is None and task.task_scratch is None
        task.cfg.inj_trig = 0 if mode == "own" else 1
        task.set_env_origins(torch.zeros(2, n))
        task.tgt[0] = torch.tensor(d["init_tgt"][:, 0], device=DEV)
        task.tgt[1] = torch.tensor(d["init_tgt"][:, 1], device=DEV)
        tasks[mode] = task
    layout = stat_names(tasks["e2e"].cfg)
    names = [k for k, _ in layout]
    assert names == [str(k) for k in d["extras_names"]]
    w = d["obs"].shape[-1]
    cols = ET.obs_cols(w)
    ru = 0
    for t in range(T):
        mask = d["reset_mask"][t]
        ids = np.nonzero(mask)[0]
        U = np.zeros((n, NU_RESET), np.float32)
        U[ids] = d["reset_U"][ru:ru + len(ids)]
        ru += len(ids)
        want_state = np.stack([d[k][t] for k in STATE_KEYS]).T
        for mode, tn in (("post", f"replay_{variant}_post"), ("e2e", f"replay_{variant}"),
                         ("own", f"replay_{variant}_owntrig")):
            task = tasks[mode]
            np.testing.assert_array_equal(task.reset_buf.cpu().numpy().astype(bool), mask)
            assert task.current_action_bias() == pytest.approx(float(d["bias"][t]))
            post = torch.tensor(want_state.T.astype(np.float32), device=DEV) if mode == "post" else None
            obs, rew, dones = task.env_step(torch.tensor(d["actions"][t], device=DEV),
                                            u_step=torch.tensor(d["u_step"][t], device=DEV),
                                            u_reset=torch.tensor(U, device=DEV), post_state=post)
            torch.cuda.synchronize()
            o, r, dn = obs.cpu().numpy(), rew.cpu().numpy(), dones.cpu().numpy()
            ex = task.extras_buf.cpu().numpy()[[slot for _, slot in layout]]
            st = task.state.cpu().numpy()
            if mode == "e2e":
                ET.check(tn, "state", st.T, want_state, 0.0, 0.0, list(STATE_KEYS), f"{tn} state t={t}")
            elif mode == "own":
                ET.check(tn, "state", st.T, want_state, 1e-5, 1e-5, list(STATE_KEYS), f"{tn} state t={t}")
            ET.check(tn, "obs", o[:, :w], d["obs"][t], 1e-5, 1e-5, cols, f"{tn} obs t={t}")
            np.testing.assert_array_equal(dn, d["reset"][t], err_msg=f"{tn} dones t={t}")
            np.testing.assert_array_equal(task.ibuf[0].cpu().numpy(), d["goal_cnt"][t], err_msg=f"{tn} goal_cnt t={t}")
            if mode == "own":
                ET.record(tn, "rew", r, d["rew"][t], tol=("recorded", 0))
                continue
            ET.check(tn, "rew", r, d["rew"][t], 1e-5, 1e-5, err_msg=f"{tn} rew t={t}")
            if len(ids):
                ET.check(tn, "extras", ex, d["extras"][t], 1e-5, 1e-5, names, f"{tn} extras t={t}")
            np.testing.assert_allclose(task.tgt.cpu().numpy().T, d["tgt"][t], rtol=1e-6, atol=1e-6)


def _quiet(cfg_d, ep_len=7):
    """The fixture's config with in-kernel draws that the restatement needs no copy of: no observation or action
    noise; short episodes so every env resets three times in 24 steps."""
    c = copy.deepcopy(cfg_d)
    obs = c["env"]["disturbances"]["observations"]
    for k in ("add_noise_on_pos", "add_noise_on_vel", "add_noise_on_heading"):
        obs[k] = False
    c["env"]["disturbances"]["actions"]["add_noise_on_act"] = False
    c["env"]["maxEpisodeLength"] = ep_len
    return c


def _dev_state(task):
    st = task.state.cpu().numpy()
    return {k: st[i] for i, k in enumerate(STATE_KEYS[:6])}


@pytest.mark.parametrize("n", [1, 33, 1000])
@pytest.mark.parametrize("variant", sorted(FIXTURE))
def test_in_kernel_draws_match_restatement(golden, variant, n):
    """24 steps with maxEpisodeLength 7 (three resets of every env, below a wave / not a multiple of 64 or 256 /
    several workgroups): every step's task columns, reward and dones equal the restatement evaluated on the
    device's own post-step state and targets."""
    cfg_d = _quiet(_cfg_of(golden(f"episode_{variant}.npz")))
    task = _task(cfg_d, n, seed=21)
    cfg = task.cfg
    ep = R.Episode(cfg.task_kind, cfg, n, [k for k, _ in stat_names(cfg)])
    rng = np.random.default_rng(5 + n)
    resets = 0
    tn = f"philox_{FIXTURE[variant]}"
    for t in range(24):
        a = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
        mask = task.reset_buf.cpu().numpy().astype(bool)
        resets += int(mask.sum())
        bias = task.current_action_bias()
        obs, rew, dones = task.env_step(torch.tensor(a, device=DEV))
        torch.cuda.synchronize()
        cols, r, dn, cnt, _ = ep.step(_dev_state(task), task.tgt.cpu().numpy().T, a, mask, bias)
        np.testing.assert_array_equal(dones.cpu().numpy(), dn, err_msg=f"dones t={t}")
        np.testing.assert_array_equal(task.ibuf[0].cpu().numpy(), cnt, err_msg=f"goal_cnt t={t}")
        ET.check(tn, "task_cols", obs.cpu().numpy()[:, R.TASK_COLS], cols, 1e-5, 1e-5, None, f"cols t={t}")
        ET.check(tn, "rew", rew.cpu().numpy(), r, 1e-5, 1e-5, None, f"rew t={t}")
    assert resets >= 4 * n   # the initial reset and three time-outs at the least
    task.check_nan()


def _pair_cfgs(a, b):
    """Two kinds on the same shared path: the same spawn / goal parameters, kills that never fire."""
    ya, yb = _quiet(_yaml(a)), _quiet(_yaml(b))
    if a == "GoToXY":
        common = dict(goal_random_position=2.0, min_spawn_dist=0.3, max_spawn_dist=3.0, kill_dist=1.0e6,
                      position_tolerance=1.0e-9, kill_after_n_steps_in_tolerance=1000000, spawn_curriculum=True,
                      spawn_curriculum_min_dist=0.2, spawn_curriculum_max_dist=1.5, spawn_curriculum_kill_dist=1.0e6,
                      spawn_curriculum_warmup=0, spawn_curriculum_end=1)
        ya["env"]["task_parameters"].update(common)
        yb["env"]["task_parameters"].update(common)
    else:   # the same target-velocity range on the same two draws
        yb["env"]["task_parameters"]["goal_random_linear_velocity"] = ya["env"]["task_parameters"]["goal_random_velocity"]
    return ya, yb


@pytest.mark.parametrize("a,b", [("GoToXY", "GoToPose"), ("TrackXYVelocity", "TrackXYOVelocity")])
def test_shared_path_is_bit_identical_across_kinds(a, b):
    """The integrator, the DR draws, the spawn expressions and slots are shared: with the same seed and actions
    and kills that never fire, state, DR parameters, targets and reset masks agree bit for bit over 24 steps at
    n = 1000 (time-outs every 7 steps: three rounds of spawns, the curriculum moving under GoToXY / GoToPose)."""
    n = 1000
    ta, tb = (_task(y, n, seed=13) for y in _pair_cfgs(a, b))
    rng = np.random.default_rng(3)
    for t in range(24):
        act = torch.tensor(rng.uniform(-1, 1, (n, 2)).astype(np.float32), device=DEV)
        for task in (ta, tb):
            task.env_step(act)
        torch.cuda.synchronize()
        for key in ("state", "params"):
            np.testing.assert_array_equal(getattr(ta, key).cpu().numpy(), getattr(tb, key).cpu().numpy(),
                                          err_msg=f"{key} t={t}")
        # progress and the reset mask (the goal counter is each task's own: TrackXYOVelocity's also asks the yaw rate)
        np.testing.assert_array_equal(ta.ibuf[1:3].cpu().numpy(), tb.ibuf[1:3].cpu().numpy(), err_msg=f"ibuf t={t}")
        np.testing.assert_array_equal(ta.tgt.cpu().numpy(), tb.tgt.cpu().numpy(), err_msg=f"tgt t={t}")
        np.testing.assert_array_equal(ta.dones.cpu().numpy(), tb.dones.cpu().numpy(), err_msg=f"dones t={t}")
    assert int(ta.ibuf[1].max()) < 7 and float(ta.state[0].abs().max()) > 0


def test_action_variation_penalty_on_go_to_pose():
    """penalize_action_variation on an A20 kind (n = 33): the reward moves by exactly the restated penalty of
    sum(actions) - sum(previous actions), resets not clearing the previous sum; the state does not move; with
    penalties_use_thrust_u the reference's aliased tensors make it identically 0."""
    n = 33
    base = _quiet(_yaml("GoToPose"))
    on = copy.deepcopy(base)
    on["env"]["penalties_parameters"]["penalize_action_variation"] = True
    on["env"]["action_processing"]["penalties_use_thrust_u"] = False
    off = copy.deepcopy(on)
    off["env"]["penalties_parameters"]["penalize_action_variation"] = False
    alias = copy.deepcopy(on)
    alias["env"]["action_processing"]["penalties_use_thrust_u"] = True
    alias_off = copy.deepcopy(alias)
    alias_off["env"]["penalties_parameters"]["penalize_action_variation"] = False
    t_on, t_off, t_al, t_al_off = (_task(y, n, seed=4) for y in (on, off, alias, alias_off))
    cfg = t_on.cfg
    slot = dict(stat_names(cfg))["action_variation_penalty"]
    rng = np.random.default_rng(8)
    prev = np.zeros(n, np.float32)
    acc = np.zeros(n, np.float32)
    for t in range(24):
        a = rng.uniform(-1.5, 1.5, (n, 2)).astype(np.float32)
        mask = t_on.reset_buf.cpu().numpy().astype(bool)
        acc[mask] = 0
        at = torch.tensor(a, device=DEV)
        bias = t_on.current_action_bias()
        rews = [task.env_step(at)[1].cpu().numpy() for task in (t_on, t_off, t_al, t_al_off)]
        torch.cuda.synchronize()
        o = R.observe(cfg, _dev_state(t_on))
        cmd, _, unit = R.thrust_units(cfg, a, bias)
        pens, _, prev = R.penalties(cfg, o, cmd, unit, np.zeros(n, np.float32), prev, t > 0)
        want = pens["action_variation_penalty"]
        acc += want
        assert t == 0 or np.abs(want).max() > 0
        ET.check("actv_GoToPose", "rew_delta", rews[0] - rews[1], want, 1e-5, 1e-5, None, f"t={t}")
        ET.check("actv_GoToPose", "sum", t_on.stats[slot].cpu().numpy(), acc, 1e-5, 1e-5, None, f"t={t}")
        np.testing.assert_array_equal(rews[2], rews[3], err_msg=f"aliased t={t}")
        np.testing.assert_array_equal(t_on.state.cpu().numpy(), t_off.state.cpu().numpy())


def _capture_and_xy_cfgs(dist_on):
    """CaptureXY's test config (quiet) and the same config carrying GoToXY's task and reward blocks: every
    constant of the shared path (dynamics, DR, action processing, observation frame, privileged tail) is one."""
    from omniisaacgymenvs_loop_amd.tasks.usv_config import load_yaml
    cap = _quiet(load_yaml(os.path.join(CFG, "IROS2024", "USV_Virtual_CaptureXY_SysID-TEST.yaml")), ep_len=1000)
    if dist_on:
        d = cap["env"]["disturbances"]
        for key in ("use_force_disturbance", "use_constant_force", "use_sinusoidal_force"):
            d["forces"][key] = True
        for key in ("use_torque_disturbance", "use_constant_torque", "use_sinusoidal_torque"):
            d["torques"][key] = True
        cap["env"]["water_current"] = {"use_water_current": True, "flow_velocity": [-0.2, 0.35, 0.0]}
    xy, own = copy.deepcopy(cap), _yaml("GoToXY")
    xy["env"]["task_parameters"] = own["env"]["task_parameters"]
    xy["env"]["reward_parameters"] = own["env"].get("reward_parameters", {}) or {}
    return cap, xy


@pytest.mark.parametrize("n,dist_on", [(33, False), (33, True), (2048, False)], ids=["33", "33-dist", "2048"])
def test_capture_and_task_kernels_share_one_step(n, dist_on):
    """k_env_step (CaptureXY) and k_env_step_task<GO_TO_XY> on the same inputs, through usv_env_step itself: the
    state rows, observation columns 0-2, the previous-command columns (and their array) and the privileged tail
    agree bit for bit over 12 steps.  Every step hands both kernels CaptureXY's state / params / damp / dist /
    env_org, random finite stale rows and the same random just_reset mask (a quarter of the envs: the stale-root
    first substep, the zeroed thrust), actions past the clip and a bias that is 0 on every third step.
    n = 33: the packed slab (StepWin), a partial wave; with the disturbances on, kDist against has_dist;
    n = 2048: the canonical slab (FixedWin<13>), 8 workgroups."""
    from omniisaacgymenvs_loop_amd import _capi
    from omniisaacgymenvs_loop_amd._abi import DEFINES
    cap, xy = (_task(y, n, seed=17) for y in _capture_and_xy_cfgs(dist_on))
    assert cap.cfg.task_kind == 0 and xy.cfg.task_kind == DEFINES["USV_TASK_GO_TO_XY"]
    assert cap.cfg.stale_root == 1 and (cap.dist is not None) == dist_on and (xy.dist is not None) == dist_on
    assert bool(cap.cfg.fsin_on and cap.cfg.tsin_on and cap.cfg.current_on) == dist_on
    rng = np.random.default_rng(40 + n)
    first = torch.tensor(rng.uniform(-1, 1, (n, 2)).astype(np.float32), device=DEV)
    bufs = []
    for task in (cap, xy):
        task.env_step(first)
        b = task._make_bufs()
        b.clock = None   # the step index and the bias are the arguments' (not the device clock's)
        bufs.append(b)
    pa, priv = DEFINES["USV_NOBS_BASE"] - 2, int(cap.cfg.priv_dim)
    shared = ("state", "params", "damp", "dist", "env_org", "stale")
    for t in range(12):
        cap.stale.copy_(torch.tensor(rng.normal(0, 1, tuple(cap.stale.shape)).astype(np.float32)))
        mask = torch.tensor((rng.random(n) < 0.25).astype(np.uint8), device=DEV)
        assert 0 < int(mask.sum()) < n
        for key in shared:
            if getattr(cap, key) is not None:
                getattr(xy, key).copy_(getattr(cap, key))
        act = torch.tensor(rng.uniform(-1.2, 1.2, (n, 2)).astype(np.float32), device=DEV)
        bias = 0.0 if t % 3 == 0 else 0.05 * t
        for task, b in zip((cap, xy), bufs):
            task.just_reset.copy_(mask)
            _capi.call("usv_env_step", _capi.byref(task.cfg), _capi.byref(b), _capi.ptr(act), _capi.ptr(task.lut),
                       ctypes.c_float(bias), 17, 100 + t, None, _capi.stream_ptr())
        torch.cuda.synchronize()
        oc, ox = cap.obs_buf_t.cpu().numpy(), xy.obs_buf_t.cpu().numpy()
        for what, a, b in (("state", cap.state, xy.state), ("prev_cmd", cap.prev_cmd, xy.prev_cmd),
                           ("obs 0-2", oc[:, :3], ox[:, :3]), ("obs prev_cmd", oc[:, pa:pa + 2], ox[:, pa:pa + 2]),
                           ("priv tail", oc[:, pa + 2:pa + 2 + priv], ox[:, pa + 2:pa + 2 + priv])):
            a, b = (v.cpu().numpy() if torch.is_tensor(v) else v for v in (a, b))
            assert np.isfinite(a).all(), f"{what} t={t}"
            np.testing.assert_array_equal(a, b, err_msg=f"{what} t={t}")
        assert np.abs(oc[:, pa:pa + 2][mask.cpu().numpy() != 0]).max() == 0   # a reset env's previous command
    assert float(cap.state[6:8].abs().max()) > 0 and float(cap.state[0:6].abs().max()) > 0
    assert not dist_on or float(cap.dist.abs().max()) > 0   # drawn disturbance parameters


def _agent_env(task_name, n, minibatch, use_graph, seed=11):
    from omniisaacgymenvs_loop_amd.envs.vec_env_rlgames import VecEnvRLGames
    from omniisaacgymenvs_loop_amd.rl_games.a2c_continuous import A2CAgent
    from omniisaacgymenvs_loop_amd.scripts import rlgames_train as T
    from omniisaacgymenvs_loop_amd.utils.task_util import initialize_task
    cfg = T.build_config({"num_envs": n, "minibatch_size": minibatch, "seed": seed,
                          "task": f"USV/USV_Virtual_{task_name}"})
    env = VecEnvRLGames(headless=True)
    task = initialize_task(cfg, env)
    params = cfg["train"]["params"]
    params["config"].update(vec_env=env, train_dir="/tmp/task_test_runs", hip_graph=use_graph, print_stats=False)
    return env, task, A2CAgent("run", params)


@pytest.mark.parametrize("name", sorted(FIXTURE.values()))
def test_ppo_epochs_graph_replay_matches_eager(name):
    """A2CAgent on each new task at 256 envs: finite losses, the NaN flag clear, and the graph run (eager,
    capture, then two replayed epochs) equal to the eager run bit for bit."""
    from omniisaacgymenvs_loop_amd.tasks.usv_config import TASK_KINDS
    runs = []
    for use_graph in (False, True):
        env, task, ag = _agent_env(name, 256, 1024, use_graph)
        assert task.cfg.task_kind == TASK_KINDS[name]
        ag.obs = ag.env_reset()
        for _ in range(4):
            ag.train_epoch()
        torch.cuda.synchronize()
        env.check_errors()
        assert torch.isfinite(ag.losses).all() and torch.isfinite(ag.model_params).all()
        runs.append({"params": ag.model_params.cpu().numpy(), "m": ag.adam_m.cpu().numpy(),
                     "state": task.state.cpu().numpy(), "obs": task.obs_buf_t.cpu().numpy(),
                     "rew": ag.exp_rew.cpu().numpy(), "clock": task.clock.cpu().numpy()})
        if use_graph:
            assert ag._graph_play is not None and ag._graph_update is not None
    for k in runs[0]:
        np.testing.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)
