"""Fixed-horizon success-rate evaluation on the GPU (usv_teval_* of libusv_hip.so, eval.TaskTraceEvaluator, the
env_step hook, PpoPlayerContinuous.evaluate_horizon, scripts/evaluate_policy.py) against the reference-derived
fixture tests/golden/task_eval_golden.npz and the numpy restatement tests/test_task_eval_cpu.py validates against it.

Integers and flags exactly; the double sums at rtol = 1e-12; the heading channel's error (the device's own atan2
against numpy's) at the project's rtol = atol = 1e-5."""
import copy
import csv
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import errtab as ET
from tests import task_eval_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "omniisaacgymenvs_loop_amd", "cfg", "task", "USV")
BLOCK = 256   # k_teval_step's workgroup
YAML_OF = {"pose": "GoToPose", "track": "TrackXYOVelocity"}


@pytest.fixture(scope="module")
def tg():
    return R.load_golden()


def _yaml(name):
    from omniisaacgymenvs_loop_amd.tasks.usv_config import load_yaml
    return load_yaml(os.path.join(CFG, f"USV_Virtual_{name}.yaml"))


def _task(cfg_d, n, seed=7):
    from omniisaacgymenvs_loop_amd.tasks.usv_virtual import USVVirtual
    return USVVirtual(cfg_d, num_envs=n, device=DEV, seed=seed)


def _tiled(tg, name, envs):
    """Synthetic set `name` with its env columns picked by index list `envs`."""
    kind, obs, rew, reset, thr, levels = R.synthetic(tg, name)
    return kind, obs[:, envs], rew[:, envs], reset[:, envs], thr, levels


def _kernel_level(data, name, horizon=None, extra=None):
    """Drive usv_teval_step from a trace written into a task's observation, reward and reset buffers with torch
    (no env step).  extra: further (obs, rew, reset) steps past the trace.  Returns the evaluator."""
    from omniisaacgymenvs_loop_amd.eval import TaskTraceEvaluator
    kind, obs, rew, reset, thr, levels = data
    T, n = obs.shape[:2]
    task = _task(_yaml(YAML_OF[name]), n)
    assert int(task.cfg.task_kind) == kind
    ev = TaskTraceEvaluator(task, T if horizon is None else horizon, thresholds=[float(v) for v in thr],
                            levels=[[float(v) for v in row] for row in levels])
    assert ev.thresholds == tuple(float(v) for v in thr)
    steps = [(obs[t], rew[t], reset[t]) for t in range(T)] + list(extra or [])
    for o, r, rs in steps:
        task.obs_buf_t.copy_(torch.tensor(np.ascontiguousarray(o), device=DEV))
        task.rew_buf.copy_(torch.tensor(np.ascontiguousarray(r), device=DEV))
        task.ibuf[2] = torch.tensor(np.ascontiguousarray(rs), device=DEV, dtype=torch.int32)
        ev.step(None)
    torch.cuda.synchronize()
    return ev


def _assert_table(got, want, heading_channel=None, msg=""):
    """Integer rows, STEPS and RESETS exactly; ERR_SUM / RETURN at rtol 1e-12; ERR_LAST exactly (it is the float32
    error itself) -- except the heading channel's error rows, at rtol = atol = 1e-5."""
    assert got.shape == want.shape
    for row in (R.STEPS, R.RESETS):
        np.testing.assert_array_equal(got[row], want[row], err_msg=f"{msg} row {row}")
    np.testing.assert_allclose(got[R.RETURN], want[R.RETURN], rtol=1e-12, atol=0, err_msg=f"{msg} return")
    for c in range(2):
        g, w = got[R.CH_STRIDE * c:R.CH_STRIDE * (c + 1)], want[R.CH_STRIDE * c:R.CH_STRIDE * (c + 1)]
        for row in R.INT_ROWS:
            np.testing.assert_array_equal(g[row], w[row], err_msg=f"{msg} channel {c} row {row}")
        if c == heading_channel:
            for row, qty in ((R.ERR_LAST, "err_last"), (R.ERR_SUM, "err_sum")):
                ok = ~np.isnan(w[row])
                np.testing.assert_array_equal(np.isnan(g[row]), ~ok, err_msg=f"{msg} heading {qty} NaN")
                ET.check(f"teval_{msg.split()[0]}", f"head_{qty}", g[row][ok], w[row][ok], 1e-5, 1e-5, None,
                         f"{msg} heading {qty}")
        else:
            np.testing.assert_array_equal(g[R.ERR_LAST], w[R.ERR_LAST], err_msg=f"{msg} channel {c} err_last")
            np.testing.assert_allclose(g[R.ERR_SUM], w[R.ERR_SUM], rtol=1e-12, atol=0, equal_nan=True,
                                       err_msg=f"{msg} channel {c} err_sum")


@pytest.fixture(scope="module")
def synthetic_runs(tg):
    """The two synthetic sets at n = 70 through the kernels, shared by the kernel-level and summary tests."""
    return {name: _kernel_level(_tiled(tg, name, np.arange(70)), name) for name in ("pose", "track")}


@pytest.mark.parametrize("name", ["pose", "track"])
def test_kernels_reproduce_reference_on_synthetic_set(tg, synthetic_runs, name):
    """n = 70 (one full wave plus six lanes), 24 steps: the fixture's integers and flags, and every row of the
    restatement."""
    ev = synthetic_runs[name]
    tab = ev.table.cpu().numpy()
    for c in range(2):
        R.assert_channel(R.channel_records(tab, c), R.golden_channel(tg, f"A_{name}", c), msg=f"{name} channel {c}")
    want = R.restate(*R.synthetic(tg, name), horizon=24)
    _assert_table(tab, want, heading_channel=1 if name == "pose" else None, msg=name)
    assert (tab[R.STEPS] == 24).all() and tab[R.RESETS].sum() > 0
    rec = ev.records()
    np.testing.assert_array_equal(rec["position_first_thr" if name == "pose" else "xy_velocity_first_thr"],
                                  tg[f"A_{name}_first_thr"][0])


@pytest.mark.parametrize("name", ["pose", "track"])
@pytest.mark.parametrize("n", [1, BLOCK + 1])
def test_kernels_at_one_env_and_past_one_block(tg, name, n):
    names = [str(s) for s in tg[f"A_{name}_case_names"]]
    envs = np.array([names.index("reached_then_out")]) if n == 1 else np.arange(n) % 70
    data = _tiled(tg, name, envs)
    ev = _kernel_level(data, name)
    tab = ev.table.cpu().numpy()
    _assert_table(tab, R.restate(*data, horizon=24), heading_channel=1 if name == "pose" else None, msg=f"{name} n={n}")
    for c in range(2):
        want = {k: (v[..., envs]) for k, v in R.golden_channel(tg, f"A_{name}", c).items()}
        R.assert_channel(R.channel_records(tab, c), want, msg=f"{name} n={n} channel {c}")


@pytest.mark.parametrize("name", ["pose", "track"])
def test_a_step_past_the_horizon_changes_nothing_but_steps(tg, name):
    data = _tiled(tg, name, np.arange(70))
    kind, obs, rew, reset, thr, levels = data
    short = (kind, obs[:20], rew[:20], reset[:20], thr, levels)
    a = _kernel_level(short, name).table.cpu().numpy()
    # four more steps past horizon = 20, with values that would change every row
    extra = [(np.zeros_like(obs[0]), np.ones_like(rew[0]), np.ones_like(reset[0]))] * 4
    b = _kernel_level(short, name, horizon=20, extra=extra).table.cpu().numpy()
    assert (a[R.STEPS] == 20).all() and (b[R.STEPS] == 24).all()
    b[R.STEPS] = a[R.STEPS]
    np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))


def _check_summary(ev, nch):
    from omniisaacgymenvs_loop_amd.eval.report import task_summary_from_device
    a = ev.summary_raw().cpu().numpy().copy()
    b = ev.summary_raw().cpu().numpy().copy()
    np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))   # two calls: the same bits
    tab = ev.table.cpu().numpy()
    want = R.summarize(tab, nch)
    counts = [R.S_ENVS, R.S_CHANNELS, R.S_STEPS_MIN, R.S_STEPS_MAX, R.S_RESETS, R.S_RESET_ENVS, R.S_RETURN]
    for c in range(2):
        counts += [R.S_CH + R.S_CH_STRIDE * c + q for q in range(6)]
    np.testing.assert_array_equal(a[counts], want[counts])
    rest = [i for i in range(R.S_N) if i not in counts]
    np.testing.assert_allclose(a[rest], want[rest], rtol=1e-12, atol=0, equal_nan=True)
    s = ev.summary()
    again = task_summary_from_device(a, ev.channels, ev.thresholds_given, ev.thresholds, ev.levels, ev.horizon)
    assert s["envs"] == tab.shape[1] and all(s[k]["table"] == again[k]["table"] for k in ev.channels)
    return s, tab


@pytest.mark.parametrize("name", ["pose", "track"])
def test_summary_matches_numpy_and_is_deterministic(tg, synthetic_runs, name):
    s, tab = _check_summary(synthetic_runs[name], 2)
    first = s["channels"][0]
    rec = R.channel_records(tab, 0)
    assert list(s[first]["table"].values()) == [R.rates(rec)[0], R.rates(rec)[1], R.rates(rec)[2] * 100]
    assert 0 < s[first]["table"][list(s[first]["table"])[0]] < 100 and s["envs_reset"] > 0


@pytest.mark.parametrize("n", [1, 1100])
def test_summary_at_one_env_and_with_two_envs_per_thread(tg, n):
    """n = 1100: threads 0..75 of the one workgroup fold a second env."""
    data = _tiled(tg, "track", np.arange(n) % 70 if n > 1 else np.array([2]))
    s, tab = _check_summary(_kernel_level(data, "track"), 2)
    assert s["steps_min"] == s["steps_max"] == 24 and s["envs"] == n


def test_summary_of_a_one_channel_kind(tg):
    """GoToXY-like use: TrackXYVelocity reads only the norm channel; the second channel's slots stay 0."""
    from omniisaacgymenvs_loop_amd.eval import TaskTraceEvaluator
    kind, obs, rew, reset, thr, levels = _tiled(tg, "track", np.arange(70))
    task = _task(_yaml("TrackXYVelocity"), 70)
    ev = TaskTraceEvaluator(task, 24, thresholds=[float(thr[0])], levels=[[float(v) for v in levels[0]]])
    for t in range(24):
        task.obs_buf_t.copy_(torch.tensor(obs[t], device=DEV))
        task.rew_buf.copy_(torch.tensor(rew[t], device=DEV))
        task.ibuf[2] = torch.tensor(reset[t], device=DEV, dtype=torch.int32)
        ev.step(None)
    tab = ev.table.cpu().numpy()
    want = R.restate(R.TRACK_XY, obs, rew, reset, thr[:1], levels[:1], horizon=24)
    _assert_table(tab, want, msg="track_xy")
    R.assert_channel(R.channel_records(tab, 0), R.golden_channel(tg, "A_track", 0), msg="track_xy")
    s, _ = _check_summary(ev, 1)
    assert s["channels"] == ["xy_velocity"] and "omega_velocity" not in s
    assert (ev.summary_raw().cpu().numpy()[R.S_CH + R.S_CH_STRIDE:R.S_RETURN] == 0).all()


@pytest.mark.parametrize("variant", sorted(R.FIXTURE_KIND))
def test_fixture_replay_with_evaluator(tg, golden, variant):
    """The reference's recorded episodes X / K / V / P / T through USVVirtual.env_step(evaluator=...) with the
    recorded draws injected (as test_fixture_replay_on_gpu): the integer and flag rows equal the reference's
    results on its recorded observations (fixture (b): every compared value at least 1e-4 (1 + level) from every
    level, the device's observations within 1e-5 + 1e-5 |x|); every row equals the restatement fed the device's
    own observations, rewards and dones."""
    from omniisaacgymenvs_loop_amd._abi import DEFINES
    from omniisaacgymenvs_loop_amd.eval import TaskTraceEvaluator
    d = golden(f"episode_{variant}.npz")
    cfg_d = json.loads(bytes(d["config_json"]).decode())
    kind = R.FIXTURE_KIND[variant]
    T, n = d["obs"].shape[:2]
    task = _task(cfg_d, n)
    assert int(task.cfg.task_kind) == kind
    task.cfg.inj_trig = 1
    task.set_grid_lin(torch.tensor(d["grid_lin"]))
    task.set_env_origins(torch.zeros(2, n))
    task.tgt[0] = torch.tensor(d["init_tgt"][:, 0], device=DEV)
    task.tgt[1] = torch.tensor(d["init_tgt"][:, 1], device=DEV)
    thr, levels = tg[f"B_{variant}_thr"], tg[f"B_{variant}_levels"]
    ev = TaskTraceEvaluator(task, T, thresholds=[float(v) for v in thr],
                            levels=[[float(v) for v in row] for row in levels])
    nu = DEFINES["USV_NU_RESET"]
    dev = {"obs": [], "rew": [], "done": []}
    ru = 0
    for t in range(T):
        ids = np.nonzero(d["reset_mask"][t])[0]
        U = np.zeros((n, nu), np.float32)
        U[ids] = d["reset_U"][ru:ru + len(ids)]
        ru += len(ids)
        obs, rew, dones = task.env_step(torch.tensor(d["actions"][t], device=DEV),
                                        u_step=torch.tensor(d["u_step"][t], device=DEV),
                                        u_reset=torch.tensor(U, device=DEV), evaluator=ev)
        dev["obs"].append(task.obs_buf_t.clone())
        dev["rew"].append(rew.clone())
        dev["done"].append(dones.clone())
    torch.cuda.synchronize()
    dev = {k: torch.stack(v).cpu().numpy() for k, v in dev.items()}
    np.testing.assert_array_equal(dev["done"], d["reset"])
    np.testing.assert_allclose(dev["obs"][:, :, :d["obs"].shape[-1]], d["obs"], rtol=1e-5, atol=1e-5)
    tab = ev.table.cpu().numpy()
    nch = len(R.CHANNELS[kind])
    for c in range(nch):
        R.assert_channel(R.channel_records(tab, c), R.golden_channel(tg, f"B_{variant}", c),
                         msg=f"replay_{variant} channel {c} vs fixture")
    own = R.restate(kind, dev["obs"], dev["rew"], dev["done"], thr, levels, horizon=T)
    _assert_table(tab, own, heading_channel=1 if kind == R.GO_TO_POSE else None, msg=f"replay_{variant}")
    np.testing.assert_array_equal(tab[R.RESETS], d["reset"].sum(0))
    s = ev.summary()
    for c, name in enumerate(R.CHANNELS[kind]):
        got = list(s[name]["table"].values())
        want = tg[f"B_{variant}_rates"][c]
        assert got == [want[0], want[1], want[2] * 100], name
        np.testing.assert_allclose(np.array(list(s[name]["time_under"].values())),
                                   tg[f"B_{variant}_time_under"][c] * 100, rtol=1e-12)


@pytest.mark.parametrize("name", ["GoToPose", "TrackXYOVelocity"])
def test_evaluator_has_no_side_effect(name):
    """n = 70, 40 steps, in-kernel Philox draws: obs, rew, dones and the state are bit-identical with and without
    an evaluator at every step; the overlapped step refuses one."""
    from omniisaacgymenvs_loop_amd.eval import TaskTraceEvaluator
    cfg_d = _yaml(name)
    cfg_d["env"]["maxEpisodeLength"] = 15
    n, T = 70, 40
    plain, hooked = _task(copy.deepcopy(cfg_d), n, seed=11), _task(copy.deepcopy(cfg_d), n, seed=11)
    ev = TaskTraceEvaluator(hooked, T)
    g = torch.Generator(device="cpu").manual_seed(3)
    acts = (torch.rand((T, n, 2), generator=g) * 2 - 1).to(DEV)
    outs = {"plain": [], "hooked": []}
    for t in range(T):
        for key, task, kw in (("plain", plain, {}), ("hooked", hooked, {"evaluator": ev})):
            obs, rew, dones = task.env_step(acts[t], **kw)
            outs[key].append((obs.clone(), rew.clone(), dones.clone(), task.state.clone()))
    torch.cuda.synchronize()
    for t in range(T):
        for a, b, what in zip(outs["plain"][t], outs["hooked"][t], ("obs", "rew", "dones", "state")):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b), f"{what} differs at step {t}"
    tab = ev.table.cpu().numpy()
    assert (tab[R.STEPS] == T).all()
    assert int(tab[R.RESETS].sum()) == int(sum(o[2].sum() for o in outs["hooked"])) > 0
    with pytest.raises(ValueError, match="evaluator"):
        hooked.env_step(acts[0], overlap=True, evaluator=ev)


def test_capture_xy_is_refused():
    from omniisaacgymenvs_loop_amd.eval import TaskTraceEvaluator
    from omniisaacgymenvs_loop_amd.tasks.usv_config import load_yaml
    task = _task(load_yaml(os.path.join(CFG, "IROS2024", "USV_Virtual_CaptureXY_SysID-TEST.yaml")), 8)
    with pytest.raises(ValueError, match="EpisodeEvaluator"):
        TaskTraceEvaluator(task, 10)


def _player(n, horizon):
    import yaml

    from omniisaacgymenvs_loop_amd.envs.vec_env_rlgames import VecEnvRLGames
    from omniisaacgymenvs_loop_amd.rl_games.players import PpoPlayerContinuous
    cfg_d = _yaml("GoToPose")
    cfg_d["env"]["maxEpisodeLength"] = horizon + 2
    cfg_d["env"]["fixed_horizon_eval"] = True
    env = VecEnvRLGames(headless=True)
    env.set_task(_task(cfg_d, n))
    with open(os.path.join(ROOT, "omniisaacgymenvs_loop_amd/cfg/train/USV/USV_PPOcontinuous_MLP.yaml")) as f:
        params = yaml.safe_load(f)["params"]
    params["config"].update(num_actors=n, device=DEV, vec_env=env)
    return PpoPlayerContinuous(params)


def test_player_evaluate_horizon_and_script_csv(tmp_path):
    """PpoPlayerContinuous.evaluate_horizon(24) on 256 GoToPose envs with the default-initialised network: no env
    resets inside the horizon, 24 steps each; the summary equals the restatement on the observations a wrapping
    policy callable collected.  The script writes a 256-row CSV and the summary JSON for TrackXYVelocity."""
    from omniisaacgymenvs_loop_amd.eval import default_levels, default_thresholds, task_csv_columns
    H, n = 24, 256
    player = _player(n, H)
    task = player.env._task
    seen = []
    inner = player.get_action

    def spy(obs, det=True):
        seen.append(obs.clone())
        return inner(obs, det)

    player.get_action = spy
    records, summary = player.evaluate_horizon(horizon=H)
    assert len(seen) == H
    obs = torch.stack(seen[1:] + [task.obs_view.clone()]).cpu().numpy()   # trace index t: the observation after step t
    assert (records["resets"] == 0).all() and (records["steps"] == H).all()
    assert summary["resets"] == 0 and summary["steps_min"] == summary["steps_max"] == H and summary["envs"] == n
    thr = default_thresholds(task.cfg)
    assert player.evaluator.thresholds_given == thr
    levels = [default_levels(float(np.float32(t))) for t in thr]
    zeros = np.zeros((H, n), np.float32)
    tab = R.restate(R.GO_TO_POSE, obs, zeros, zeros, thr, levels, horizon=H)
    got = player.evaluator.table.cpu().numpy()
    tab[R.RETURN] = got[R.RETURN]   # the rewards were not collected
    _assert_table(got, tab, heading_channel=1, msg="player")   # the same float32 observations: exact but atan2
    want = R.summarize(tab, 2)
    for c, name in enumerate(("position", "heading")):
        o = want[R.S_CH + R.S_CH_STRIDE * c:]
        assert list(summary[name]["table"].values()) == [o[0] / n * 100, o[1] / n * 100, o[2] / n * 100]
        np.testing.assert_allclose(list(summary[name]["time_under"].values()), o[3:6] / (H * n) * 100, rtol=1e-12)
    assert np.isfinite(records["return_raw"]).all()

    from omniisaacgymenvs_loop_amd.scripts import evaluate_policy
    out_csv, out_json = str(tmp_path / "teval.csv"), str(tmp_path / "teval.json")
    rec2, s2 = evaluate_policy.main(["task=USV/USV_Virtual_TrackXYVelocity", "num_envs=256", "eval.horizon=24",
                                     f"eval.output_csv={out_csv}", f"eval.summary_json={out_json}"])
    rows = list(csv.reader(open(out_csv)))
    assert tuple(rows[0]) == task_csv_columns(("xy_velocity",)) and len(rows) - 1 == 256
    s = json.load(open(out_json))
    assert s["envs"] == 256 and s["horizon"] == 24 and s["resets"] == 0 and s["channels"] == ["xy_velocity"]
    assert s["steps_min"] == s["steps_max"] == 24 and len(s["xy_velocity"]["table"]) == 3
    assert all(k.endswith("_m/s") for k in s["xy_velocity"]["table"])
    with pytest.raises(SystemExit, match="eval.horizon"):
        evaluate_policy.main(["task=USV/USV_Virtual_TrackXYVelocity", "num_envs=256", "eval.episodes_per_env=2"])
    with pytest.raises(SystemExit, match="eval.episodes_per_env"):
        evaluate_policy.main(["num_envs=64", "eval.horizon=24"])
