"""Batched policy evaluation on the GPU (usv_eval_* of libusv_hip.so, eval.EpisodeEvaluator, the env_step hook,
PpoPlayerContinuous.evaluate, scripts/evaluate_policy.py) against the reference-derived fixture
tests/golden/eval_golden.npz and the numpy restatement tests/test_eval_cpu.py validates against it."""
import csv
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import eval_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_KEYS = ("px", "py", "yaw", "vx", "vy", "wz", "fl", "fr")


@pytest.fixture(scope="module")
def eg():
    return dict(np.load(os.path.join(R.GOLDEN, "eval_golden.npz"), allow_pickle=False))


def _task(cfg_d, n, seed=7):
    from omniisaacgymenvs_loop_amd.tasks.usv_virtual import USVVirtual
    return USVVirtual(cfg_d, num_envs=n, device=DEV, seed=seed)


def _kernel_level(tr, cfg_d, K):
    """Drive usv_eval_mark / usv_eval_step from a recorded trajectory written into a task's buffers with torch
    (no env step): returns the evaluator."""
    from omniisaacgymenvs_loop_amd.eval import EpisodeEvaluator
    T, n = tr["px"].shape
    cfg_d = json.loads(json.dumps(cfg_d))
    cfg_d["env"]["scene_replay"] = {"enabled": False}   # scene_last is written by hand below
    task = _task(cfg_d, n)
    task.scene_last = torch.full((n,), -1, device=DEV, dtype=torch.int32)
    task._bufs.scene_last = task.scene_last.data_ptr()
    ev = EpisodeEvaluator(task, episodes_per_env=K)
    dv = {k: torch.tensor(np.ascontiguousarray(v), device=DEV) for k, v in tr.items()}
    obst = dv["obst"].permute(0, 2, 3, 1).reshape(T, 32, n).contiguous()   # [T][n][16][2] -> [T][16][2][n]
    for t in range(T):
        st = dv["started"][t]
        if bool(tr["started"][t].any()):
            # the state right after the reset kernels: spawn, new goal and obstacles, just_reset set
            task.state[0] = torch.where(st, dv["start_x"][t], task.state[0])
            task.state[1] = torch.where(st, dv["start_y"][t], task.state[1])
            task.tgt[0] = torch.where(st, dv["start_gx"][t], task.tgt[0])
            task.tgt[1] = torch.where(st, dv["start_gy"][t], task.tgt[1])
            task.obst.copy_(obst[t])
            task.just_reset.copy_(st.to(torch.uint8))
            ev.mark()
        # the state the env step leaves
        task.just_reset.zero_()
        task.state[0], task.state[1], task.state[2] = dv["px"][t], dv["py"][t], dv["yaw"][t]
        task.tgt[0], task.tgt[1] = dv["tgt_x"][t], dv["tgt_y"][t]
        task.obst.copy_(obst[t])
        task.rew_buf.copy_(dv["rew"][t])
        task.ibuf[2], task.ibuf[3], task.ibuf[4] = dv["done"][t], dv["done_succ"][t], dv["done_coll"][t]
        task.scene_last.copy_(dv["scene_last"][t])
        ev.step(dv["actions"][t].contiguous())
    torch.cuda.synchronize()
    return ev


def _dropped(ev):
    return int(np.maximum(ev.ep_count.cpu().numpy().astype(np.int64) - ev.max_episodes, 0).sum())


@pytest.fixture(scope="module")
def synthetic_run(eg):
    cfg_d = R.fixture_traj("A", eg)[2]
    return _kernel_level(R.synthetic_traj(eg), cfg_d, R.K_EPISODES)


def test_kernels_reproduce_reference_records_of_synthetic_set(eg, synthetic_run):
    """n = 70 (one full wave plus six lanes), 24 steps, K = 3: integers, reasons, flags, slots, the dropped count
    and the float32 distances exactly; doubles at rtol = 1e-12."""
    ev = synthetic_run
    R.assert_records(ev.episodes(), R.golden_records(eg, "C"), msg="synthetic on device")
    assert _dropped(ev) == int(eg["C_dropped"])
    assert ev.control_dt == float(eg["C_control_dt"])


def test_kernels_at_one_env(eg):
    cfg_d = R.fixture_traj("A", eg)[2]
    e = R.ENV_FOUR_ENDINGS
    ev = _kernel_level(R.select_env(R.synthetic_traj(eg), e), cfg_d, R.K_EPISODES)
    want = R.golden_records(eg, "C")
    sel = want["env"] == e
    want1 = {k: (np.zeros(sel.sum(), np.int32) if k == "env" else v[sel]) for k, v in want.items()}
    assert sel.sum() == R.K_EPISODES
    R.assert_records(ev.episodes(), want1, msg="synthetic n=1 on device")
    assert _dropped(ev) == 1


def _check_summary(ev):
    from omniisaacgymenvs_loop_amd.eval import SUMMARY_METRICS, summarize_host
    a = ev.summary_raw().cpu().numpy().copy()
    b = ev.summary_raw().cpu().numpy().copy()
    np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))   # two calls: the same bits
    got, want = ev.summary(), summarize_host(ev.episodes(), _dropped(ev))
    for k in ("episodes", "dropped", "done_reason", "collision", "out_of_bounds"):
        assert got[k] == want[k], k
    assert sum(got["done_reason"].values()) == got["episodes"]
    for k in SUMMARY_METRICS:
        g, w = got["metrics"][k], want["metrics"][k]
        assert g["count"] == w["count"], k
        for q in ("mean", "std", "ci95_lo", "ci95_hi"):
            np.testing.assert_allclose(g[q], w[q], rtol=1e-9, atol=1e-12, equal_nan=True, err_msg=f"{k} {q}")
    return got


def test_summary_matches_numpy_and_is_deterministic(synthetic_run):
    s = _check_summary(synthetic_run)
    assert s["metrics"]["success"]["mean"] > 0 and s["metrics"]["time_to_goal_sec"]["count"] > 0
    assert s["metrics"]["action_smoothness_mean"]["count"] < s["episodes"]   # the one-step episodes' NaN left out
    assert s["dropped"] > 0


def test_summary_of_a_table_without_success(eg):
    tr, _, cfg_d = R.fixture_traj("S", eg)
    ev = _kernel_level(tr, cfg_d, R.K_EPISODES)
    s = _check_summary(ev)
    assert s["episodes"] == 18 and s["metrics"]["success"]["mean"] == 0.0
    ttg = s["metrics"]["time_to_goal_sec"]
    assert ttg["count"] == 0 and np.isnan(ttg["mean"]) and np.isnan(ttg["std"])


@pytest.mark.parametrize("variant", ["A", "S"])
def test_fixture_replay_with_evaluator(eg, variant):
    """The reference's recorded episode through USVVirtual.env_step (post_state mode, as test_fixture_replay_on_gpu)
    with an evaluator attached: the records equal the fixture's, except the return (the float64 running sum of the
    device's own rewards, which are within 1e-5 of the reference's, not bit-equal), the env's own done flags (not in
    the episode fixtures: read back) and, for A, the start-dependent fields (the episode fixture does not record
    the spawn: compared with the restatement fed the device's post-reset state, read inside the hook)."""
    from omniisaacgymenvs_loop_amd.eval import EpisodeEvaluator
    tr, d, cfg_d = R.fixture_traj(variant, eg)
    if cfg_d["env"]["scene_replay"].get("enabled"):
        cfg_d["env"]["scene_replay"]["npz_path"] = os.path.join(R.GOLDEN, "scenes_S.npz")
    T, n = d["px"].shape
    task = _task(cfg_d, n)
    task.cfg.inj_trig = 1
    task.set_grid_lin(torch.tensor(d["grid_lin"]))
    task.set_env_origins(torch.zeros(2, n))
    task.tgt[0] = torch.tensor(d["init_tgt"][:, 0], device=DEV)
    task.tgt[1] = torch.tensor(d["init_tgt"][:, 1], device=DEV)
    spawns = []

    class Spy(EpisodeEvaluator):
        def mark(self):
            super().mark()
            spawns.append(task.state[0:2].clone())

    ev = Spy(task, episodes_per_env=R.K_EPISODES)
    from omniisaacgymenvs_loop_amd._abi import DEFINES
    nu = DEFINES["USV_NU_RESET"]
    reset_U = d["reset_U"]
    if reset_U.shape[1] < nu:
        reset_U = np.concatenate([reset_U, np.zeros((reset_U.shape[0], nu - reset_U.shape[1]), reset_U.dtype)], 1)
    dev = {k: [] for k in ("rew", "done", "done_succ", "done_coll", "scene_last")}
    ru = 0
    for t in range(T):
        ids = np.nonzero(d["reset_mask"][t])[0]
        U = np.zeros((n, nu), np.float32)
        U[ids] = reset_U[ru:ru + len(ids)]
        ru += len(ids)
        post = torch.tensor(np.stack([d[k][t] for k in STATE_KEYS]).astype(np.float32), device=DEV)
        _, rew, dones = task.env_step(torch.tensor(d["actions"][t], device=DEV),
                                      u_step=torch.tensor(d["u_step"][t], device=DEV),
                                      u_reset=torch.tensor(U, device=DEV), post_state=post, evaluator=ev)
        dev["rew"].append(rew.clone())
        dev["done"].append(dones.clone())
        dev["done_succ"].append(task.ibuf[3].clone())
        dev["done_coll"].append(task.ibuf[4].clone())
        dev["scene_last"].append(task.scene_last.clone() if task.scene_last is not None
                                 else torch.full((n,), -1, device=DEV, dtype=torch.int32))
    torch.cuda.synchronize()
    dev = {k: torch.stack(v).cpu().numpy() for k, v in dev.items()}
    sp = torch.stack(spawns).cpu().numpy()
    np.testing.assert_array_equal(dev["done"], d["reset"])
    got, want = ev.episodes(), R.golden_records(eg, variant)
    assert len(got["env"]) == (12 if variant == "A" else 18)
    # the restatement on the device's own rewards, flags and post-reset state
    tr_dev = dict(tr, rew=dev["rew"], done_succ=dev["done_succ"], done_coll=dev["done_coll"],
                  start_x=sp[:, 0], start_y=sp[:, 1])
    own, _ = R.restate(tr_dev, R.thresholds(task.cfg), R.K_EPISODES, ev.control_dt)
    np.testing.assert_allclose(dev["rew"], d["rew"], rtol=1e-5, atol=1e-5)
    own_keys = ("return_raw", "env_done_succ", "env_done_coll") + (R.START_KEYS if variant == "A" else ())
    R.assert_records(got, want, skip=own_keys, msg=f"replay_{variant} vs fixture")
    np.testing.assert_array_equal(got["return_raw"], own["return_raw"])
    R.assert_records(got, own, skip=tuple(k for k in R.INT_KEYS + R.F32_KEYS + R.F64_KEYS if k not in own_keys),
                     msg=f"replay_{variant} vs the restatement on device inputs")
    if variant == "S":   # scene_idx is the fixture's scene_last at each ending, and the device's
        np.testing.assert_array_equal(dev["scene_last"], d["scene_last"])
        ends = {(int(e), k): int(d["scene_last"][t, e]) for e in range(n)
                for k, t in enumerate(np.nonzero(d["reset"][:, e])[0])}
        for e, k, s in zip(got["env"], got["episode"], got["scene_idx"]):
            assert ends[(int(e), int(k))] == s
    else:
        assert (got["scene_idx"] == -1).all()


def test_evaluator_has_no_side_effect():
    """n = 70, 40 steps, in-kernel Philox draws: obs, rew, dones and the state are bit-identical with and without
    an evaluator at every step; the overlapped step refuses one."""
    from omniisaacgymenvs_loop_amd.eval import EpisodeEvaluator
    from omniisaacgymenvs_loop_amd.tasks.usv_config import load_yaml
    cfg_d = load_yaml(os.path.join(ROOT, "omniisaacgymenvs_loop_amd", "cfg", "task", "USV", "IROS2024",
                                   "USV_Virtual_CaptureXY_SysID-TEST.yaml"))
    n, T = 70, 40
    plain, hooked = _task(cfg_d, n, seed=11), _task(cfg_d, n, seed=11)
    ev = EpisodeEvaluator(hooked, episodes_per_env=2)
    g = torch.Generator(device="cpu").manual_seed(3)
    acts = (torch.rand((T, n, 2), generator=g) * 2 - 1).to(DEV)
    outs = {"plain": [], "hooked": []}
    for t in range(T):
        for name, task, kw in (("plain", plain, {}), ("hooked", hooked, {"evaluator": ev})):
            obs, rew, dones = task.env_step(acts[t], **kw)
            outs[name].append((obs.clone(), rew.clone(), dones.clone(), task.state.clone()))
    torch.cuda.synchronize()
    for t in range(T):
        for a, b, what in zip(outs["plain"][t], outs["hooked"][t], ("obs", "rew", "dones", "state")):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b), f"{what} differs at step {t}"
    assert int(ev.ep_count.sum()) == int(sum(o[2].sum() for o in outs["hooked"]))
    with pytest.raises(ValueError, match="evaluator"):
        hooked.env_step(acts[0], overlap=True, evaluator=ev)


def _player(n, max_len):
    import yaml

    from omniisaacgymenvs_loop_amd.envs.vec_env_rlgames import VecEnvRLGames
    from omniisaacgymenvs_loop_amd.rl_games.players import PpoPlayerContinuous
    from omniisaacgymenvs_loop_amd.tasks.usv_config import load_yaml
    cfg_d = load_yaml(os.path.join(ROOT, "omniisaacgymenvs_loop_amd", "cfg", "task", "USV", "IROS2024",
                                   "USV_Virtual_CaptureXY_SysID-TEST.yaml"))
    cfg_d["env"]["maxEpisodeLength"] = max_len
    env = VecEnvRLGames(headless=True)
    env.set_task(_task(cfg_d, n))
    with open(os.path.join(ROOT, "omniisaacgymenvs_loop_amd/cfg/train/USV/USV_PPOcontinuous_MLP.yaml")) as f:
        params = yaml.safe_load(f)["params"]
    params["config"].update(num_actors=n, device=DEV, vec_env=env)
    return PpoPlayerContinuous(params)


def test_player_evaluate_and_script_csv(tmp_path):
    """PpoPlayerContinuous.evaluate(2) on 64 envs with the default-initialised network and short episodes: 128
    records, the summary counts them; the script writes a 128-row CSV and the summary JSON."""
    from omniisaacgymenvs_loop_amd.eval import CSV_COLUMNS
    player = _player(64, 12)
    episodes, summary = player.evaluate(episodes_per_env=2)
    assert len(episodes["env"]) == 128 and summary["episodes"] == 128
    assert sum(summary["done_reason"].values()) == 128
    assert sorted(zip(episodes["env"], episodes["episode"])) == [(e, k) for e in range(64) for k in range(2)]
    assert (episodes["episode_len_steps"] >= 1).all() and (episodes["episode_len_steps"] <= 12).all()
    assert np.isfinite(episodes["return_raw"]).all() and (episodes["path_length"] > 0).all()
    from omniisaacgymenvs_loop_amd.scripts import evaluate_policy
    out_csv, out_json = str(tmp_path / "eval.csv"), str(tmp_path / "eval.json")
    evaluate_policy.main(["num_envs=64", "task.env.maxEpisodeLength=12", "eval.episodes_per_env=2",
                          f"eval.output_csv={out_csv}", f"eval.summary_json={out_json}"])
    rows = list(csv.reader(open(out_csv)))
    assert tuple(rows[0]) == CSV_COLUMNS and len(rows) - 1 == 128
    s = json.load(open(out_json))
    assert s["episodes"] == 128 and s["num_envs"] == 64 and s["control_dt"] == pytest.approx(0.2)
