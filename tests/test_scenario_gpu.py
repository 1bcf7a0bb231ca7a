"""Scenario tables on the device (csrc/usv_scenario.hip, lz_play, scenario.ScenarioRunner, scripts/teacher_filter)
against the reference's recorded outputs (tests/golden/scenario_golden.npz) and the host restatements."""
import csv
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE20 = os.path.join(ROOT, "tests", "golden", "scenario_pre20.npz")
TASK_YAML = os.path.join(ROOT, "omniisaacgymenvs_loop_amd", "cfg", "task", "USV", "IROS2024",
                         "USV_Virtual_CaptureXY_SysID-TEST.yaml")
DEV = "cuda:0"
METRICS = ("d_spawn", "d_goal", "d_corr", "d_oo", "density_score")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def gold(golden):
    return golden("scenario_golden.npz")


def _task(n, seed=7, max_len=12):
    from omniisaacgymenvs_loop_amd.tasks.usv_config import load_yaml
    from omniisaacgymenvs_loop_amd.tasks.usv_virtual import USVVirtual
    cfg_d = load_yaml(TASK_YAML)
    cfg_d["env"]["maxEpisodeLength"] = max_len
    return USVVirtual(cfg_d, num_envs=n, device=DEV, seed=seed)


def _actor(obs_dim, seed=3):
    import torch
    from omniisaacgymenvs_loop_amd.loopz import Actor, MLPEncode_wrap, SquashedGaussianDiagonalCovariance
    arch = MLPEncode_wrap([128, 128], torch.nn.LeakyReLU, obs_dim, 2, torch.nn.Tanh, False, speed_dim=3, mass_dim=8,
                          seed=seed)
    return Actor(arch, SquashedGaussianDiagonalCovariance(2, 0.3, action_scale=[1.0, 0.75]), DEV)


# ------------------------------------------------------------------------------------------------ metrics
@pytest.mark.parametrize("lo,hi", [(0, 67), (41, 42), (40, 41)])
def test_metrics_equal_the_reference_bit_for_bit(gold, lo, hi):
    import torch
    from omniisaacgymenvs_loop_amd._abi import DEFINES as D
    from omniisaacgymenvs_loop_amd.scenario.sampling import metrics_device, metrics_host
    s = hi - lo
    rows = np.zeros((s, D["USV_SCENE_STRIDE"]), np.float32)
    rows[:, :32] = gold["m_obstacles_xy"][lo:hi].reshape(s, 32)
    rows[:, D["USV_SC_START"]:D["USV_SC_START"] + 2] = gold["m_spawn_xy"][lo:hi]
    rows[:, D["USV_SC_GOAL"]:D["USV_SC_GOAL"] + 2] = gold["m_goal_xy"][lo:hi]
    got = metrics_device(torch.from_numpy(rows).to(DEV), 0.5).cpu().numpy()
    want = gold["m_out"][:, lo:hi].astype(np.float32)
    host = metrics_host(gold["m_obstacles_xy"][lo:hi], gold["m_spawn_xy"][lo:hi], gold["m_goal_xy"][lo:hi], 0.5)
    assert got.shape == (5, s) and got.dtype == np.float32
    for i, k in enumerate(METRICS):
        bad = np.nonzero(bits(got[i]) != bits(want[i]))[0]
        assert bad.size == 0, (k, lo + bad, got[i][bad], want[i][bad], host[k][bad])
    assert np.array_equal(np.isposinf(got), np.isposinf(want))
    if (lo, hi) == (0, 67):
        assert np.isposinf(got[:, 40]).all() and np.isposinf(got[3, 41]) and np.isfinite(got[:3, 41]).all()


# ----------------------------------------------------------------------------------------------- generate
def _ulp_close(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("count", [67, 1])
@pytest.mark.parametrize("vel", ["zero", "rand"])
def test_generate_equals_the_host_restatement(count, vel):
    from omniisaacgymenvs_loop_amd._abi import DEFINES as D
    from omniisaacgymenvs_loop_amd.scenario.sampling import SamplingParams, generate_device, philox_host
    p = SamplingParams(init_vel_mode=vel)
    first, seed = 1000, 0x1234567890ABCDEF
    rows_d, quat_d = generate_device(first, count, seed, p, DEV)
    rows, quat = rows_d.cpu().numpy(), quat_d.cpu().numpy()
    want, wquat = philox_host(first, count, seed, p)
    st = slice(D["USV_SC_START"], D["USV_SC_START"] + 2)
    exact = np.ones(D["USV_SCENE_STRIDE"], bool)
    exact[st] = False
    bad = np.nonzero(bits(rows[:, exact]) != bits(want[:, exact]))
    assert bad[0].size == 0, (bad, rows[:, exact][bad], want[:, exact][bad])
    # the double cos / sin may differ in the last place between libm and the device: 1 float32 ulp
    assert _ulp_close(rows[:, st], want[:, st]).all() and _ulp_close(quat, wquat).all()
    assert (quat[:, 1:3] == 0).all()
    if vel == "zero":
        assert (rows[:, D["USV_SC_VEL"]:D["USV_SC_VEL"] + 2] == 0).all()


def _law_check(rows, box, safe):
    from omniisaacgymenvs_loop_amd._abi import DEFINES as D
    n, f = rows.shape[0], np.float32
    obs = rows[:, :32].reshape(n, 16, 2)
    s = rows[:, None, D["USV_SC_START"]:D["USV_SC_START"] + 2]
    g = rows[:, None, D["USV_SC_GOAL"]:D["USV_SC_GOAL"] + 2]
    limbo = (obs == f(999.0)).all(2)
    assert ((obs == f(999.0)).any(2) == limbo).all()        # every other entry is exactly (999, 999)
    for ref in (s, g):
        dx, dy = obs[..., 0] - ref[..., 0], obs[..., 1] - ref[..., 1]
        assert (np.sqrt(dx * dx + dy * dy)[~limbo] >= f(safe)).all()
    lo, hi = g - f(box), g + f(box)                        # the float32 box the draws are mapped into
    inside = (obs >= lo) & (obs <= hi)
    assert inside[~limbo].all()
    return limbo


def test_generate_obeys_the_law_at_4096():
    from omniisaacgymenvs_loop_amd.scenario.sampling import SamplingParams, generate_device
    p = SamplingParams()
    rows = generate_device(0, 4096, 11, p, DEV)[0].cpu().numpy()
    _law_check(rows, p.box_half_range, p.min_dist_safe)
    r = np.hypot(rows[:, 32].astype(np.float64), rows[:, 33].astype(np.float64))
    assert (r >= 0.5 - 1e-6).all() and (r <= 5.0 + 1e-6).all() and (np.abs(rows[:, 37:39]) <= 5.0).all()
    assert (rows[:, 34] >= 0).all() and (rows[:, 34] <= np.float32(np.pi)).all() and (rows[:, 39] == 0).all()
    assert len({r.tobytes() for r in rows}) == 4096


def test_generate_takes_the_limbo_branch():
    from omniisaacgymenvs_loop_amd.scenario.sampling import SamplingParams, generate_device, philox_host
    p = SamplingParams(max_iterations=1, min_dist_safe=12.0, box_half_range=15.0)
    rows = generate_device(0, 67, 5, p, DEV)[0].cpu().numpy()
    limbo = _law_check(rows, 15.0, 12.0)
    assert limbo.any() and not limbo.all()
    assert np.array_equal(bits(rows[:, :32]), bits(philox_host(0, 67, 5, p)[0][:, :32]))


# --------------------------------------------------------------------------------------------------- fold
@pytest.mark.parametrize("case", ["fold_a", "fold_b"])
def test_fold_equals_the_reference_aggregate(gold, case):
    import torch
    from omniisaacgymenvs_loop_amd import _capi
    from omniisaacgymenvs_loop_amd._abi import DEFINES as D
    from omniisaacgymenvs_loop_amd.eval import EpisodeEvaluator
    from omniisaacgymenvs_loop_amd.scenario.runner import fold_to_dict
    p = json.loads(str(gold["fold_params"]))
    ev = EpisodeEvaluator(_task(p["n"]), episodes_per_env=p["K"])
    ev.table.copy_(torch.from_numpy(gold[f"{case}_table"]))
    ev.ep_count.copy_(torch.from_numpy(gold[f"{case}_ep_count"]))
    outs = []
    for _ in range(2):
        out = torch.full((D["USV_SCF_ROWS"], p["S"]), -1.0, device=DEV, dtype=torch.float64)
        _capi.call("usv_scn_fold", _capi.byref(ev._ev), p["n"], p["S"], p["R"], p["K"], p["collision_threshold"],
                   p["easy_steps_max"], p["easy_margin_min"], p["max_steps"], _capi.ptr(out), _capi.stream_ptr())
        outs.append(out.cpu().numpy())
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    got = fold_to_dict(outs[0])
    for k, g in (("rollouts_present", "present"), ("collision_any", "collision_any"), ("reason", "reason"),
                 ("out_of_bounds_any", "out_of_bounds_any"), ("steps", "steps"), ("verdict", "verdict")):
        assert np.array_equal(got[k], gold[f"{case}_{g}"]), (k, got[k], gold[f"{case}_{g}"])
    for k in ("success_rate", "collision_rate", "out_of_bounds_rate", "ep_return_raw", "final_dist_to_goal",
              "min_obs_dist_min", "min_margin_min", "difficulty"):
        # doubles that differ only in summation order
        np.testing.assert_allclose(got[k], gold[f"{case}_{k}"], rtol=1e-12, atol=0, err_msg=k)


# ------------------------------------------------------------------------------------------------ lz_play
@pytest.mark.parametrize("n", [1, 70])
@pytest.mark.parametrize("obs_dim", [33, 36])
def test_lz_play_equals_lz_act_without_noise(n, obs_dim):
    import torch
    from omniisaacgymenvs_loop_amd.loopz import PPO, Critic, LoopzTeacher, MLPEncode_wrap
    actor = _actor(obs_dim)
    critic = Critic(MLPEncode_wrap([128, 128], torch.nn.LeakyReLU, obs_dim, 1, speed_dim=3, mass_dim=8, seed=4), DEV)
    teacher = LoopzTeacher(actor, DEV)
    ppo = PPO(actor, critic, num_envs=n, num_transitions_per_env=1, num_learning_epochs=1, num_mini_batches=1,
              device=DEV, mini_batch_sampling="in_order")
    gen = torch.Generator().manual_seed(n * 100 + obs_dim)
    obs = (torch.randn((n, obs_dim), generator=gen) * 2.0).to(DEV)
    want = ppo.observe_device(obs, eps_inject=torch.zeros((n, 2), device=DEV)).cpu().numpy().copy()
    got = teacher(obs).cpu().numpy()
    assert got.shape == (n, 2) and np.array_equal(bits(got), bits(want))
    assert np.abs(got).max() > 1e-3 and (np.abs(got[:, 1]) <= 0.75).all()
    # deterministic: nothing is drawn
    assert np.array_equal(bits(teacher(obs).cpu().numpy()), bits(got))


# --------------------------------------------------------------------------------------------- end to end
def _numpy_fold(ep, S, R, K, thr, easy_steps, easy_margin, max_steps):
    """The filter's aggregate (:712-759) and verdict of evaluator.episodes() in numpy, per scenario."""
    from omniisaacgymenvs_loop_amd.eval.report import REASON_NAMES
    from omniisaacgymenvs_loop_amd.scenario.filter import difficulty, select_keep
    p = ep["env"].astype(np.int64) * K + ep["episode"]
    out = []
    for s in range(S):
        sel = [int(np.nonzero(p == s * R + r)[0][0]) for r in range(R)]
        reasons = [REASON_NAMES[int(ep["done_reason"][i])] for i in sel]
        succ = float(np.mean([1.0 if r == "goal_tolerance" else 0.0 for r in reasons]))
        ca, oa = int("collision" in reasons), int("out_of_bounds" in reasons)
        reason = 0 if ca else 1 if oa else 2 if succ >= 1.0 - 1e-9 else 4 if succ > 0.0 else 3
        mo = [float(ep["min_obs_dist_episode"][i]) for i in sel]
        row = {"scenario_id": s, "success_rate": succ, "collision_any": ca, "out_of_bounds_any": oa, "reason": reason,
               "collision_rate": float(np.mean([r == "collision" for r in reasons])),
               "out_of_bounds_rate": float(np.mean([r == "out_of_bounds" for r in reasons])),
               "steps": int(np.mean([int(ep["episode_len_steps"][i]) for i in sel])),
               "ep_return_raw": float(np.mean([ep["return_raw"][i] for i in sel])),
               "final_dist_to_goal": float(np.mean([ep["dist_to_goal"][i] for i in sel])),
               "min_obs_dist_min": min([m for m in mo if np.isfinite(m)] or [np.inf]),
               "min_margin_min": min([m - thr for m in mo if np.isfinite(m)] or [np.inf]), "max_steps": max_steps}
        one = select_keep([row], 1, 1, easy_steps, easy_margin)[2]
        row["verdict"] = 1 if one["n_hard_reject"] else 2 if one["n_easy_reject"] else 0
        row["difficulty"] = difficulty(row["steps"], row["min_margin_min"], max_steps)
        out.append(row)
    return out


@pytest.mark.parametrize("R,K,pad", [(3, 1, 4), (5, 2, 28)])
def test_runner_end_to_end(R, K, pad):
    import torch
    from omniisaacgymenvs_loop_amd._abi import DEFINES as D
    from omniisaacgymenvs_loop_amd.loopz import LoopzTeacher
    from omniisaacgymenvs_loop_amd.scenario import ScenarioRunner, load_table
    table = load_table(PRE20)
    n, S = 64, 20
    assert K * n - S * R == pad

    def play(policy_of):
        task = _task(n, seed=21)
        runner = ScenarioRunner(task, table, rollouts=R)
        assert (runner.K, runner.rows.shape[0]) == (K, K * n)
        fold = runner.run(policy_of(task))
        return runner, fold

    teacher_of = lambda task: LoopzTeacher(_actor(int(task.num_observations)), DEV)
    runner, fold = play(teacher_of)
    ev = runner.evaluator
    tab, cnt = ev.table.cpu().numpy(), ev.ep_count.cpu().numpy()
    assert (cnt >= K).all() and (fold["rollouts_present"] == R).all()
    e, k = np.meshgrid(np.arange(n), np.arange(K), indexing="ij")
    col = (k * n + e).reshape(-1)
    scene = tab[D["USV_EV_SCENE_IDX"]][col]
    assert np.array_equal(scene, (e * K + k).reshape(-1))
    sc = (scene.astype(np.int64) % (S * R)) // R
    for row, want in ((D["USV_EV_START_X"], table["spawn_root_pos"][sc, 0]), (D["USV_EV_START_Y"], table["spawn_root_pos"][sc, 1]),
                      (D["USV_EV_GOAL_X"], table["target_pos"][sc, 0]), (D["USV_EV_GOAL_Y"], table["target_pos"][sc, 1])):
        assert np.array_equal(tab[row][col], want.astype(np.float64))
    # the device fold against a numpy fold of the evaluator's episodes
    want = _numpy_fold(ev.episodes(), S, R, K, runner.collision_threshold, runner.easy_steps_max,
                       runner.easy_margin_min, runner.max_steps_episode)
    for key in ("collision_any", "out_of_bounds_any", "reason", "steps", "verdict"):
        assert np.array_equal(fold[key], [w[key] for w in want]), key
    for key in ("success_rate", "collision_rate", "out_of_bounds_rate", "ep_return_raw", "final_dist_to_goal",
                "min_obs_dist_min", "min_margin_min", "difficulty"):
        np.testing.assert_allclose(fold[key], [w[key] for w in want], rtol=1e-12, atol=0, err_msg=key)
    assert (fold["steps"] >= 1).all() and (fold["steps"] <= 12).all()
    # a second run gives the same bits
    runner2, fold2 = play(teacher_of)
    assert np.array_equal(bits(runner2._out.cpu().numpy()), bits(runner._out.cpu().numpy()))
    assert np.array_equal(bits(runner2.evaluator.table.cpu().numpy()[:, col]), bits(tab[:, col]))
    # another policy: the same starts and goals in every (env, episode 0)
    zero = torch.zeros((n, 2), device=DEV)
    runner3, _ = play(lambda task: (lambda obs: zero))
    tab3 = runner3.evaluator.table.cpu().numpy()
    for row in ("START_X", "START_Y", "GOAL_X", "GOAL_Y", "SCENE_IDX"):
        assert np.array_equal(tab3[D[f"USV_EV_{row}"]][:n], tab[D[f"USV_EV_{row}"]][:n]), row


def test_runner_refuses_incomplete_scenarios():
    import torch
    from omniisaacgymenvs_loop_amd.scenario import ScenarioRunner, load_table
    task = _task(64, seed=21)
    runner = ScenarioRunner(task, load_table(PRE20), rollouts=5)
    zero = torch.zeros((64, 2), device=DEV)
    with pytest.raises(RuntimeError, match="without a record"):
        runner.run(lambda obs: zero, max_steps=13)   # K = 2 episodes of 12 steps do not fit
    fold = runner.run(lambda obs: zero, max_steps=13, allow_incomplete=True)
    assert (fold["verdict"][fold["rollouts_present"] < 5] == 3).all() and (fold["rollouts_present"] < 5).any()


def test_set_scene_table_checks_its_arguments():
    import torch
    task = _task(8)
    rows = torch.zeros((4, 40), device=DEV)
    first = torch.zeros(8, device=DEV, dtype=torch.int32)
    with pytest.raises(ValueError):
        task.set_scene_table(rows[:, :39].contiguous(), first)
    with pytest.raises(ValueError):
        task.set_scene_table(rows, first[:4])
    task.set_scene_table(rows, first)
    assert task.scene_replay_num_scenes == 4 and int(task.scene_last.max()) == -1


# ------------------------------------------------------------------------------------------- command line
def test_scenario_table_main_with_the_device_sampler(tmp_path):
    from omniisaacgymenvs_loop_amd.scenario import load_table, metrics_host, philox_host, SamplingParams
    from omniisaacgymenvs_loop_amd.scripts import scenario_table
    out = str(tmp_path / "scenarios")
    files = scenario_table.main(["--sampler", "philox", "--n-candidates", "300", "--n-preselect", "100", "--n-selected",
                                 "20", "--seed", "9", "--save-candidates", "--out-dir", out])
    assert files == ["candidates_300_unique.npz", "preselect_100.npz", "selected_20.npz", "scenario_table.meta.json"]
    cand, pre = load_table(os.path.join(out, files[0])), load_table(os.path.join(out, files[1]))
    assert len(set(cand["obstacles_hash"])) == 300 and np.array_equal(cand["scenario_id"], np.arange(300))
    rows, _ = philox_host(0, 300, 9, SamplingParams())   # the candidates are the device sampler's, in order
    assert np.array_equal(bits(cand["obstacles_xy"].reshape(300, 32)), bits(rows[:, :32]))
    host = metrics_host(cand["obstacles_xy"], cand["spawn_root_pos"][:, :2], cand["target_pos"][:, :2], 0.5)
    for k in METRICS:   # the device metrics of the device rows
        assert np.array_equal(bits(cand[k]), bits(host[k].astype(np.float32))), k
    src = pre["source_candidate_id"]
    assert len(set(src)) == 100 and np.array_equal(bits(pre["obstacles_xy"]), bits(cand["obstacles_xy"][src]))
    assert json.loads(pre["meta"])["sampler"] == "philox"
    assert load_table(os.path.join(out, files[2]))["scenario_id"].shape == (20,)


def test_teacher_filter_main(tmp_path, monkeypatch):
    import torch
    from omniisaacgymenvs_loop_amd.scenario import CSV_COLUMNS, load_table
    from omniisaacgymenvs_loop_amd.scripts import teacher_filter
    monkeypatch.chdir(tmp_path)
    actor = _actor(33)
    ckpt = str(tmp_path / "full_0.pt")
    torch.save({"actor_architecture_state_dict": actor.architecture.state_dict(),
                "actor_distribution_state_dict": actor.distribution.state_dict()}, ckpt)
    out_dir = str(tmp_path / "filter")
    rows, keep_idx, final_idx, meta = teacher_filter.main(
        ["num_envs=64", "task.env.maxEpisodeLength=12", f"scenario_npz={PRE20}", f"checkpoint={ckpt}",
         f"out_dir={out_dir}", "teacher_filter.n_rollouts=2", "teacher_filter.n_keep=5", "teacher_filter.n_final=3"])
    files = sorted(os.listdir(out_dir))
    kept, final = f"kept_{keep_idx.size}.npz", f"final_{final_idx.size}.npz"
    assert files == sorted({kept, final, "teacher_eval.csv", "teacher_filter.meta.json"})
    table = list(csv.reader(open(os.path.join(out_dir, "teacher_eval.csv"))))
    assert table[0] == CSV_COLUMNS + ["source_candidate_id"] and len(table) - 1 == 20 == len(rows)
    t = load_table(os.path.join(out_dir, kept))
    assert np.array_equal(t["source_preselect_id"], keep_idx)
    assert np.array_equal(t["scenario_id"], np.arange(keep_idx.size))
    assert json.loads(t["meta"])["teacher_filter"] == meta and meta["n_rollouts"] == 2 and meta["n_total"] == 20
    assert json.load(open(os.path.join(out_dir, "teacher_filter.meta.json"))) == meta
    assert final_idx.size <= 3 and keep_idx.size <= 5
