"""Measurements of the batched evaluation (evaluation section).  Recorded, not asserted.

    python profiles/eval_measure.py bytes                     # algorithmic bytes per env, from the shapes
    python profiles/eval_measure.py ab [n] [steps] [blocks]   # rollout ms / step with and without the evaluator,
                                                              # alternating blocks in one process -> JSON line
    python profiles/eval_measure.py steps [n] [steps]         # `steps` evaluated steps, for a kernel trace:
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o eval -- python profiles/eval_measure.py steps
    python profiles/eval_measure.py stats DIR/.../eval_kernel_stats.csv   # the three kernels' rows of that trace
"""
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from omniisaacgymenvs_loop_amd._abi import DEFINES  # noqa: E402


def algorithmic_bytes():
    """Bytes per env the two per-step kernels must move, counted from the buffer shapes (k_eval_mark / k_eval_step
    in csrc/usv_eval.hip); the finished-episode record is extra, once per episode."""
    f32, f64, i32, u8 = 4, 8, 4, 1
    acc = DEFINES["USV_EVA_ROWS"]
    mark_reset_env = u8 + 4 * f32 + acc * f64                  # just_reset, px, py, tgt_x, tgt_y -> 16 acc rows
    mark_other_env = u8
    # step: actions (2), rew, px, py, 16 obstacles x 2, reset_buf; every acc row but the four start / goal rows is
    # read and written
    step_in = (2 + 1 + 2 + 2 * DEFINES["USV_NOBST"]) * f32 + i32
    step_acc = 2 * (acc - 4) * f64
    record = (2 + 1) * f32 + 3 * i32 + 4 * f64 + 2 * i32 + DEFINES["USV_EV_ROWS"] * f64   # tgt, yaw, flags, start/goal
    return {"mark_bytes_per_reset_env": mark_reset_env, "mark_bytes_per_other_env": mark_other_env,
            "step_bytes_per_env": step_in + step_acc, "step_input_bytes": step_in, "step_accumulator_bytes": step_acc,
            "record_bytes_per_finished_episode": record}


def _setup(n):
    import torch
    import yaml

    from omniisaacgymenvs_loop_amd.envs.vec_env_rlgames import VecEnvRLGames
    from omniisaacgymenvs_loop_amd.eval import EpisodeEvaluator
    from omniisaacgymenvs_loop_amd.rl_games.players import PpoPlayerContinuous
    from omniisaacgymenvs_loop_amd.tasks.usv_config import load_yaml
    from omniisaacgymenvs_loop_amd.tasks.usv_virtual import USVVirtual
    pkg = os.path.join(ROOT, "omniisaacgymenvs_loop_amd", "cfg")
    task = USVVirtual(load_yaml(os.path.join(pkg, "task", "USV", "IROS2024", "USV_Virtual_CaptureXY_SysID-TEST.yaml")),
                      num_envs=n, device="cuda:0", seed=42)
    env = VecEnvRLGames(headless=True)
    env.set_task(task)
    with open(os.path.join(pkg, "train", "USV", "USV_PPOcontinuous_MLP.yaml")) as f:
        params = yaml.safe_load(f)["params"]
    params["config"].update(num_actors=n, device="cuda:0", vec_env=env)
    player = PpoPlayerContinuous(params)
    return torch, task, player, EpisodeEvaluator(task, episodes_per_env=1)


def _run(torch, task, player, ev, steps, obs):
    for _ in range(steps):
        obs, _, _ = task.env_step(player.get_action(obs, True), evaluator=ev)
    torch.cuda.synchronize()
    return obs


def ab(n=131072, steps=7, blocks=100, warmup=300):
    """Short alternating blocks: the cost of a step follows the number of envs reset in it (their potential
    fields), a wave with the period of the 200-step time-out that spreads only slowly.  A pair of blocks must
    not divide that period (7 + 7 steps: the pairs drift through the wave), or one arm would always hold the
    wave's step; compare the means over whole periods, not the medians."""
    torch, task, player, ev = _setup(n)
    obs, _, _ = task.env_step(torch.zeros((n, 2), device="cuda:0"))
    obs = _run(torch, task, player, None, warmup, obs)
    obs = _run(torch, task, player, ev, 20, obs)
    ms = {"without": [], "with": []}
    for _ in range(blocks):
        for name, e in (("without", None), ("with", ev)):
            t0 = time.perf_counter()
            obs = _run(torch, task, player, e, steps, obs)
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    ms = {k: [round(x, 4) for x in v] for k, v in ms.items()}
    print(json.dumps({"num_envs": n, "steps_per_block": steps, "blocks": blocks, "warmup_steps": warmup,
                      "ms_per_step": ms, "median_ms_per_step": med, "mean_ms_per_step": mean,
                      "evaluator_overhead_pct_of_means": 100.0 * (mean["with"] - mean["without"]) / mean["without"],
                      "algorithmic_bytes": algorithmic_bytes()}))


def steps_only(n=131072, steps=60):
    torch, task, player, ev = _setup(n)
    obs, _, _ = task.env_step(torch.zeros((n, 2), device="cuda:0"))
    ev.begin()
    _run(torch, task, player, ev, steps, obs)
    print(json.dumps({"num_envs": n, "steps": steps, "summary_episodes": ev.summary()["episodes"]}))


def stats(path):
    rows = [r for r in csv.DictReader(open(path))
            if any(k in r.get("Name", "") for k in ("k_eval_mark", "k_eval_step", "k_env_step", "k_eval_summary"))]
    print(json.dumps([{k: r[k] for k in ("Name", "Calls", "AverageNs", "MinNs", "MaxNs") if k in r} for r in rows]))


if __name__ == "__main__":
    mode, args = sys.argv[1], sys.argv[2:]
    if mode == "bytes":
        print(json.dumps(algorithmic_bytes()))
    elif mode == "ab":
        ab(*[int(a) for a in args])
    elif mode == "steps":
        steps_only(*[int(a) for a in args])
    elif mode == "stats":
        stats(args[0])
