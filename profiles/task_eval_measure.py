"""Measurements of the fixed-horizon task evaluation.  Recorded, not asserted.

    python profiles/task_eval_measure.py bytes [task]              # algorithmic bytes per env, from the shapes
    python profiles/task_eval_measure.py ab [n] [steps] [blocks]   # rollout ms / step with and without the
                                                                   # evaluator, alternating blocks in one process
    python profiles/task_eval_measure.py wall [n] [horizon]        # wall time of one evaluate_horizon()
    python profiles/task_eval_measure.py steps [n] [steps]         # `steps` evaluated steps, for a kernel trace:
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o teval -- \
            python profiles/task_eval_measure.py steps
    python profiles/task_eval_measure.py stats DIR/.../teval_kernel_stats.csv   # the kernels' rows of that trace
Every mode prints one JSON line.  The task is GoToPose at 65,536 envs (tools/task_bench.py's size) by default.
"""
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from omniisaacgymenvs_loop_amd._abi import DEFINES  # noqa: E402

TASK = "GoToPose"
CHANNELS = {"GoToXY": 1, "KeepXY": 1, "TrackXYVelocity": 1, "GoToPose": 2, "TrackXYOVelocity": 2}
OBS_COLS = {"GoToXY": 1, "KeepXY": 1, "TrackXYVelocity": 2, "GoToPose": 3, "TrackXYOVelocity": 3}


def algorithmic_bytes(task=TASK):
    """Bytes per env k_teval_step must move, counted from the buffer shapes (csrc/usv_task_eval.hip): the
    observation columns it reads, rew, reset_buf, and the table rows it reads and writes every step (FIRST_THR /
    FIRST_THR2 are read every step and written once; UNDER* are written only under their level: counted as read +
    write, the upper bound).  The observation row is 33 floats at a 132-byte lane stride: the columns share one
    or two 64-byte sectors per env, so the fetched bytes are up to 128 per env whatever the column count."""
    f32, f64, i32 = 4, 8, 4
    ch = CHANNELS[task]
    inputs = OBS_COLS[task] * f32 + f32 + i32
    common = 3 * 2 * f64                                   # STEPS, RETURN, RESETS: read + write
    per_channel = 2 * f64 + 2 * f64 + DEFINES["USV_TEV_LEVELS"] * 2 * f64 + 2 * f64 + f64
    return {"task": task, "step_bytes_per_env": inputs + common + ch * per_channel, "step_input_bytes": inputs,
            "step_table_bytes": common + ch * per_channel,
            "obs_row_bytes_the_step_kernel_stores": DEFINES["USV_NOBS"] * f32,
            "obs_sector_bytes_fetched_upper_bound": 128, "table_bytes_per_env": DEFINES["USV_TEV_ROWS"] * f64}


def _setup(n, horizon, task_name=TASK):
    import torch
    import yaml

    from omniisaacgymenvs_loop_amd.envs.vec_env_rlgames import VecEnvRLGames
    from omniisaacgymenvs_loop_amd.eval import TaskTraceEvaluator
    from omniisaacgymenvs_loop_amd.rl_games.players import PpoPlayerContinuous
    from omniisaacgymenvs_loop_amd.tasks.usv_config import load_yaml
    from omniisaacgymenvs_loop_amd.tasks.usv_virtual import USVVirtual
    pkg = os.path.join(ROOT, "omniisaacgymenvs_loop_amd", "cfg")
    cfg_d = load_yaml(os.path.join(pkg, "task", "USV", f"USV_Virtual_{task_name}.yaml"))
    cfg_d["env"]["fixed_horizon_eval"] = True
    cfg_d["env"]["maxEpisodeLength"] = horizon + 2
    task = USVVirtual(cfg_d, num_envs=n, device="cuda:0", seed=42)
    env = VecEnvRLGames(headless=True)
    env.set_task(task)
    with open(os.path.join(pkg, "train", "USV", "USV_PPOcontinuous_MLP.yaml")) as f:
        params = yaml.safe_load(f)["params"]
    params["config"].update(num_actors=n, device="cuda:0", vec_env=env)
    player = PpoPlayerContinuous(params)
    return torch, task, player, TaskTraceEvaluator(task, horizon)


def _run(torch, task, player, ev, steps, obs):
    for _ in range(steps):
        obs, _, _ = task.env_step(player.get_action(obs, True), evaluator=ev)
    torch.cuda.synchronize()
    return obs


def ab(n=65536, steps=25, blocks=60, warmup=200):
    """Alternating blocks in one process (these kinds have no potential field: a step costs the same whatever
    resets in it, so medians are fair).  The horizon and the episode length are past the run: every step does the
    evaluator's full update and no env resets."""
    torch, task, player, ev = _setup(n, horizon=2 * (warmup + 2 * steps * blocks))
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
    print(json.dumps({"mode": "ab", "task": TASK, "num_envs": n, "steps_per_block": steps, "blocks": blocks,
                      "warmup_steps": warmup, "median_ms_per_step": med, "mean_ms_per_step": mean,
                      "min_ms_per_step": {k: min(v) for k, v in ms.items()},
                      "evaluator_overhead_pct_of_medians": 100.0 * (med["with"] - med["without"]) / med["without"],
                      "algorithmic_bytes": algorithmic_bytes()}))


def wall(n=65536, horizon=500):
    torch, task, player, _ = _setup(n, horizon)
    out = []
    for _ in range(3):   # the first run warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        records, summary = player.evaluate_horizon(horizon)
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    print(json.dumps({"mode": "wall", "task": TASK, "num_envs": n, "horizon": horizon, "wall_seconds": out,
                      "env_steps_per_second": n * horizon / min(out[1:]), "resets": summary["resets"],
                      "steps_min": summary["steps_min"], "steps_max": summary["steps_max"]}))


def steps_only(n=65536, steps=60):
    torch, task, player, ev = _setup(n, steps)
    obs, _, _ = task.env_step(torch.zeros((n, 2), device="cuda:0"))
    ev.begin()
    _run(torch, task, player, ev, steps, obs)
    s = ev.summary()
    print(json.dumps({"mode": "steps", "num_envs": n, "steps": steps, "steps_min": s["steps_min"],
                      "resets": s["resets"]}))


def stats(path):
    keys = ("k_teval_step", "k_teval_begin", "k_teval_summary", "k_env_step", "k_track_finish", "k_reset")
    rows = [r for r in csv.DictReader(open(path)) if any(k in r.get("Name", "") for k in keys)]
    print(json.dumps({"mode": "stats", "kernels": [{k: r[k] for k in ("Name", "Calls", "AverageNs", "MinNs", "MaxNs")
                                                    if k in r} for r in rows]}))


if __name__ == "__main__":
    mode, args = sys.argv[1], sys.argv[2:]
    if mode == "bytes":
        print(json.dumps(algorithmic_bytes(*args)))
    elif mode == "ab":
        ab(*[int(a) for a in args])
    elif mode == "wall":
        wall(*[int(a) for a in args])
    elif mode == "steps":
        steps_only(*[int(a) for a in args])
    elif mode == "stats":
        stats(args[0])
