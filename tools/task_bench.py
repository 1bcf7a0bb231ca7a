"""Step-kernel time and training rate of the non-CaptureXY tasks at one size (default 65,536 envs, BASELINE
configs[3]'s per-GPU share).  bench.py measures the headline and its --task choices are fixed; this measures
the task kinds it does not name, with GoToPose in the same run as the yardstick.

    python tools/task_bench.py GoToXY KeepXY TrackXYVelocity GoToPose [--envs 65536] [--steps 10] [--warmup 3]

Per task one JSON line: step_kernel_us = the median of HIP-event timings of usv_env_step alone (reset kernel not
included; blocks of `--block` back-to-back launches, so launch gaps are inside), env_steps_per_s = envs x horizon
x timed epochs / wall time of A2CAgent.train_epoch (graph-replayed), min / max over the epochs alongside.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build(name, envs, seed):
    from omniisaacgymenvs_loop_amd.envs.vec_env_rlgames import VecEnvRLGames
    from omniisaacgymenvs_loop_amd.rl_games import vecenv
    from omniisaacgymenvs_loop_amd.rl_games.a2c_continuous import A2CAgent
    from omniisaacgymenvs_loop_amd.scripts.rlgames_train import build_config
    from omniisaacgymenvs_loop_amd.utils.task_util import initialize_task
    cfg = build_config({"num_envs": envs, "seed": seed, "task": f"USV/USV_Virtual_{name}"})
    cfg["train"]["params"]["config"].update(train_dir="/tmp/task_bench_runs", print_stats=False, hip_graph=True)
    env = VecEnvRLGames(headless=True)
    task = initialize_task(cfg, env)
    vecenv.register("RLGPU", lambda nm, n, **kw: vecenv.RLGPUEnv(nm, n, **kw))
    vecenv.register_env("rlgpu", {"vecenv_type": "RLGPU", "env_creator": lambda **kw: env})
    return env, task, A2CAgent("run", cfg["train"]["params"])


def step_kernel_us(task, blocks, block):
    """usv_env_step alone on the task's buffers (the envs keep stepping past their dones: timing only)."""
    import torch
    from omniisaacgymenvs_loop_amd import _capi
    act = torch.zeros((task.num_envs, 2), device=task.device)
    cfg, b, s = _capi.byref(task.cfg), _capi.byref(task._bufs), _capi.stream_ptr()
    out = []
    for i in range(blocks + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(block):
            _capi.call("usv_env_step", cfg, b, _capi.ptr(act), _capi.ptr(task.lut), ctypes.c_float(0.0), task.seed, 0,
                       None, s)
        e1.record()
        torch.cuda.synchronize()
        if i:   # the first block warms up
            out.append(e0.elapsed_time(e1) * 1e3 / block)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("tasks", nargs="+")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    import torch
    for name in args.tasks:
        env, task, ag = build(name, args.envs, args.seed)
        ag.obs = ag.env_reset()
        for _ in range(args.warmup):
            ag.train_epoch()
        torch.cuda.synchronize()
        per = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            ag.train_epoch()
            torch.cuda.synchronize()
            per.append(time.perf_counter() - t0)
        env.check_errors()
        frames = args.envs * ag.horizon_length
        ks = step_kernel_us(task, args.blocks, args.block)
        print(json.dumps({"task": name, "envs": args.envs, "step_kernel_us": round(statistics.median(ks), 2),
                          "step_kernel_us_min_max": [round(min(ks), 2), round(max(ks), 2)],
                          "env_steps_per_s": round(frames * len(per) / sum(per)),
                          "env_steps_per_s_min_max": [round(frames / max(per)), round(frames / min(per))],
                          "epochs": len(per), "graph": ag._graph_play is not None}), flush=True)
        del env, task, ag
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
