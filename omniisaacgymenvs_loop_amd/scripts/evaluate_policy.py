"""Evaluate a checkpoint on every env at once: one CSV row per finished episode and a summary
(the reference's env-0 evaluation, omniisaacgymenvs/scripts/rlgames_play_loopz.py, batched on the device).

    python -m omniisaacgymenvs_loop_amd.scripts.evaluate_policy \
        task=USV/IROS2024/USV_Virtual_CaptureXY_SysID-TEST train=USV/USV_PPOcontinuous_MLP \
        checkpoint=runs/USV/nn/last.pth num_envs=131072 \
        eval.episodes_per_env=1 eval.output_csv=eval.csv eval.summary_json=eval.json [eval.max_steps=N]
        [task.env.scene_replay.enabled=True task.env.scene_replay.npz_path=scenes.npz ...]

The task / train / checkpoint / num_envs overrides are rlgames_train's.  With scene replay on, every record carries
the index of the scene its episode ran (scene_idx), so the rows join to the scenario table.  Without a checkpoint
the default-initialised network is evaluated.

A task without obstacles (GoToXY, KeepXY, GoToPose, TrackXYVelocity, TrackXYOVelocity) is evaluated over a fixed
horizon instead (the reference's scripts/evaluate_policy.py with utils/eval_metrics.py: first time under a threshold,
reached-and-stayed, share of time under three levels), one CSV row per env:

    python -m omniisaacgymenvs_loop_amd.scripts.evaluate_policy \
        task=USV/USV_Virtual_GoToPose train=USV/USV_PPOcontinuous_MLP checkpoint=... num_envs=4096 \
        eval.horizon=500 [eval.thresholds=[0.3,0.087]] [eval.levels=[[0.75,0.3,0.15],[0.2,0.087,0.04]]]
        [eval.output_csv=eval.csv eval.summary_json=eval.json]

task.env.fixed_horizon_eval=True (only the time-out ends an episode) and task.env.maxEpisodeLength = horizon + 2 are
set unless given, so no env resets inside the horizon.  The default thresholds are the task's own tolerances."""
from __future__ import annotations

import sys
import time

from .rlgames_train import build_config, parse_overrides

EVAL_DEFAULTS = {"eval.episodes_per_env": 1, "eval.output_csv": "", "eval.summary_json": "", "eval.max_steps": ""}
# the fixed-horizon evaluation of the kinds without obstacles
HORIZON_DEFAULTS = {"eval.horizon": 500, "eval.thresholds": "", "eval.levels": "", "eval.output_csv": "",
                    "eval.summary_json": ""}
CAPTURE_ONLY = ("eval.episodes_per_env", "eval.max_steps")
HORIZON_ONLY = ("eval.horizon", "eval.thresholds", "eval.levels")


def _is_capture(cfg) -> bool:
    from ..tasks.usv_config import TASK_KINDS, build_usv_cfg
    return int(build_usv_cfg(cfg["task"]).task_kind) == TASK_KINDS["CaptureXY"]


def _floats(v, what):
    if v == "":
        return None
    try:
        if isinstance(v, (list, tuple)) and v and isinstance(v[0], (list, tuple)):
            return [[float(x) for x in row] for row in v]
        return [float(x) for x in v] if isinstance(v, (list, tuple)) else [float(v)]
    except (TypeError, ValueError):
        raise SystemExit(f"{what}: a number or a list of numbers expected, got {v!r}")


def _player_of(cfg):
    from ..envs.vec_env_rlgames import VecEnvRLGames
    from ..rl_games import vecenv
    from ..rl_games.torch_runner import Runner
    from ..utils.task_util import initialize_task
    env = VecEnvRLGames(headless=True, sim_device=0)
    initialize_task(cfg, env)
    vecenv.register("RLGPU", lambda config_name, num_actors, **kwargs: vecenv.RLGPUEnv(config_name, num_actors,
                                                                                       **kwargs))
    vecenv.register_env("rlgpu", {"vecenv_type": "RLGPU", "env_creator": lambda **kwargs: env})
    runner = Runner()
    runner.load(cfg["train"])
    player = runner.create_player()
    if cfg["checkpoint"]:
        player.restore(cfg["checkpoint"])
    return player


def main_horizon(ov, ev_ov):
    """The fixed-horizon evaluation: returns (records, summary)."""
    opt = dict(HORIZON_DEFAULTS)
    for k, v in ev_ov.items():
        if k in CAPTURE_ONLY:
            raise SystemExit(f"{k} is for CaptureXY (per-episode records); this task is evaluated over a fixed "
                             "horizon: use eval.horizon")
        if k not in opt:
            raise SystemExit(f"unknown override {k}")
        opt[k] = v
    horizon = int(opt["eval.horizon"])
    if horizon < 1:
        raise SystemExit(f"eval.horizon must be >= 1, got {horizon}")
    ov = dict(ov)
    # the reference script's maxEpisodeLength = horizon + 2 with the kill rules off
    ov.setdefault("task.env.fixed_horizon_eval", True)
    ov.setdefault("task.env.maxEpisodeLength", horizon + 2)
    cfg = build_config(ov)
    import torch

    from ..eval import format_task_summary, write_summary_json, write_task_csv
    player = _player_of(cfg)
    t0 = time.perf_counter()
    records, summary = player.evaluate_horizon(horizon, thresholds=_floats(opt["eval.thresholds"], "eval.thresholds"),
                                               levels=_floats(opt["eval.levels"], "eval.levels"))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ev = player.evaluator
    summary.update(num_envs=int(cfg["num_envs"]), wall_seconds=wall,
                   env_steps_per_second=horizon * ev.n / wall if wall > 0 else float("nan"))
    if opt["eval.output_csv"]:
        rows = write_task_csv(str(opt["eval.output_csv"]), records, ev.channels)
        print(f"[evaluate] wrote {rows} rows to {opt['eval.output_csv']}")
    print(format_task_summary(summary))
    print(f"[evaluate] {horizon} steps x {ev.n} envs in {wall:.3f} s")
    if opt["eval.summary_json"]:
        write_summary_json(str(opt["eval.summary_json"]), summary)
    return records, summary


def main(argv=None):
    ov = parse_overrides(sys.argv[1:] if argv is None else argv)
    ev_ov = {k: ov.pop(k) for k in list(ov) if k.startswith("eval.")}
    cfg = build_config(ov)
    if not _is_capture(cfg):
        return main_horizon(ov, ev_ov)
    opt = dict(EVAL_DEFAULTS)
    for k, v in ev_ov.items():
        if k in HORIZON_ONLY:
            raise SystemExit(f"{k} is for the tasks without obstacles (fixed-horizon evaluation); CaptureXY is "
                             "evaluated per episode: use eval.episodes_per_env")
        if k not in opt:
            raise SystemExit(f"unknown override {k}")
        opt[k] = v
    import torch

    from ..eval import format_summary, write_csv, write_summary_json
    player = _player_of(cfg)
    max_steps = int(opt["eval.max_steps"]) if opt["eval.max_steps"] != "" else None
    t0 = time.perf_counter()
    episodes, summary = player.evaluate(int(opt["eval.episodes_per_env"]), max_steps=max_steps)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ev = player.evaluator
    shaper = cfg["train"]["params"]["config"].get("reward_shaper", {}) or {}
    reward_scale = float(shaper.get("scale_value", 1.0))
    summary.update(num_envs=int(cfg["num_envs"]), episodes_per_env=ev.max_episodes, control_dt=ev.control_dt,
                   reward_scale=reward_scale, wall_seconds=wall,
                   episodes_per_second=summary["episodes"] / wall if wall > 0 else float("nan"))
    if opt["eval.output_csv"]:
        rows = write_csv(str(opt["eval.output_csv"]), episodes, ev.control_dt, reward_scale)
        print(f"[evaluate] wrote {rows} rows to {opt['eval.output_csv']}")
    print(format_summary(summary))
    print(f"[evaluate] {summary['episodes']} episodes in {wall:.3f} s ({summary['episodes_per_second']:.1f} episodes/s)")
    if opt["eval.summary_json"]:
        write_summary_json(str(opt["eval.summary_json"]), summary)
    return episodes, summary


if __name__ == "__main__":
    main()
