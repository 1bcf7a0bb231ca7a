"""Evaluate a checkpoint on every env at once: one CSV row per finished episode and a summary
(the reference's env-0 evaluation, omniisaacgymenvs/scripts/rlgames_play_loopz.py, batched on the device).

    python -m omniisaacgymenvs_loop_amd.scripts.evaluate_policy \
        task=USV/IROS2024/USV_Virtual_CaptureXY_SysID-TEST train=USV/USV_PPOcontinuous_MLP \
        checkpoint=runs/USV/nn/last.pth num_envs=131072 \
        eval.episodes_per_env=1 eval.output_csv=eval.csv eval.summary_json=eval.json [eval.max_steps=N]
        [task.env.scene_replay.enabled=True task.env.scene_replay.npz_path=scenes.npz ...]

The task / train / checkpoint / num_envs overrides are rlgames_train's.  With scene replay on, every record carries
the index of the scene its episode ran (scene_idx), so the rows join to the scenario table.  Without a checkpoint
the default-initialised network is evaluated."""
from __future__ import annotations

import sys
import time

from .rlgames_train import build_config, parse_overrides

EVAL_DEFAULTS = {"eval.episodes_per_env": 1, "eval.output_csv": "", "eval.summary_json": "", "eval.max_steps": ""}


def main(argv=None):
    ov = parse_overrides(sys.argv[1:] if argv is None else argv)
    opt = dict(EVAL_DEFAULTS)
    for k in list(ov):
        if k.startswith("eval."):
            if k not in opt:
                raise SystemExit(f"unknown override {k}")
            opt[k] = ov.pop(k)
    cfg = build_config(ov)
    import torch

    from ..envs.vec_env_rlgames import VecEnvRLGames
    from ..eval import format_summary, write_csv, write_summary_json
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
