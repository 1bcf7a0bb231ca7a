"""Filter a scenario table by what the teacher can solve (the reference's
omniisaacgymenvs/scripts/teacher_filter_scenario_table.py), every (scenario, rollout) pair as one env's episode.

    python -m omniisaacgymenvs_loop_amd.scripts.teacher_filter \
        task=USV/IROS2024/USV_Virtual_CaptureXY_SysID-TEST num_envs=131072 \
        scenario_npz=runs/scenarios/preselect_300.npz checkpoint=runs/USV/nn/full_2000.pt \
        out_dir=runs/scenarios/teacher_filter [teacher_filter.n_rollouts=1 teacher_filter.n_keep=250
        teacher_filter.n_final=200 teacher_filter.easy_steps_max=80 teacher_filter.easy_margin_min=0.8]

The other overrides are rlgames_train's; num_envs is free (the reference demands 1).  The policy is the loopz
teacher (loopz.LoopzTeacher, deterministic) for a `full_*.pt`, or the rl_games player's clamp(mu) for a `.pth`.
Outputs, under the reference's names: teacher_eval.csv (its columns, one row per scenario), kept_<n>.npz,
final_<n>.npz (scenario.subset) and teacher_filter.meta.json."""
from __future__ import annotations

import csv
import json
import os
import sys
import time

from .rlgames_train import build_config, parse_overrides

DEFAULTS = {"scenario_npz": "", "out_dir": "runs/scenarios/teacher_filter", "teacher_filter.n_rollouts": 1,
            "teacher_filter.n_keep": 250, "teacher_filter.n_final": 200, "teacher_filter.easy_steps_max": 80,
            "teacher_filter.easy_margin_min": 0.8, "teacher_filter.max_steps": ""}


def build_policy(cfg, cfg_dir, env, task):
    """(policy callable, action scale) for cfg["checkpoint"]."""
    path = str(cfg["checkpoint"])
    action_scale = float(cfg["task"]["env"].get("clipActions", 1.0))
    if path.endswith(".pth"):
        from ..rl_games import vecenv
        from ..rl_games.torch_runner import Runner
        vecenv.register("RLGPU", lambda config_name, num_actors, **kw: vecenv.RLGPUEnv(config_name, num_actors, **kw))
        vecenv.register_env("rlgpu", {"vecenv_type": "RLGPU", "env_creator": lambda **kw: env})
        runner = Runner()
        runner.load(cfg["train"])
        player = runner.create_player()
        player.restore(path)
        return (lambda obs: player.get_action(obs, True)), action_scale
    from ..loopz import LoopzTeacher
    from .loopz_train import merge_loopz_overrides
    merge_loopz_overrides(cfg, cfg_dir)
    ec, ac = cfg.get("environment", {}), cfg.get("architecture", {})
    teacher = LoopzTeacher.from_checkpoint(
        path, int(task.num_observations), action_scale=action_scale, device=cfg.get("rl_device", "cuda:0"),
        policy_net=ac.get("policy_net", [128, 128]), speed_dim=int(ec.get("speed_dim", 3)),
        mass_dim=int(ec.get("mass_dim", 8)), mass_latent_dim=int(ac.get("mass_latent_dim", 8)),
        mass_encoder_shape=tuple(int(v) for v in (ac.get("mass_encoder_shape") or (64, 16))))
    return teacher, action_scale


def main(argv=None):
    ov = parse_overrides(sys.argv[1:] if argv is None else argv)
    opt = dict(DEFAULTS)
    for k in list(ov):
        if k in opt:
            opt[k] = ov.pop(k)
        elif k.startswith("teacher_filter."):
            raise SystemExit(f"unknown override {k}")
    if not opt["scenario_npz"]:
        raise SystemExit("Missing scenario_npz=... (e.g. runs/scenarios/preselect_300.npz)")
    if "train" not in ov and not str(ov.get("checkpoint", "")).endswith(".pth"):
        ov["train"] = "USV/USV_MLP"
    cfg_dir = ov.get("cfg_dir", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cfg"))
    cfg = build_config(ov)
    if not cfg["checkpoint"]:
        raise SystemExit("Missing checkpoint=... (a loopz full_*.pt or an rl_games .pth)")
    import torch

    from ..envs.vec_env_rlgames import VecEnvRLGames
    from ..scenario import ScenarioRunner, eval_rows, load_table, save_table, select_keep, subset
    from ..utils.task_util import initialize_task
    scenario_npz, out_dir = str(opt["scenario_npz"]), str(opt["out_dir"])
    n_rollouts = int(opt["teacher_filter.n_rollouts"])
    n_keep, n_final = int(opt["teacher_filter.n_keep"]), int(opt["teacher_filter.n_final"])
    easy_steps_max = int(opt["teacher_filter.easy_steps_max"])
    easy_margin_min = float(opt["teacher_filter.easy_margin_min"])
    table = load_table(scenario_npz)
    n_scenarios = int(table["scenario_id"].shape[0])
    print(f"[teacher-filter] loaded scenario table: {scenario_npz} (n={n_scenarios})")
    env = VecEnvRLGames(headless=True, sim_device=0)
    initialize_task(cfg, env)
    task = env._task
    policy, action_scale = build_policy(cfg, cfg_dir, env, task)
    runner = ScenarioRunner(task, table, rollouts=n_rollouts, action_scale=action_scale,
                            easy_steps_max=easy_steps_max, easy_margin_min=easy_margin_min)
    max_steps = int(opt["teacher_filter.max_steps"]) if opt["teacher_filter.max_steps"] != "" else None
    t0 = time.perf_counter()
    fold = runner.run(policy, max_steps=max_steps)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    print(f"[teacher-filter] {n_scenarios} scenarios x {n_rollouts} rollouts on {runner.n} envs "
          f"({runner.K} per env): {runner.steps_taken} steps in {wall:.3f} s")
    rows = eval_rows(table, fold, runner.max_steps_episode)
    keep_idx, final_idx, sel_summary = select_keep(rows, n_keep, n_final, easy_steps_max, easy_margin_min)
    os.makedirs(out_dir, exist_ok=True)
    eval_csv = os.path.join(out_dir, "teacher_eval.csv")
    with open(eval_csv, "w", encoding="utf-8", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(rows[0].keys()) if rows else [])
        w.writeheader()
        w.writerows(rows)
    extra_meta = {"scenario_npz": scenario_npz, "checkpoint": str(cfg["checkpoint"]), "n_rollouts": n_rollouts,
                  **sel_summary}
    keep_npz = os.path.join(out_dir, f"kept_{int(keep_idx.size)}.npz")
    final_npz = os.path.join(out_dir, f"final_{int(final_idx.size)}.npz")
    save_table(keep_npz, subset(table, keep_idx, extra_meta))
    save_table(final_npz, subset(table, final_idx, extra_meta))
    meta_path = os.path.join(out_dir, "teacher_filter.meta.json")
    with open(meta_path, "w", encoding="utf-8") as f:
        json.dump(extra_meta, f, ensure_ascii=False, indent=2)
    for p in (eval_csv, keep_npz, final_npz, meta_path):
        print(f"[teacher-filter] wrote: {p}")
    return rows, keep_idx, final_idx, extra_meta


if __name__ == "__main__":
    main()
