"""Play a scenario table with the teacher and the student side by side and say, per scenario, what the student lost
(the reference's scripts/rlgames_play_loopz_compare.py with eval.priv_tail_mode, and scripts/dagger_usv_viz_loopz.py
with sysid.zero_latent), every (scenario, rollout) pair as one env's episode.

    python -m omniisaacgymenvs_loop_amd.scripts.compare_policies \
        task=USV/IROS2024/USV_Virtual_CaptureXY_SysID-TEST num_envs=131072 \
        scenario_npz=runs/scenarios/teacher_filter/final_200.npz checkpoint=runs/USV/nn/full_2000.pt \
        id_encoder=runs/sysid/nn/id_encoder_500.pth out_dir=runs/scenarios/compare \
        [compare.arms=teacher,teacher_base_tail,teacher_wrong_tail,student,student_zero_latent
         compare.n_rollouts=1 compare.seed=0 compare.kernel=default compare.max_steps=]

The other overrides are teacher_filter's.  Every arm plays a fresh task with the same seed, so with one episode per
env (paired_draws in the output) the arms meet the same scenes with the same reset draws.  The first arm is the
baseline of every pair.  Outputs: compare_scenarios.csv (one row per scenario and arm), compare_pairs.csv (the
paired rows of every other arm against the first) and compare.meta.json (totals with intervals, paired_draws,
wall time per arm)."""
from __future__ import annotations

import copy
import csv
import json
import math
import os
import sys

from .rlgames_train import build_config, parse_overrides

ARMS = "teacher,teacher_base_tail,teacher_wrong_tail,student,student_zero_latent"
DEFAULTS = {"scenario_npz": "", "out_dir": "runs/scenarios/compare", "id_encoder": "", "compare.arms": ARMS,
            "compare.n_rollouts": 1, "compare.seed": 0, "compare.kernel": "", "compare.max_steps": ""}
SCENARIO_COLUMNS = ["arm", "scenario_id", "source_preselect_id", "done_reason", "rollouts_present", "success_rate",
                    "collision_rate", "out_of_bounds_rate", "steps", "ep_return_raw", "final_dist_to_goal",
                    "min_obs_dist_min", "min_margin_min"]
PAIR_COLUMNS = ["arm_a", "arm_b", "scenario_id", "source_preselect_id", "pairs", "both_success", "only_a", "only_b",
                "neither", "collision_a", "collision_b", "out_of_bounds_a", "out_of_bounds_b", "d_steps", "d_return",
                "d_final_dist", "d_min_margin"]


def _clean(x):
    """Strict JSON: NaN and infinities become null."""
    if isinstance(x, dict):
        return {k: _clean(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_clean(v) for v in x]
    if isinstance(x, float) and not math.isfinite(x):
        return None
    return x


def main(argv=None):
    ov = parse_overrides(sys.argv[1:] if argv is None else argv)
    opt = dict(DEFAULTS)
    for k in list(ov):
        if k in opt:
            opt[k] = ov.pop(k)
        elif k.startswith("compare."):
            raise SystemExit(f"unknown override {k}")
    if not opt["scenario_npz"]:
        raise SystemExit("Missing scenario_npz=... (e.g. runs/scenarios/teacher_filter/final_200.npz)")
    ov.setdefault("train", "USV/USV_MLP")
    cfg_dir = ov.get("cfg_dir", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cfg"))
    cfg = build_config(ov)
    if not cfg["checkpoint"] or str(cfg["checkpoint"]).endswith(".pth"):
        raise SystemExit("Missing checkpoint=... (the teacher's loopz full_*.pt)")
    arms = opt["compare.arms"]
    names = [a.strip() for a in (arms.split(",") if isinstance(arms, str) else arms) if str(a).strip()]
    from ..envs.vec_env_rlgames import VecEnvRLGames
    from ..loopz import LoopzTeacher
    from ..scenario import ScenarioRunner, eval_rows, load_table
    from ..scenario import compare as C
    from ..sysid.dagger import DEFAULT_PLAY_KERNEL, SysIDStudent
    from ..utils.task_util import initialize_task
    from .loopz_train import merge_loopz_overrides
    merge_loopz_overrides(cfg, cfg_dir)
    ec, ac = cfg.get("environment", {}), cfg.get("architecture", {})
    arch = dict(policy_net=ac.get("policy_net", [128, 128]), speed_dim=int(ec.get("speed_dim", 3)),
                mass_dim=int(ec.get("mass_dim", 8)), mass_latent_dim=int(ac.get("mass_latent_dim", 8)),
                mass_encoder_shape=tuple(int(v) for v in (ac.get("mass_encoder_shape") or (64, 16))))
    device = cfg.get("rl_device", "cuda:0")
    action_scale = float(cfg["task"]["env"].get("clipActions", 1.0))
    scenario_npz, out_dir = str(opt["scenario_npz"]), str(opt["out_dir"])
    n_rollouts, seed = int(opt["compare.n_rollouts"]), int(opt["compare.seed"])
    kernel = str(opt["compare.kernel"]) or DEFAULT_PLAY_KERNEL
    max_steps = int(opt["compare.max_steps"]) if opt["compare.max_steps"] != "" else None
    table = load_table(scenario_npz)
    S = int(table["scenario_id"].shape[0])
    print(f"[compare] loaded scenario table: {scenario_npz} (n={S})")

    def runner_factory():
        env = VecEnvRLGames(headless=True, sim_device=0)
        initialize_task(copy.deepcopy(cfg), env)
        return ScenarioRunner(env._task, table, rollouts=n_rollouts, action_scale=action_scale)

    def make_teacher(runner):
        return LoopzTeacher.from_checkpoint(str(cfg["checkpoint"]), int(runner.task.num_observations),
                                            action_scale=action_scale, device=device, **arch)

    def make_student(runner, zero_latent):
        return SysIDStudent.from_files(str(cfg["checkpoint"]), str(opt["id_encoder"]), num_envs=runner.n,
                                       obs_dim=int(runner.task.num_observations), device=device,
                                       zero_latent=zero_latent, kernel=kernel, **arch)

    factories = C.arm_factories(names, make_teacher, make_student if opt["id_encoder"] else None, seed)
    res = C.compare(runner_factory, factories, max_steps=max_steps)
    if not res["paired_draws"]:
        print(f"[compare] {res['episodes_per_env']} episodes per env: episodes after the first share the scene "
              "only, not the reset draws (paired_draws = false)")
    os.makedirs(out_dir, exist_ok=True)
    scen_csv, pair_csv = os.path.join(out_dir, "compare_scenarios.csv"), os.path.join(out_dir, "compare_pairs.csv")
    with open(scen_csv, "w", encoding="utf-8", newline="") as f:
        w = csv.DictWriter(f, fieldnames=SCENARIO_COLUMNS, extrasaction="ignore")
        w.writeheader()
        for name in names:
            fold = res["arms"][name]["fold"]
            for si, row in enumerate(eval_rows(table, fold, 0)):
                w.writerow({"arm": name, "rollouts_present": int(fold["rollouts_present"][si]), **row})
    base = res["baseline"]
    with open(pair_csv, "w", encoding="utf-8", newline="") as f:
        w = csv.DictWriter(f, fieldnames=PAIR_COLUMNS)
        w.writeheader()
        for name in names[1:]:
            cmp = res["pairs"][name]["scenarios"]
            for si in range(S):
                row = {"arm_a": base, "arm_b": name, "scenario_id": int(table["scenario_id"][si]),
                       "source_preselect_id": si}
                for k in C.CMP_KEYS:
                    row[k] = int(cmp[k][si]) if k in C.CMP_INT_KEYS else float(cmp[k][si])
                w.writerow(row)
    meta = {"scenario_npz": scenario_npz, "checkpoint": str(cfg["checkpoint"]), "id_encoder": str(opt["id_encoder"]),
            "arms": names, "baseline": base, "n_envs": res["n"], "n_scenarios": res["S"], "n_rollouts": res["R"],
            "episodes_per_env": res["episodes_per_env"], "paired_draws": bool(res["paired_draws"]),
            "tail_seed": seed, "student_kernel": kernel,
            "per_arm": {name: {"steps": res["arms"][name]["steps"], "wall_s": res["arms"][name]["wall_s"],
                               "ms_per_step": res["arms"][name]["ms_per_step"],
                               "success_rate_mean": float(res["arms"][name]["fold"]["success_rate"].mean())}
                        for name in names},
            "totals": {name: res["pairs"][name]["totals"] for name in names[1:]}}
    meta_path = os.path.join(out_dir, "compare.meta.json")
    with open(meta_path, "w", encoding="utf-8") as f:
        json.dump(_clean(meta), f, ensure_ascii=False, indent=2, allow_nan=False)
        f.write("\n")
    for name in names[1:]:
        t = meta["totals"][name]
        sd = t["success_diff"]
        print(f"[compare] {name} vs {base}: pairs={t['pairs']} only_{base}={t['only_a']} only_{name}={t['only_b']} "
              f"success diff={sd['mean']:.4g} 95%CI=[{sd['ci95_lo']:.4g}, {sd['ci95_hi']:.4g}]")
    for p in (scen_csv, pair_csv, meta_path):
        print(f"[compare] wrote: {p}")
    return res, meta


if __name__ == "__main__":
    main()
