"""Play a scenario table with the teacher and the student side by side and say, per scenario, what the student lost
(the reference's scripts/rlgames_play_loopz_compare.py with eval.priv_tail_mode, and scripts/dagger_usv_viz_loopz.py
with sysid.zero_latent), every (scenario, rollout) pair as one env's episode.

    python -m omniisaacgymenvs_loop_amd.scripts.compare_policies \
        task=USV/IROS2024/USV_Virtual_CaptureXY_SysID-TEST num_envs=131072 \
        scenario_npz=runs/scenarios/teacher_filter/final_200.npz checkpoint=runs/USV/nn/full_2000.pt \
        id_encoder=runs/sysid/nn/id_encoder_500.pth out_dir=runs/scenarios/compare \
        [compare.arms=teacher,teacher_base_tail,teacher_wrong_tail,student,student_zero_latent
         compare.n_rollouts=1 compare.seed=0 compare.kernel=default compare.max_steps=
         compare.bootstrap=2000 compare.strata=straight_line_dist,d_spawn,d_goal,d_corr,d_oo,density,start_speed
         compare.n_bins=5 compare.min_per_bin=5 compare.boot_seed=0]

The other overrides are teacher_filter's.  Every arm plays a fresh task with the same seed, so with one episode per
env (paired_draws in the output) the arms meet the same scenes with the same reset draws.  The first arm is the
baseline of every pair.  Outputs: compare_scenarios.csv (one row per scenario and arm), compare_pairs.csv (the
paired rows of every other arm against the first) and compare.meta.json (totals with intervals, paired_draws,
wall time per arm).

compare.bootstrap=<n_boot> (default 0: off) adds the analysis stage (scenario.analysis, the reference's
analyze_play_csv.py on the device), every arm against the first: layer0_summary.csv (each arm resampled on its own),
layer0_paired_summary.csv (per-scenario deltas resampled over scenarios) and stratified_effects.csv (the effect
curves over compare.strata), with the reference's headers, in out_dir/<arm>_vs_<first arm>/; the settings go into
compare.meta.json.
Strata: straight_line_dist (the baseline arm's USV_EV_STRAIGHT), d_spawn / d_goal / d_corr / d_oo / density
(usv_scn_metrics of the scene rows) and start_speed (|init_root_vel_xy|)."""
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
            "compare.n_rollouts": 1, "compare.seed": 0, "compare.kernel": "", "compare.max_steps": "",
            "compare.bootstrap": 0, "compare.strata": "", "compare.n_bins": 5, "compare.min_per_bin": 5,
            "compare.boot_seed": 0}
STRATA = ("straight_line_dist", "d_spawn", "d_goal", "d_corr", "d_oo", "density", "start_speed")
ANALYSIS_FILES = {"unpaired": "layer0_summary.csv", "paired": "layer0_paired_summary.csv",
                  "stratified": "stratified_effects.csv"}
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


def split_overrides(ov):
    """(this tool's options, the overrides left for the config) of parsed key=value arguments."""
    ov, opt = dict(ov), dict(DEFAULTS)
    for k in list(ov):
        if k in opt:
            opt[k] = ov.pop(k)
        elif k.startswith("compare."):
            raise SystemExit(f"unknown override {k}")
    return opt, ov


def analysis_options(opt):
    """The analysis stage's settings from the options: n_boot 0 = off."""
    from .._abi import DEFINES
    n_boot = int(opt["compare.bootstrap"] or 0)
    if not 0 <= n_boot <= DEFINES["USV_ANA_MAX_BOOT"]:
        raise SystemExit(f"compare.bootstrap must be in 0..{DEFINES['USV_ANA_MAX_BOOT']}, got {n_boot}")
    raw = opt["compare.strata"]
    strata = [a.strip() for a in (raw.split(",") if isinstance(raw, str) else raw) if str(a).strip()]
    for name in strata:
        if name not in STRATA:
            raise SystemExit(f"unknown stratum {name!r}; known: {', '.join(STRATA)}")
    return {"n_boot": n_boot, "strata": strata, "n_bins": int(opt["compare.n_bins"]),
            "min_per_bin": int(opt["compare.min_per_bin"]), "seed": int(opt["compare.boot_seed"])}


def strata_of(names, table, res, device):
    """name -> a float64 device vector per playlist row [S R] (straight_line_dist) or per scenario [S]."""
    import numpy as np
    import torch

    from .._abi import DEFINES
    from ..scenario import METRIC_KEYS, to_scene_rows
    from ..scenario.analysis import playlist_columns
    from ..scenario.sampling import metrics_device
    from ..scenario.table import meta_of
    out, met = {}, None
    for name in names:
        if name == "straight_line_dist":
            # a playlist row's own record: the baseline arm's where it has one, else the first arm's that has (the
            # start and goal are the scene's), NaN where no arm recorded the row (such a row is not pooled)
            x = None
            for arm in [res["arms"][res["baseline"]]] + [a for k, a in res["arms"].items() if k != res["baseline"]]:
                present, col = playlist_columns(arm["table"], res["n"], res["S"], res["R"], res["episodes_per_env"])
                v = torch.where(present, arm["table"].table[DEFINES["USV_EV_STRAIGHT"]][col],
                                torch.full((), float("nan"), device=device, dtype=torch.float64))
                x = v if x is None else torch.where(torch.isnan(x), v, x)
            out[name] = x
        elif name == "start_speed":
            v = torch.as_tensor(np.asarray(table["init_root_vel_xy"], np.float32), device=device)
            out[name] = torch.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]).double()
        else:
            if met is None:
                rows = torch.as_tensor(to_scene_rows(table), device=device)
                radius = float(meta_of(table).get("obstacle_radius", 0.5))
                met = metrics_device(rows, radius).double()
            out[name] = met[METRIC_KEYS.index("density_score" if name == "density" else name)]
    return out


def write_analysis(out_dir, ana, baseline):
    """The analysis stage's CSVs with the reference's headers, one directory per arm (<arm>_vs_<baseline>, the
    shape of the reference tool's outdir); returns the paths."""
    from ..scenario import analysis as A
    cols = {"unpaired": A.UNPAIRED_COLUMNS, "paired": A.PAIRED_COLUMNS, "stratified": A.STRAT_COLUMNS}
    paths = []
    for name, per in ana.items():
        arm_dir = os.path.join(out_dir, f"{name}_vs_{baseline}")
        os.makedirs(arm_dir, exist_ok=True)
        for kind, fname in ANALYSIS_FILES.items():
            paths.append(os.path.join(arm_dir, fname))
            with open(paths[-1], "w", encoding="utf-8", newline="") as f:
                w = csv.DictWriter(f, fieldnames=cols[kind])
                w.writeheader()
                w.writerows(per[kind])
    return paths


def main(argv=None):
    opt, ov = split_overrides(parse_overrides(sys.argv[1:] if argv is None else argv))
    ana_opt = analysis_options(opt)
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
    written = [scen_csv, pair_csv]
    if ana_opt["n_boot"] > 0:
        from ..scenario.analysis import analyse
        shaper = (cfg.get("train", {}).get("params", {}).get("config", {}) or {}).get("reward_shaper", {}) or {}
        reward_scale = float(shaper.get("scale_value", 1.0))
        ana = analyse(res, reward_scale=reward_scale, n_boot=ana_opt["n_boot"], seed=ana_opt["seed"],
                      strata=strata_of(ana_opt["strata"], table, res, device), n_bins=ana_opt["n_bins"],
                      min_per_bin=ana_opt["min_per_bin"])
        written += write_analysis(out_dir, ana, base)
        meta["analysis"] = {**ana_opt, "reward_scale": reward_scale}
    meta_path = os.path.join(out_dir, "compare.meta.json")
    with open(meta_path, "w", encoding="utf-8") as f:
        json.dump(_clean(meta), f, ensure_ascii=False, indent=2, allow_nan=False)
        f.write("\n")
    for name in names[1:]:
        t = meta["totals"][name]
        sd = t["success_diff"]
        print(f"[compare] {name} vs {base}: pairs={t['pairs']} only_{base}={t['only_a']} only_{name}={t['only_b']} "
              f"success diff={sd['mean']:.4g} 95%CI=[{sd['ci95_lo']:.4g}, {sd['ci95_hi']:.4g}]")
    for p in written + [meta_path]:
        print(f"[compare] wrote: {p}")
    return res, meta


if __name__ == "__main__":
    main()
