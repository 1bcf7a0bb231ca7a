"""Host side of the evaluation report: the episode table as a CSV (the reference's column names where it has
them, scripts/rlgames_play_loopz.py:989-1030, 1380-1401) and the summary in its "metric: mean std CI" form
(:1046-1073).  Pure numpy / stdlib: no device needed.

The interval is the normal approximation mean +- 1.96 std / sqrt(count) on the finite values; the reference's
2,000-resample bootstrap (:504-530) is not run here (evaluation section; the comparison stage resamples on
the device, scenario.analysis)."""
from __future__ import annotations

import csv
import json
import math
from typing import Any, Dict

import numpy as np

from .._abi import DEFINES

REASON_NAMES = ("collision", "out_of_bounds", "goal_tolerance", "other")   # USV_EV_REASON_* order
assert [DEFINES[f"USV_EV_REASON_{k}"] for k in ("COLLISION", "OOB", "GOAL", "OTHER")] == [0, 1, 2, 3]
# _summarize_eval's metrics, in its order (= USV_EVS_METRICS order)
SUMMARY_METRICS = ("success", "time_to_goal_sec", "path_efficiency", "action_smoothness_mean",
                   "action_saturation_rate", "return_raw")
assert len(SUMMARY_METRICS) == DEFINES["USV_EVS_NMETRIC"]

# episode dict key -> (USV_EV_* row, dtype the value is exact in)
EPISODE_FIELDS = {
    "success": ("SUCCESS", np.int32), "done_reason": ("REASON", np.int32),
    "episode_len_steps": ("LEN_STEPS", np.int32), "time_to_goal_sec": ("TIME_TO_GOAL", np.float64),
    "return_raw": ("RETURN", np.float64), "path_length": ("PATH_LENGTH", np.float64),
    "straight_line_dist": ("STRAIGHT", np.float64), "path_efficiency": ("PATH_EFF", np.float64),
    "action_smoothness_mean": ("SMOOTH_MEAN", np.float64), "action_smoothness_sum": ("SMOOTH_SUM", np.float64),
    "action_saturation_rate": ("SAT_RATE", np.float64), "collision": ("COLLISION", np.int32),
    "out_of_bounds": ("OOB", np.int32), "in_goal_tolerance": ("IN_TOL", np.int32),
    "dist_to_goal": ("DIST_TO_GOAL", np.float64),
    "start_x": ("START_X", np.float32), "start_y": ("START_Y", np.float32),
    "goal_x": ("GOAL_X", np.float32), "goal_y": ("GOAL_Y", np.float32),
    "end_x": ("END_X", np.float32), "end_y": ("END_Y", np.float32), "end_yaw": ("END_YAW", np.float32),
    "min_obs_dist_end": ("MIN_OBS_END", np.float32), "min_obs_dist_episode": ("MIN_OBS_EP", np.float32),
    "scene_idx": ("SCENE_IDX", np.int32), "env_done_succ": ("ENV_SUCC", np.int32),
    "env_done_coll": ("ENV_COLL", np.int32), "action_delta_count": ("SMOOTH_COUNT", np.int32),
    "action_saturation_count": ("SAT_COUNT", np.int32),
}

# the reference's columns first (its names), then this project's own
CSV_COLUMNS = ("success", "done_reason", "episode_len_steps", "time_to_goal_sec", "return_raw", "return_scaled",
               "path_length", "straight_line_dist", "path_efficiency", "action_smoothness_mean",
               "action_smoothness_sum", "action_saturation_rate", "collision", "out_of_bounds", "control_dt",
               "reward_scale",
               "env", "episode", "scene_idx", "start_x", "start_y", "goal_x", "goal_y", "end_x", "end_y", "end_yaw",
               "min_obs_dist_end", "min_obs_dist_episode", "env_done_succ", "env_done_coll")


def table_to_episodes(table: np.ndarray, ep_count: np.ndarray, max_episodes: int) -> Dict[str, np.ndarray]:
    """The device table ([USV_EV_ROWS][K * n] doubles) and the per-env finished counts as a dict of arrays with
    one entry per kept episode, in column order (episode-major: episode 0 of every env, then episode 1, ...)."""
    n = int(ep_count.shape[0])
    k_idx, e_idx = np.divmod(np.arange(max_episodes * n), n)
    keep = k_idx < np.minimum(ep_count, max_episodes)[e_idx]
    out = {"env": e_idx[keep].astype(np.int32), "episode": k_idx[keep].astype(np.int32)}
    for key, (row, dt) in EPISODE_FIELDS.items():
        out[key] = table[DEFINES[f"USV_EV_{row}"]][keep].astype(dt)
    return out


def _fmt(v: Any) -> str:
    """CSV cell: integers as integers, floats by repr (round-trips), NaN as 'nan'."""
    if isinstance(v, (str, int, np.integer)):
        return str(v)
    v = float(v)
    return "nan" if math.isnan(v) else repr(v)


def write_csv(path: str, episodes: Dict[str, np.ndarray], control_dt: float, reward_scale: float = 1.0) -> int:
    """One row per episode, CSV_COLUMNS order; returns the row count.  return_scaled = return_raw x reward_scale
    (the reference sums reward x scale per step; equal for scale 1, within rounding otherwise)."""
    rows = int(episodes["env"].shape[0])
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS)
        for i in range(rows):
            rec = {k: episodes[k][i] for k in CSV_COLUMNS if k in episodes}
            rec["done_reason"] = REASON_NAMES[int(episodes["done_reason"][i])]
            rec["return_scaled"] = float(episodes["return_raw"][i]) * float(reward_scale)
            rec["control_dt"], rec["reward_scale"] = float(control_dt), float(reward_scale)
            w.writerow([_fmt(rec[k]) for k in CSV_COLUMNS])
    return rows


def _with_ci(count: int, mean: float, std: float) -> Dict[str, float]:
    half = 1.96 * std / math.sqrt(count) if count > 0 else float("nan")
    return {"count": int(count), "mean": float(mean), "std": float(std), "ci95_lo": float(mean - half),
            "ci95_hi": float(mean + half)}


def summary_from_device(out: np.ndarray) -> Dict[str, Any]:
    """usv_eval_summary's [USV_EVS_N] doubles as a dict, plus the host's normal-approximation 95 % interval."""
    s: Dict[str, Any] = {"episodes": int(out[DEFINES["USV_EVS_EPISODES"]]),
                         "dropped": int(out[DEFINES["USV_EVS_DROPPED"]]),
                         "done_reason": {k: int(out[DEFINES["USV_EVS_REASONS"] + i])
                                         for i, k in enumerate(REASON_NAMES)},
                         "collision": int(out[DEFINES["USV_EVS_COLLISION"]]),
                         "out_of_bounds": int(out[DEFINES["USV_EVS_OOB"]]), "metrics": {}}
    m0 = DEFINES["USV_EVS_METRICS"]
    for i, k in enumerate(SUMMARY_METRICS):
        s["metrics"][k] = _with_ci(int(out[m0 + 3 * i]), out[m0 + 3 * i + 1], out[m0 + 3 * i + 2])
    return s


def summarize_host(episodes: Dict[str, np.ndarray], dropped: int = 0) -> Dict[str, Any]:
    """The same summary from an episode dict with numpy (np.mean / np.std, ddof = 0, over the finite values):
    what the device summary is checked against."""
    s: Dict[str, Any] = {"episodes": int(episodes["env"].shape[0]), "dropped": int(dropped),
                         "done_reason": {k: int((episodes["done_reason"] == i).sum())
                                         for i, k in enumerate(REASON_NAMES)},
                         "collision": int(episodes["collision"].sum()),
                         "out_of_bounds": int(episodes["out_of_bounds"].sum()), "metrics": {}}
    for k in SUMMARY_METRICS:
        v = np.asarray(episodes[k], np.float64)
        v = v[np.isfinite(v)]
        s["metrics"][k] = (_with_ci(v.size, float(np.mean(v)), float(np.std(v))) if v.size
                           else _with_ci(0, float("nan"), float("nan")))
    return s


def format_summary(s: Dict[str, Any]) -> str:
    """The reference's summary lines (play_loopz.py:1065-1073)."""
    lines = [f"[evaluate] episodes={s['episodes']} dropped={s['dropped']} "
             + " ".join(f"{k}={v}" for k, v in s["done_reason"].items())]
    for k in SUMMARY_METRICS:
        m = s["metrics"][k]
        lines.append(f"  {k}: mean={m['mean']:.6g} std={m['std']:.6g} 95%CI=[{m['ci95_lo']:.6g}, {m['ci95_hi']:.6g}]")
    return "\n".join(lines)


def write_summary_json(path: str, s: Dict[str, Any]) -> None:
    """Strict JSON: NaN (a metric without a finite value) is written as null."""
    def clean(x):
        if isinstance(x, dict):
            return {k: clean(v) for k, v in x.items()}
        if isinstance(x, float) and not math.isfinite(x):
            return None
        return x
    with open(path, "w") as f:
        json.dump(clean(s), f, indent=2, allow_nan=False)
        f.write("\n")


# ---- fixed-horizon success-rate evaluation (usv_teval_*, eval.task_evaluator) -------------------------------
# the reference's tables (utils/eval_metrics.py): group key -> unit suffix of its column names, and the prefix of
# the time-under rows (its PT5 / PT2 / PT1 and OT5 / OT2 / OT1 are position and heading; the others in that style)
TASK_UNITS = {"position": "m", "heading": "rad", "xy_velocity": "m/s", "omega_velocity": "rad/s"}
TASK_TIME_UNDER_PREFIX = {"position": "PT", "heading": "OT", "xy_velocity": "VT", "omega_velocity": "WT"}
TASK_CHANNEL_FIELDS = ("first_thr", "first_thr2", "stay", "under0", "under1", "under2", "err_mean", "err_last")


def task_column_names(channel: str, thr: float) -> tuple:
    """The reference's three column names for a channel at threshold thr (a Python float, formatted as it does)."""
    u = TASK_UNITS[channel]
    return (f"success_rate_{thr}_{u}", f"success_rate_{thr / 2}_{u}", f"success_and_stay_within_{thr * 7.5}_{u}")


def task_csv_columns(channels) -> tuple:
    return ("env", "steps", "return_raw", "resets") + tuple(f"{c}_{f}" for c in channels for f in TASK_CHANNEL_FIELDS)


def task_records_from_table(table: np.ndarray, channels, horizon: int) -> Dict[str, np.ndarray]:
    """The device table ([USV_TEV_ROWS][n] doubles) as per-env arrays."""
    n = table.shape[1]
    steps = table[DEFINES["USV_TEV_STEPS"]].astype(np.int64)
    out = {"env": np.arange(n, dtype=np.int32), "steps": steps,
           "return_raw": table[DEFINES["USV_TEV_RETURN"]].copy(),
           "resets": table[DEFINES["USV_TEV_RESETS"]].astype(np.int64)}
    seen = np.maximum(np.minimum(steps, int(horizon)), 1)
    for c, name in enumerate(channels):
        r = table[DEFINES["USV_TEV_CH_STRIDE"] * c:DEFINES["USV_TEV_CH_STRIDE"] * (c + 1)]
        out[f"{name}_first_thr"] = r[DEFINES["USV_TEV_FIRST_THR"]].astype(np.int64)
        out[f"{name}_first_thr2"] = r[DEFINES["USV_TEV_FIRST_THR2"]].astype(np.int64)
        out[f"{name}_stay"] = r[DEFINES["USV_TEV_STAY"]].astype(np.int32)
        for l in range(DEFINES["USV_TEV_LEVELS"]):
            out[f"{name}_under{l}"] = r[DEFINES["USV_TEV_UNDER0"] + l].astype(np.int64)
        out[f"{name}_err_mean"] = r[DEFINES["USV_TEV_ERR_SUM"]] / seen
        out[f"{name}_err_last"] = r[DEFINES["USV_TEV_ERR_LAST"]].copy()
    return out


def write_task_csv(path: str, records: Dict[str, np.ndarray], channels) -> int:
    """One row per env, task_csv_columns order; returns the row count."""
    cols = task_csv_columns(channels)
    rows = int(records["env"].shape[0])
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(cols)
        for i in range(rows):
            w.writerow([_fmt(records[k][i]) for k in cols])
    return rows


def task_summary_from_device(out: np.ndarray, channels, thresholds, thresholds_f32, levels,
                             horizon: int) -> Dict[str, Any]:
    """usv_teval_summary's [USV_TEVS_N] doubles as the reference's tables: per channel group key a "table" with
    its three column names (percentages: mean(first_thr > -1) * 100, the same for thr / 2, mean(stay) * 100) and
    the "time_under" percentages of all (step, env) pairs.  thresholds: as given (they name the columns);
    thresholds_f32: what the device compared with."""
    envs = int(out[DEFINES["USV_TEVS_ENVS"]])
    smin, smax = int(out[DEFINES["USV_TEVS_STEPS_MIN"]]), int(out[DEFINES["USV_TEVS_STEPS_MAX"]])
    s: Dict[str, Any] = {"envs": envs, "channels": list(channels), "horizon": int(horizon), "steps_min": smin,
                         "steps_max": smax, "resets": int(out[DEFINES["USV_TEVS_RESETS"]]),
                         "envs_reset": int(out[DEFINES["USV_TEVS_RESET_ENVS"]])}
    r0 = DEFINES["USV_TEVS_RETURN"]
    s["return_raw"] = _with_ci(int(out[r0]), out[r0 + 1], out[r0 + 2])
    pairs = float(max(min(smin, int(horizon)), 1) * max(envs, 1))
    for c, name in enumerate(channels):
        o = out[DEFINES["USV_TEVS_CH"] + DEFINES["USV_TEVS_CH_STRIDE"] * c:]
        names = task_column_names(name, float(thresholds[c]))
        rates = (o[DEFINES["USV_TEVS_N_THR"]] / envs * 100, o[DEFINES["USV_TEVS_N_THR2"]] / envs * 100,
                 o[DEFINES["USV_TEVS_N_STAY"]] / envs * 100)
        under = [float(o[DEFINES["USV_TEVS_UNDER"] + l]) for l in range(DEFINES["USV_TEV_LEVELS"])]
        s[name] = {"threshold": float(thresholds[c]), "threshold_f32": float(thresholds_f32[c]),
                   "levels": [float(v) for v in levels[c]],
                   "table": {k: float(v) for k, v in zip(names, rates)},
                   "time_under": {f"{TASK_TIME_UNDER_PREFIX[name]}_{float(lv):.6g}": u / pairs * 100
                                  for lv, u in zip(levels[c], under)},
                   "mean_error": float(o[DEFINES["USV_TEVS_ERR_SUM"]]) / pairs}
    return s


def format_task_summary(s: Dict[str, Any]) -> str:
    """The reference's tables, one line per column, and a warning when the run was not fixed-horizon."""
    lines = [f"[evaluate] envs={s['envs']} horizon={s['horizon']} steps={s['steps_min']}..{s['steps_max']}"]
    for name in s["channels"]:
        g = s[name]
        lines.append(f"  {name}:")
        lines += [f"    {k}: {v:.4f}" for k, v in g["table"].items()]
        lines.append("    percentage of time spent under (" + ", ".join(f"{lv:.6g}" for lv in g["levels"]) + f") "
                     f"{TASK_UNITS[name]}: " + " ".join(f"{k}={v:.4f}" for k, v in g["time_under"].items()))
    m = s["return_raw"]
    lines.append(f"  return_raw: mean={m['mean']:.6g} std={m['std']:.6g} "
                 f"95%CI=[{m['ci95_lo']:.6g}, {m['ci95_hi']:.6g}]")
    if s["resets"] > 0:
        lines.append(f"[evaluate] WARNING: {s['envs_reset']} env(s) were reset inside the horizon ({s['resets']} "
                     "resets): the traces run on across them; set task.env.fixed_horizon_eval=True and "
                     "task.env.maxEpisodeLength >= horizon + 2")
    if s["steps_min"] < s["horizon"]:
        lines.append(f"[evaluate] WARNING: only {s['steps_min']} of {s['horizon']} steps were evaluated")
    return "\n".join(lines)
