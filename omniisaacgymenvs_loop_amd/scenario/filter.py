"""The teacher filter's selection (scripts/teacher_filter_scenario_table.py, _select_keep_indices :492-568) and
the rows of teacher_eval.csv (:738-766) from usv_scn_fold's per-scenario arrays."""
from __future__ import annotations

from typing import Any, Dict, List, Tuple

import numpy as np

from .._abi import DEFINES

REASON_NAMES = {DEFINES["USV_EV_REASON_COLLISION"]: "collision", DEFINES["USV_EV_REASON_OOB"]: "out_of_bounds",
                DEFINES["USV_EV_REASON_GOAL"]: "goal_tolerance", DEFINES["USV_EV_REASON_OTHER"]: "other",
                DEFINES["USV_EV_REASON_MIXED"]: "mixed"}
VERDICT_NAMES = {DEFINES["USV_SCV_KEEP"]: "keep", DEFINES["USV_SCV_HARD_REJECT"]: "hard_reject",
                 DEFINES["USV_SCV_EASY_REJECT"]: "easy_reject", DEFINES["USV_SCV_INCOMPLETE"]: "incomplete"}
CSV_COLUMNS = ["scenario_id", "source_preselect_id", "obstacles_hash", "density_score", "d_spawn", "d_goal", "d_corr",
               "d_oo", "done_reason", "success_rate", "collision_rate", "out_of_bounds_rate", "collision_any",
               "out_of_bounds_any", "steps", "ep_return_raw", "final_dist_to_goal", "min_obs_dist_min",
               "min_margin_min", "max_steps"]


def difficulty(steps: float, margin: float, max_steps: int) -> float:
    """:546-552: normalised steps + 0.3 x normalised tightness (a smaller margin is harder)."""
    steps_n = float(steps) / max(1.0, float(max_steps))
    tight_n = float(np.clip((0.5 - float(margin)) / 0.5, -2.0, 2.0))
    return float(steps_n + 0.3 * tight_n)


def select_keep(rows: List[Dict[str, Any]], n_keep: int, n_final: int, easy_steps_max: int,
                easy_margin_min: float) -> Tuple[np.ndarray, np.ndarray, Dict[str, Any]]:
    """(keep_idx, final_idx, summary), indices in the input table's row space.  The ranking is np.argsort(-scores)
    on the host in table order, as the reference's (not a stable sort: equal difficulties may swap)."""
    n = len(rows)
    if n == 0:
        return np.zeros((0,), np.int64), np.zeros((0,), np.int64), {"n": 0}
    hard_keep, hard_reject, easy_reject = [], [], []
    for r in rows:
        idx = int(r["source_preselect_id"]) if "source_preselect_id" in r else int(r["scenario_id"])
        success_rate = float(r.get("success_rate", float(r.get("success", 0))))
        if int(r.get("collision_any", 0)) > 0 or int(r.get("out_of_bounds_any", 0)) > 0 or not (success_rate > 0.0):
            hard_reject.append(idx)
        elif (int(r.get("steps", 10 ** 9)) <= int(easy_steps_max)
              and float(r.get("min_margin_min", float("inf"))) >= float(easy_margin_min)):
            easy_reject.append(idx)
        else:
            hard_keep.append(idx)
    keep = np.array(hard_keep, dtype=np.int64)
    if keep.size == 0:
        keep_idx = final_idx = keep
    else:
        by_idx = {int(r.get("source_preselect_id", r.get("scenario_id"))): r for r in rows}
        max_steps = max(int(r.get("max_steps", 1)) for r in rows)
        scores = np.array([difficulty(by_idx[int(i)].get("steps", 0.0), by_idx[int(i)].get("min_margin_min", 0.0),
                                      max_steps) for i in keep], dtype=np.float64)
        ranked = keep[np.argsort(-scores)]
        keep_idx = ranked[:min(int(n_keep), ranked.size)]
        final_idx = keep_idx[:min(int(n_final), keep_idx.size)]
    summary = {"n_total": int(n), "n_hard_reject": len(hard_reject), "n_easy_reject": len(easy_reject),
               "n_keep": int(keep_idx.size), "n_final": int(final_idx.size)}
    return keep_idx, final_idx, summary


def eval_rows(table: Dict[str, Any], fold: Dict[str, np.ndarray], max_steps: int) -> List[Dict[str, Any]]:
    """One teacher_eval.csv row per scenario (:738-766, the reference's columns in its order) from a table and
    ScenarioRunner.run's per-scenario arrays."""
    out = []
    for si in range(int(np.asarray(table["scenario_id"]).shape[0])):
        row = {"scenario_id": int(table["scenario_id"][si]), "source_preselect_id": int(si),
               "obstacles_hash": str(table["obstacles_hash"][si])}
        for k in ("density_score", "d_spawn", "d_goal", "d_corr", "d_oo"):
            row[k] = float(table[k][si])
        row["done_reason"] = REASON_NAMES[int(fold["reason"][si])]
        for k in ("success_rate", "collision_rate", "out_of_bounds_rate"):
            row[k] = float(fold[k][si])
        for k in ("collision_any", "out_of_bounds_any", "steps"):
            row[k] = int(fold[k][si])
        for k in ("ep_return_raw", "final_dist_to_goal", "min_obs_dist_min", "min_margin_min"):
            row[k] = float(fold[k][si])
        row["max_steps"] = int(max_steps)
        if "source_candidate_id" in table:
            row["source_candidate_id"] = int(table["source_candidate_id"][si])
        out.append(row)
    return out
