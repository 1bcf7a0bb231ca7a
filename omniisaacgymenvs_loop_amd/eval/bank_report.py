"""The report of scripts/multi_model_eval.py: one CSV row per model (the reference's all_success_rate_df of
scripts/multi_model_eval.py:114-123 with `model` inserted first), built from BankTraceEvaluator.summaries()."""
from __future__ import annotations

import csv
from typing import Any, Dict, List, Sequence

from .report import TASK_TIME_UNDER_PREFIX, _fmt, task_column_names

MOTION_COLUMNS = ("ALV", "AAV", "AAC")
TAIL_COLUMNS = ("return_mean", "return_std", "resets")


def bank_csv_columns(channels: Sequence[str], thresholds: Sequence[float], levels) -> tuple:
    """model, then per channel the reference table's three columns and its three time-under columns (report.py's
    names), then ALV, AAV, AAC, the return's mean and standard deviation and the resets inside the horizon."""
    cols = ["model"]
    for c, name in enumerate(channels):
        cols += list(task_column_names(name, float(thresholds[c])))
        cols += [f"{TASK_TIME_UNDER_PREFIX[name]}_{float(lv):.6g}" for lv in levels[c]]
    return tuple(cols) + MOTION_COLUMNS + TAIL_COLUMNS


def bank_csv_row(model: str, s: Dict[str, Any]) -> Dict[str, Any]:
    """The row of one model from its summary (task_summary_from_device's dict plus ALV, AAV, AAC)."""
    row: Dict[str, Any] = {"model": model}
    for name in s["channels"]:
        row.update(s[name]["table"])
        row.update(s[name]["time_under"])
    row.update({k: s[k] for k in MOTION_COLUMNS})
    row.update(return_mean=s["return_raw"]["mean"], return_std=s["return_raw"]["std"], resets=s["resets"])
    return row


def write_bank_csv(path: str, names: Sequence[str], summaries: List[Dict[str, Any]]) -> int:
    """One row per model in the given order; returns the row count."""
    s0 = summaries[0]
    cols = bank_csv_columns(s0["channels"], [s0[c]["threshold"] for c in s0["channels"]],
                            [s0[c]["levels"] for c in s0["channels"]])
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(cols)
        for name, s in zip(names, summaries):
            row = bank_csv_row(name, s)
            w.writerow([row[k] if k == "model" else _fmt(row[k]) for k in cols])
    return len(summaries)


def format_bank_summary(names: Sequence[str], summaries: List[Dict[str, Any]]) -> str:
    lines = []
    for name, s in zip(names, summaries):
        rates = " ".join(f"{k}={v:.4f}" for c in s["channels"] for k, v in s[c]["table"].items())
        lines.append(f"[bank] {name}: {rates} ALV={s['ALV']:.6g} AAV={s['AAV']:.6g} AAC={s['AAC']:.6g} "
                     f"return={s['return_raw']['mean']:.6g} resets={s['resets']}")
    return "\n".join(lines)
