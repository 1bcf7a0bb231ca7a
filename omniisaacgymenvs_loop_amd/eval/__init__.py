"""On-device batched policy evaluation: one record per finished episode of every env (usv_eval_* of
include/usv_hip.h) for CaptureXY, the fixed-horizon success-rate evaluation of the other kinds (usv_teval_*), a
reduced summary, and the CSV / JSON report of scripts/evaluate_policy.py."""
from .bank_evaluator import BankTraceEvaluator, motion_figures, rollout_bank
from .bank_report import bank_csv_columns, bank_csv_row, format_bank_summary, write_bank_csv
from .evaluator import EpisodeEvaluator, rollout
from .report import (CSV_COLUMNS, REASON_NAMES, SUMMARY_METRICS, TASK_UNITS, format_summary, format_task_summary,
                     summarize_host, summary_from_device, task_column_names, task_csv_columns, write_csv,
                     write_summary_json, write_task_csv)
from .task_evaluator import (CHANNELS, TaskTraceEvaluator, default_levels, default_thresholds, rollout_horizon)

__all__ = ["EpisodeEvaluator", "rollout", "CSV_COLUMNS", "REASON_NAMES", "SUMMARY_METRICS", "format_summary",
           "summarize_host", "summary_from_device", "write_csv", "write_summary_json",
           "TaskTraceEvaluator", "rollout_horizon", "CHANNELS", "TASK_UNITS", "default_levels", "default_thresholds",
           "format_task_summary", "task_column_names", "task_csv_columns", "write_task_csv",
           "BankTraceEvaluator", "rollout_bank", "motion_figures", "bank_csv_columns", "bank_csv_row",
           "format_bank_summary", "write_bank_csv"]
