"""On-device batched policy evaluation: one record per finished episode of every env (usv_eval_* of
include/usv_hip.h), a reduced summary, and the CSV / JSON report of scripts/evaluate_policy.py."""
from .evaluator import EpisodeEvaluator, rollout
from .report import (CSV_COLUMNS, REASON_NAMES, SUMMARY_METRICS, format_summary, summarize_host, summary_from_device,
                     write_csv, write_summary_json)

__all__ = ["EpisodeEvaluator", "rollout", "CSV_COLUMNS", "REASON_NAMES", "SUMMARY_METRICS", "format_summary",
           "summarize_host", "summary_from_device", "write_csv", "write_summary_json"]
