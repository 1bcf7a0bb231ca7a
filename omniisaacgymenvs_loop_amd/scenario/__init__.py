"""Scenario tables: device mining (sampling), the table format (table), the teacher filter's selection (filter)
the playlist runner (runner; needs a GPU, imported on first use), the teacher-vs-student comparison (compare; its entry
point is compare.compare) and the analysis of a comparison (analysis: bootstrap intervals and stratified effects on the
device; its entry point is analysis.analyse)."""
from .compare import (TailOverride, base_const_tail, base_const_tail_host, cmp_totals, pairing_info,
                      tail_params, wrong_random_tail_host)
from .filter import CSV_COLUMNS, eval_rows, select_keep
from .sampling import (METRIC_KEYS, SamplingParams, build_candidates, metrics_host, philox_host, preselect,
                       select_from_pre, table_of)
from .table import load_table, make_table, obstacles_hash, save_table, subset, to_scene_arrays, to_scene_rows


def __getattr__(name):
    if name in ("ScenarioRunner", "fold_to_dict"):
        from . import runner
        return getattr(runner, name)
    raise AttributeError(name)


__all__ = ["TailOverride", "base_const_tail", "base_const_tail_host", "cmp_totals", "pairing_info",
           "tail_params", "wrong_random_tail_host", "CSV_COLUMNS", "METRIC_KEYS", "SamplingParams", "ScenarioRunner", "build_candidates", "eval_rows",
           "fold_to_dict", "load_table", "make_table", "metrics_host", "obstacles_hash", "philox_host", "preselect",
           "save_table", "select_from_pre", "select_keep", "subset", "table_of", "to_scene_arrays", "to_scene_rows"]
