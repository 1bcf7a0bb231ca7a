"""Generate tests/golden/analysis_golden.npz: the REFERENCE's analysis tool (analyze_play_csv.py at its root) on the
small frames of tests/analysis_restate.py.

Run only where the reference tree exists (make_golden.REF) and pandas is installed:
    python tests/golden/make_analysis_golden.py

layer0_paired_bootstrap_groups, layer0_bootstrap_groups and stratified_effects_groups are IMPORTED and called.  The
module's `np` is replaced by a proxy whose random.default_rng hands out generators that record every integers()
draw, one stream per generator in creation order (the tool seeds one generator per metric, and one per stratified
call).  The fixture holds arrays only: the frames, the tool's output columns and the recorded draws (uint8: every
segment here is shorter than 256)."""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_golden import REF  # noqa: E402

from tests import analysis_restate as AR  # noqa: E402

N_BOOT_PAIRED, N_BOOT_UNPAIRED, N_BOOT_STRAT, N_BINS, MIN_PER_BIN, SEED = 32, 16, 16, 4, 5, 0
GROUPS = dict(group_col="group", treat="treat", control="control")


class _Recorder:
    def __init__(self, gen, log):
        self.gen, self.log = gen, log

    def integers(self, *a, **k):
        out = self.gen.integers(*a, **k)
        self.log.append(np.asarray(out).copy())
        return out


class _Random:
    def __init__(self, streams):
        self.streams = streams

    def default_rng(self, seed=None):
        self.streams.append([])
        return _Recorder(np.random.default_rng(seed), self.streams[-1])


class _NumpyProxy:
    def __init__(self, streams):
        self.random = _Random(streams)

    def __getattr__(self, name):
        return getattr(np, name)


def load_reference():
    spec = importlib.util.spec_from_file_location("analyze_play_csv", os.path.join(REF, "analyze_play_csv.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["analyze_play_csv"] = mod
    spec.loader.exec_module(mod)
    return mod


def to_df(pd, frame):
    d = {c: v for c, v in frame.items() if c not in ("group", "scene_idx", "rollout")}
    d["group"] = np.where(frame["group"] == AR.TREAT, "treat", "control")
    d["scene_idx"] = frame["scene_idx"].astype(np.int64)
    return pd.DataFrame(d)


def recorded(A, fn, *args, **kw):
    streams = []
    A.np = _NumpyProxy(streams)
    try:
        out = fn(*args, **kw)
    finally:
        A.np = np
    return out, [np.concatenate(s).astype(np.int64) if s else np.zeros(0, np.int64) for s in streams]


def pack(streams):
    flat = np.concatenate(streams) if streams else np.zeros(0, np.int64)
    assert flat.size == 0 or (flat.min() >= 0 and flat.max() < 256)
    return flat.astype(np.uint8), np.cumsum([0] + [len(s) for s in streams]).astype(np.int64)


def main():
    import pandas as pd
    A = load_reference()
    out = {}
    for tag, (frame, S, R) in (("a", AR.frame_a()), ("b", AR.frame_b())):
        df = to_df(pd, frame)
        for c, v in frame.items():
            out[f"{tag}_frame_{c}"] = v
        out[f"{tag}_SR"] = np.asarray([S, R], np.int64)
        res, streams = recorded(A, A.layer0_paired_bootstrap_groups, df, pair_col="scene_idx", n_boot=N_BOOT_PAIRED,
                                seed=SEED, **GROUPS)
        assert list(res["metric"]) == list(AR.METRIC_NAMES) and len(streams) == len(AR.METRICS)
        out[f"{tag}_pair_n"] = res["n_pairs"].to_numpy(np.int64)
        for k, c in (("diff", "diff_treat_minus_control"), ("lo", "ci95_lo"), ("hi", "ci95_hi")):
            out[f"{tag}_pair_{k}"] = res[c].to_numpy(np.float64)
        out[f"{tag}_pair_draws"], out[f"{tag}_pair_draws_off"] = pack(streams)
    frame, S, R = AR.frame_a()
    df = to_df(pd, frame)
    res, streams = recorded(A, A.layer0_bootstrap_groups, df, n_boot=N_BOOT_UNPAIRED, seed=SEED, **GROUPS)
    assert len(streams) == len(res)
    keep = [i for i, m in enumerate(res["metric"]) if m in AR.METRIC_NAMES]
    assert [res["metric"][i] for i in keep] == list(AR.METRIC_NAMES)
    res = res.iloc[keep]
    out["a_unp_nt"], out["a_unp_nc"] = res["n_treat"].to_numpy(np.int64), res["n_control"].to_numpy(np.int64)
    for k, c in (("diff", "diff_treat_minus_control"), ("lo", "ci95_lo"), ("hi", "ci95_hi")):
        out[f"a_unp_{k}"] = res[c].to_numpy(np.float64)
    out["a_unp_draws"], out["a_unp_draws_off"] = pack([streams[i] for i in keep])
    res, streams = recorded(A, A.stratified_effects_groups, df, strat_cols=list(AR.STRATA_A), n_bins=N_BINS,
                            min_per_bin=MIN_PER_BIN, n_boot=N_BOOT_STRAT, seed=SEED, **GROUPS)
    assert len(streams) == 1 and list(res.columns) == list(AR.STRAT_COLUMNS)
    out["a_strat_col"] = np.asarray([AR.STRATA_A.index(c) for c in res["strat_col"]], np.int64)
    for c in AR.STRAT_COLUMNS[4:]:
        out[f"a_strat_{c}"] = res[c].to_numpy(np.int64 if c in ("bin", "n", "n_treat", "n_control") else np.float64)
    out["a_strat_draws"], _ = pack(streams)
    out["settings"] = np.asarray([N_BOOT_PAIRED, N_BOOT_UNPAIRED, N_BOOT_STRAT, N_BINS, MIN_PER_BIN, SEED], np.int64)
    path = os.path.join(HERE, "analysis_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays; stratified rows: {len(res)}, "
          f"columns {sorted(set(res['strat_col']))}")


if __name__ == "__main__":
    main()
