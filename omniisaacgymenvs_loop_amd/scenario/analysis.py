"""The analysis stage of a comparison: is the student's loss real, and where does it lose?  The reference's
analyze_play_csv.py on the evaluator tables that already sit on the device (csrc/usv_analysis.hip):

  paired_bootstrap    layer0_paired_bootstrap_groups (:597-700): per-scenario deltas, resampled over scenarios
  unpaired_bootstrap  the mean and rate rows of layer0_bootstrap_groups (:464-594): each arm resampled on its own
  stratified_effects  stratified_effects_groups (:883-985): quantile bins of a condition, an interval per bin
  analyse             all three on a compare() result, every arm against the baseline (the control)

torch for plumbing (gathers, masks, sorts), the kernels for the resampling and the percentiles; the point estimates
are numpy means of the compacted segments, as the reference forms them.  Nothing loops on the host over rows,
scenarios or replicates (only over metrics, strata and bins).

Every (segment, replicate, draw) has its own Philox word (include/usv_hip.h, USV_ANA_SITE), so an interval does not
depend on which other metrics or bins were asked for; the reference seeds one numpy generator per metric, and one
for all columns and bins of the stratified curves.  `inject` = (inj_idx int32 device tensor, inj_off [J + 1]) hands
usv_ana_bootstrap the indices instead (the tests' route to the reference's own index stream)."""
from __future__ import annotations

import warnings
from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from .._abi import DEFINES

PD_ROWS, MAX_BOOT = DEFINES["USV_ANA_PD_ROWS"], DEFINES["USV_ANA_MAX_BOOT"]
NAN_PROPAGATE, NAN_IGNORE = DEFINES["USV_ANA_NAN_PROPAGATE"], DEFINES["USV_ANA_NAN_IGNORE"]
# (metric, evaluator row, success only) in usv_ana_pair_deltas' row order: the reference's names and order
METRICS = (("success_rate", "SUCCESS", False), ("collision_rate", "COLLISION", False),
           ("out_of_bounds_rate", "OOB", False), ("return_scaled_mean", "RETURN", False),
           ("return_raw_mean", "RETURN", False), ("path_efficiency_mean", "PATH_EFF", False),
           ("path_length_mean", "PATH_LENGTH", False), ("time_to_goal_sec_success_mean", "TIME_TO_GOAL", True),
           ("steps_to_goal_mean_success", "LEN_STEPS", True), ("min_obs_dist_min_success_mean", "MIN_OBS_EP", True))
assert len(METRICS) == PD_ROWS and METRICS[DEFINES["USV_ANA_PD_RET_SCALED"]][0] == "return_scaled_mean"
METRIC_NAMES = tuple(m[0] for m in METRICS)
CI = (0.025, 0.975)
PAIRED_COLUMNS = ["metric", "n_pairs", "diff_treat_minus_control", "ci95_lo", "ci95_hi"]
UNPAIRED_COLUMNS = ["metric", "n_treat", "n_control", "diff_treat_minus_control", "ci95_lo", "ci95_hi"]
STRAT_COLUMNS = ["group_col", "treat", "control", "strat_col", "bin", "bin_lo", "bin_hi", "n", "n_treat", "n_control",
                 "delta_success", "delta_success_ci95_lo", "delta_success_ci95_hi", "delta_return_scaled",
                 "delta_return_scaled_ci95_lo", "delta_return_scaled_ci95_hi"]
Inject = Optional[Tuple[Any, Sequence[int]]]


# ------------------------------------------------------------------ the entry points
def pair_deltas(control, treat, n: int, S: int, R: int, K: int, reward_scale: float):
    """usv_ana_pair_deltas of two ArmTables: a [USV_ANA_PD_ROWS][S] float64 device tensor."""
    import torch
    from .. import _capi
    out = torch.empty((PD_ROWS, int(S)), device=control.table.device, dtype=torch.float64)
    _capi.call("usv_ana_pair_deltas", _capi.byref(control.ev), _capi.byref(treat.ev), int(n), int(S), int(R), int(K),
               float(reward_scale), _capi.ptr(out), _capi.stream_ptr())
    return out


def _i64(a):
    import ctypes
    a = np.ascontiguousarray(np.asarray(a, np.int64))
    return a, a.ctypes.data_as(ctypes.c_void_p)


def bootstrap_means(values, seg_off, n_boot: int, seed: int = 0, inject: Inject = None, idx_out=None):
    """usv_ana_bootstrap: values a float64 device tensor, seg_off [J + 1] on the host -> means [J][n_boot] (device).
    idx_out: an int32 device tensor in inject's layout (its offsets: inject[1], or (None, inj_off))."""
    import torch
    from .. import _capi
    seg, seg_p = _i64(seg_off)
    J = int(seg.shape[0]) - 1
    means = torch.full((max(J, 0), int(n_boot)), float("nan"), device=values.device, dtype=torch.float64)
    if J < 1 or int(seg[-1]) == int(seg[0]):
        return means   # no segment, or every segment empty: NaN
    inj_idx, inj_off = inject if inject is not None else (None, None)
    inj_keep, inj_p = _i64(inj_off) if inj_off is not None else (None, None)
    _capi.call("usv_ana_bootstrap", _capi.ptr(values), seg_p, J, int(n_boot), int(seed) & 0xFFFFFFFFFFFFFFFF,
               _capi.ptr(inj_idx), inj_p, _capi.ptr(idx_out), _capi.ptr(means), _capi.stream_ptr())
    del inj_keep
    return means


def quantiles(x, q: Sequence[float], nan_mode: int):
    """usv_ana_quantiles of the rows of x [J][B] (float64, device): [J][len(q)] (device)."""
    import torch
    from .. import _capi
    J, B = int(x.shape[0]), int(x.shape[1])
    out = torch.full((J, len(q)), float("nan"), device=x.device, dtype=torch.float64)
    if J < 1:
        return out
    qd = torch.tensor(list(q), device=x.device, dtype=torch.float64)
    _capi.call("usv_ana_quantiles", _capi.ptr(x.contiguous()), J, B, _capi.ptr(qd), len(q), int(nan_mode),
               _capi.ptr(out), _capi.stream_ptr())
    return out


def _check_boot(n_boot: int) -> int:
    if not 1 <= int(n_boot) <= MAX_BOOT:
        raise ValueError(f"n_boot must be in 1..{MAX_BOOT}, got {n_boot}")
    return int(n_boot)


def _nanmean(v: np.ndarray) -> float:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return float(np.nanmean(v)) if v.size else float("nan")


# ------------------------------------------------------------------ the paired Layer-0
def paired_bootstrap(control, treat, n: int, S: int, R: int, K: int, reward_scale: float = 1.0, n_boot: int = 2000,
                     seed: int = 0, inject: Inject = None) -> List[Dict[str, Any]]:
    """The rows of layer0_paired_summary.csv (PAIRED_COLUMNS): per metric the finite per-scenario deltas (treat -
    control) are one segment, in scenario order; diff is their mean, the interval the 2.5 % and 97.5 % quantiles of
    n_boot means of resamples over scenarios.  No finite delta: all NaN; one: both ends equal the delta."""
    import torch
    B = _check_boot(n_boot)
    d = pair_deltas(control, treat, n, S, R, K, reward_scale)
    finite = torch.isfinite(d)
    counts = finite.sum(1).cpu().numpy().astype(np.int64)
    values = d[finite]                         # row-major: metric by metric, scenario order within
    seg_off = np.concatenate([[0], np.cumsum(counts)])
    ci = quantiles(bootstrap_means(values, seg_off, B, seed, inject), CI, NAN_PROPAGATE).cpu().numpy()
    host = values.cpu().numpy()
    rows = []
    for m, name in enumerate(METRIC_NAMES):
        v = host[seg_off[m]:seg_off[m + 1]]
        if v.size == 0:
            point = lo = hi = float("nan")
        else:
            point = float(np.mean(v))
            lo, hi = (point, point) if v.size == 1 else (float(ci[m, 0]), float(ci[m, 1]))
        rows.append({"metric": name, "n_pairs": int(v.size), "diff_treat_minus_control": point, "ci95_lo": lo,
                     "ci95_hi": hi})
    return rows


# ------------------------------------------------------------------ the unpaired Layer-0
def playlist_columns(arm, n: int, S: int, R: int, K: int):
    """(present [S R] bool, col [S R] int64) on the device: playlist row p = s R + r is column (p % K) n + p / K of
    the arm's table, present when p % K < min(ep_count[p / K], K) (usv_scn_fold's rule)."""
    import torch
    p = torch.arange(int(S) * int(R), device=arm.table.device, dtype=torch.int64)
    e, k = torch.div(p, int(K), rounding_mode="floor"), p % int(K)
    present = k < torch.clamp(arm.ep_count.to(torch.int64)[e], max=int(K))
    return present, k * int(n) + e


def _metric_rows(arm, col, reward_scale: float):
    """[USV_ANA_PD_ROWS][S R] float64: every metric's value of every playlist row (present or not), and the
    success flags."""
    import torch
    vals = torch.stack([arm.table[DEFINES[f"USV_EV_{row}"]][col] for _, row, _ in METRICS])
    vals[DEFINES["USV_ANA_PD_RET_SCALED"]] = vals[DEFINES["USV_ANA_PD_RET_SCALED"]] * float(reward_scale)
    return vals, arm.table[DEFINES["USV_EV_SUCCESS"]][col] == 1.0


def unpaired_bootstrap(control, treat, n: int, S: int, R: int, K: int, reward_scale: float = 1.0, n_boot: int = 2000,
                       seed: int = 0, inject: Inject = None) -> List[Dict[str, Any]]:
    """The mean and rate rows of layer0_summary.csv (UNPAIRED_COLUMNS): per metric two segments (treat, control:
    segment 2 m and 2 m + 1), the arm's present playlist rows in playlist order (the success-only metrics: its
    successes), resampled independently; the interval is over mean_t[b] - mean_c[b], NaN propagated."""
    import torch
    B = _check_boot(n_boot)
    segs, lens = [], []
    for arm in (treat, control):
        present, col = playlist_columns(arm, n, S, R, K)
        vals, succ = _metric_rows(arm, col, reward_scale)
        masks = torch.stack([present & succ if so else present for _, _, so in METRICS])
        segs.append((vals, masks))
        lens.append(masks.sum(1).cpu().numpy().astype(np.int64))
    parts = [segs[a][0][m][segs[a][1][m]] for m in range(PD_ROWS) for a in (0, 1)]
    values = torch.cat(parts)
    seg_off = np.concatenate([[0], np.cumsum(np.stack(lens, 1).reshape(-1))])
    means = bootstrap_means(values, seg_off, B, seed, inject)
    ci = quantiles(means[0::2] - means[1::2], CI, NAN_PROPAGATE).cpu().numpy()
    host = values.cpu().numpy()
    rows = []
    for m, name in enumerate(METRIC_NAMES):
        vt, vc = host[seg_off[2 * m]:seg_off[2 * m + 1]], host[seg_off[2 * m + 1]:seg_off[2 * m + 2]]
        if vt.size == 0 or vc.size == 0:
            point = lo = hi = float("nan")
        else:
            point, lo, hi = _nanmean(vt) - _nanmean(vc), float(ci[m, 0]), float(ci[m, 1])
        rows.append({"metric": name, "n_treat": int(vt.size), "n_control": int(vc.size),
                     "diff_treat_minus_control": point, "ci95_lo": lo, "ci95_hi": hi})
    return rows


# ------------------------------------------------------------------ the stratified effect curves
def quantile_edges(x, n_bins: int) -> np.ndarray:
    """np.unique(np.nanquantile(x, linspace(0, 1, n_bins + 1))) of a device vector: sorted on the device, numpy's
    "linear" rule on the 2 (n_bins + 1) order statistics it needs."""
    import torch
    xs = torch.sort(x[~torch.isnan(x)]).values
    m = int(xs.shape[0])
    if m == 0:
        return np.zeros(0, np.float64)
    pos = (m - 1) * np.linspace(0.0, 1.0, int(n_bins) + 1)
    lo = np.floor(pos)
    g = pos - lo
    lo_i = lo.astype(np.int64)
    hi_i = np.minimum(lo_i + 1, m - 1)
    ab = xs[torch.as_tensor(np.concatenate([lo_i, hi_i]), device=x.device)].cpu().numpy()
    a, b = ab[:lo_i.shape[0]], ab[lo_i.shape[0]:]
    with np.errstate(invalid="ignore"):
        d = b - a
        edges = np.where(g >= 0.5, b - d * (1.0 - g), a + d * g)   # numpy's _lerp
    return np.unique(edges)


def stratified_effects(control, treat, n: int, S: int, R: int, K: int, reward_scale: float = 1.0, *,
                       strata: Mapping[str, Any], n_bins: int = 5, min_per_bin: int = 5, n_boot: int = 2000,
                       seed: int = 0, inject: Inject = None, labels: Tuple[str, str, str] = ("arm", "treat", "control"),
                       return_bins: bool = False):
    """The rows of stratified_effects.csv (STRAT_COLUMNS).  strata: name -> a value per playlist row [S R] or per
    scenario [S].  The rows present in either arm are pooled (a row present in both counts twice, as in the
    reference's concatenated frame): edges = unique(nanquantile(pooled, linspace(0, 1, n_bins + 1))), a column with
    fewer than 3 edges is left out, bin = digitize(x, edges[1:-1], right=True) (a NaN lands in the last bin); a bin
    with fewer than 2 min_per_bin rows, or fewer than min_per_bin in an arm, is left out.  Per kept bin four
    segments (success of treat and of control, return_scaled of treat and of control), all bins of all columns in
    one usv_ana_bootstrap call; quantiles with NaN ignored.  labels = (group_col, treat, control) as written.
    return_bins: also {name: (edges, bin of every playlist row [S R] on the host)}."""
    import torch
    B = _check_boot(n_boot)
    dev = control.table.device
    arms = []
    for arm in (treat, control):
        present, col = playlist_columns(arm, n, S, R, K)
        arms.append((present, arm.table[DEFINES["USV_EV_SUCCESS"]][col],
                     arm.table[DEFINES["USV_EV_RETURN"]][col] * float(reward_scale)))
    kept, parts, lens, bins_out = [], [], [], {}
    for name, x in strata.items():
        x = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(dev, torch.float64).reshape(-1)
        if int(x.shape[0]) == int(S):
            x = x.repeat_interleave(int(R))
        if int(x.shape[0]) != int(S) * int(R):
            raise ValueError(f"strata[{name!r}] has {int(x.shape[0])} values: expected S = {S} or S R = {S * R}")
        edges = quantile_edges(torch.cat([x[arms[0][0]], x[arms[1][0]]]), n_bins)
        if len(edges) < 3:
            continue
        nb = len(edges) - 1
        bin_idx = torch.bucketize(x, torch.as_tensor(edges[1:-1], device=dev), right=False)
        bin_idx = torch.where(torch.isnan(x), torch.full_like(bin_idx, nb - 1), bin_idx)
        if return_bins:
            bins_out[name] = (edges, bin_idx.cpu().numpy())
        cnt = np.stack([torch.bincount(bin_idx[a[0]], minlength=nb).cpu().numpy() for a in arms])   # [treat, control]
        for b in range(nb):
            nt, nc = int(cnt[0, b]), int(cnt[1, b])
            if nt + nc < 2 * int(min_per_bin) or nt < int(min_per_bin) or nc < int(min_per_bin):
                continue
            mt, mc = arms[0][0] & (bin_idx == b), arms[1][0] & (bin_idx == b)
            parts += [arms[0][1][mt], arms[1][1][mc], arms[0][2][mt], arms[1][2][mc]]
            lens += [nt, nc, nt, nc]
            kept.append((name, b, float(edges[b]), float(edges[b + 1]), nt, nc))
    rows: List[Dict[str, Any]] = []
    if kept:
        values = torch.cat(parts)
        seg_off = np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))])
        means = bootstrap_means(values, seg_off, B, seed, inject)
        ci = quantiles(means[0::2] - means[1::2], CI, NAN_IGNORE).cpu().numpy()   # row 2 q: success, 2 q + 1: return
        host = values.cpu().numpy()
        for q, (name, b, lo, hi, nt, nc) in enumerate(kept):
            s = [host[seg_off[4 * q + i]:seg_off[4 * q + i + 1]] for i in range(4)]
            rows.append({"group_col": labels[0], "treat": labels[1], "control": labels[2], "strat_col": name, "bin": b,
                         "bin_lo": lo, "bin_hi": hi, "n": nt + nc, "n_treat": nt, "n_control": nc,
                         "delta_success": _nanmean(s[0]) - _nanmean(s[1]),
                         "delta_success_ci95_lo": float(ci[2 * q, 0]), "delta_success_ci95_hi": float(ci[2 * q, 1]),
                         "delta_return_scaled": _nanmean(s[2]) - _nanmean(s[3]),
                         "delta_return_scaled_ci95_lo": float(ci[2 * q + 1, 0]),
                         "delta_return_scaled_ci95_hi": float(ci[2 * q + 1, 1])})
    return (rows, bins_out) if return_bins else rows


# ------------------------------------------------------------------ a compare() result
def analyse(result: Mapping[str, Any], reward_scale: float = 1.0, n_boot: int = 2000, seed: int = 0,
            strata: Optional[Mapping[str, Any]] = None, n_bins: int = 5, min_per_bin: int = 5) -> Dict[str, Any]:
    """All three analyses of a scenario.compare.compare() result, every arm against the baseline (the control):
    {arm: {"paired": rows, "unpaired": rows, "stratified": rows}}."""
    base = result["baseline"]
    n, S, R, K = int(result["n"]), int(result["S"]), int(result["R"]), int(result["episodes_per_env"])
    control = result["arms"][base]["table"]
    out: Dict[str, Any] = {}
    for name, arm in result["arms"].items():
        if name == base:
            continue
        treat = arm["table"]
        out[name] = {"paired": paired_bootstrap(control, treat, n, S, R, K, reward_scale, n_boot, seed),
                     "unpaired": unpaired_bootstrap(control, treat, n, S, R, K, reward_scale, n_boot, seed),
                     "stratified": stratified_effects(control, treat, n, S, R, K, reward_scale, strata=strata,
                                                      n_bins=n_bins, min_per_bin=min_per_bin, n_boot=n_boot,
                                                      seed=seed, labels=("arm", name, base)) if strata else []}
    return out
