"""Numpy restatement of the fixed-horizon success-rate evaluation (usv_teval_* of include/usv_hip.h): the
reference's utils/eval_metrics.py (build_distance_dataframe, check_stay, the time-under shares) as a streaming rule
over the per-step float32 error, in our own words.  tests/test_task_eval_cpu.py holds it against the reference's
own results (tests/golden/task_eval_golden.npz, written by tests/golden/make_task_eval_golden.py); the GPU tests
hold the kernels against it.

Everything is float32 against the float32-rounded level; thr / 2 and thr * 7.5 are formed in double and then
rounded; a NaN compares false.  The running sums are doubles, added in step order."""
from __future__ import annotations

import os

import numpy as np

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GO_TO_POSE, TRACK_XYO, GO_TO_XY, KEEP_XY, TRACK_XY = 1, 2, 3, 4, 5
CHANNELS = {GO_TO_XY: ("position",), KEEP_XY: ("position",), GO_TO_POSE: ("position", "heading"),
            TRACK_XY: ("xy_velocity",), TRACK_XYO: ("xy_velocity", "omega_velocity")}
# table rows (include/usv_hip.h USV_TEV_*) and summary slots (USV_TEVS_*)
FIRST_THR, FIRST_THR2, STAY, UNDER0, ERR_SUM, ERR_LAST, CH_STRIDE = 0, 1, 2, 3, 6, 7, 8
STEPS, RETURN, RESETS, ROWS = 16, 17, 18, 19
S_ENVS, S_CHANNELS, S_STEPS_MIN, S_STEPS_MAX, S_RESETS, S_RESET_ENVS, S_CH, S_CH_STRIDE, S_RETURN, S_N = \
    0, 1, 2, 3, 4, 5, 6, 7, 20, 23
INT_ROWS = (FIRST_THR, FIRST_THR2, STAY, UNDER0, UNDER0 + 1, UNDER0 + 2)
FIXTURE_KIND = {"X": GO_TO_XY, "K": KEEP_XY, "V": TRACK_XY, "P": GO_TO_POSE, "T": TRACK_XYO}


def errors(kind, obs):
    """The error channels [nch][...] (float32) of observation rows obs [..., >= 8]: task column k is column 3 + k."""
    obs = np.asarray(obs, F)
    with np.errstate(invalid="ignore", over="ignore"):
        if kind in (TRACK_XY, TRACK_XYO):
            a, b = obs[..., 3], obs[..., 4]
            ch = [np.sqrt(a * a + b * b)]
            if kind == TRACK_XYO:
                ch.append(np.abs(obs[..., 5]))
        else:
            ch = [obs[..., 5].copy()]
            if kind == GO_TO_POSE:
                ch.append(np.abs(np.arctan2(obs[..., 7], obs[..., 6])))
    return np.stack(ch).astype(F)


def derived_levels(thr):
    """(float32 thr, float32(thr / 2), float32(thr * 7.5)) of a threshold held as float32."""
    t = float(F(thr))
    return F(t), F(t / 2.0), F(t * 7.5)


def default_levels(thr):
    """The time-under levels (2.5 thr, thr, thr / 2) of a float32 threshold, formed in double."""
    t = float(F(thr))
    return np.array([F(2.5 * t), F(t), F(t / 2.0)], F)


def begin_table(n):
    tab = np.zeros((ROWS, n), np.float64)
    for c in range(2):
        tab[CH_STRIDE * c + FIRST_THR] = -1
        tab[CH_STRIDE * c + FIRST_THR2] = -1
        tab[CH_STRIDE * c + STAY] = 1
    return tab


def step_table(tab, kind, obs, rew, reset, thr, levels, horizon):
    """One usv_teval_step on table tab (in place): obs [n][>= 8], rew [n], reset [n]."""
    t = tab[STEPS].copy()
    tab[STEPS] += 1
    live = t < horizon
    x = errors(kind, obs)
    tab[RETURN] = np.where(live, tab[RETURN] + np.asarray(rew, F).astype(np.float64), tab[RETURN])
    tab[RESETS] += live & (np.asarray(reset) != 0)
    for c in range(x.shape[0]):
        xv = x[c]
        th, th2, mg = derived_levels(thr[c])
        r = tab[CH_STRIDE * c:CH_STRIDE * (c + 1)]
        with np.errstate(invalid="ignore"):
            lt_thr, lt_thr2, lt_mg = xv < th, xv < th2, xv < mg
            under = [xv < F(levels[c][l]) for l in range(3)]
        stay = (r[STAY] != 0) & lt_mg
        hit = (r[FIRST_THR] < 0) & lt_thr
        stay = stay | hit
        hit2 = (r[FIRST_THR2] < 0) & lt_thr2
        r[FIRST_THR] = np.where(live & hit, t, r[FIRST_THR])
        r[FIRST_THR2] = np.where(live & hit2, t, r[FIRST_THR2])
        r[STAY] = np.where(live, stay.astype(np.float64), r[STAY])
        for l in range(3):
            r[UNDER0 + l] += live & under[l]
        r[ERR_SUM] = np.where(live, r[ERR_SUM] + xv.astype(np.float64), r[ERR_SUM])
        r[ERR_LAST] = np.where(live, xv.astype(np.float64), r[ERR_LAST])
    return tab


def restate(kind, obs, rew, reset, thr, levels, horizon, steps=None):
    """The table after `steps` (default: all T) steps over obs [T][n][>= 8], rew [T][n], reset [T][n]."""
    T, n = np.asarray(obs).shape[:2]
    tab = begin_table(n)
    for t in range(T if steps is None else steps):
        step_table(tab, kind, obs[t], rew[t], reset[t], thr, levels, horizon)
    return tab


def channel_records(tab, c):
    r = tab[CH_STRIDE * c:CH_STRIDE * (c + 1)]
    return dict(first_thr=r[FIRST_THR].astype(np.int64), first_thr2=r[FIRST_THR2].astype(np.int64),
                stay=r[STAY] != 0, under=r[UNDER0:UNDER0 + 3].astype(np.int64), err_sum=r[ERR_SUM],
                err_last=r[ERR_LAST])


def rates(rec):
    """(success_rate_thr, success_rate_thr2, success_and_stay) as check_stay returns them: two percentages and
    a share."""
    return (float((rec["first_thr"] > -1).mean() * 100), float((rec["first_thr2"] > -1).mean() * 100),
            float(rec["stay"].mean()))


def time_under(rec, steps):
    """The share of all (step, env) pairs under each level (np.mean of the comparison)."""
    return rec["under"].sum(1) / float(steps * rec["under"].shape[1])


def summarize(tab, nch):
    """usv_teval_summary's vector with numpy."""
    out = np.zeros(S_N, np.float64)
    n = tab.shape[1]
    out[S_ENVS], out[S_CHANNELS] = n, nch
    out[S_STEPS_MIN], out[S_STEPS_MAX] = tab[STEPS].min(), tab[STEPS].max()
    out[S_RESETS], out[S_RESET_ENVS] = tab[RESETS].sum(), (tab[RESETS] > 0).sum()
    for c in range(nch):
        r = tab[CH_STRIDE * c:CH_STRIDE * (c + 1)]
        o = out[S_CH + S_CH_STRIDE * c:S_CH + S_CH_STRIDE * (c + 1)]
        o[0], o[1], o[2] = (r[FIRST_THR] > -1).sum(), (r[FIRST_THR2] > -1).sum(), (r[STAY] != 0).sum()
        o[3:6] = r[UNDER0:UNDER0 + 3].sum(1)
        o[6] = r[ERR_SUM].sum()
    ret = tab[RETURN][np.isfinite(tab[RETURN])]
    out[S_RETURN] = ret.size
    out[S_RETURN + 1] = ret.mean() if ret.size else np.nan
    out[S_RETURN + 2] = ret.std() if ret.size else np.nan
    return out


def load_golden():
    return dict(np.load(os.path.join(GOLDEN, "task_eval_golden.npz"), allow_pickle=False))


def synthetic(g, name):
    """Synthetic set `name` ("pose": GoToPose, scalar + heading; "track": TrackXYOVelocity, norm + scalar):
    (kind, obs [T][n][33], rew, reset, thr, levels)."""
    kind = GO_TO_POSE if name == "pose" else TRACK_XYO
    o8 = g[f"A_{name}_obs"]
    obs = np.zeros(o8.shape[:2] + (33,), F)
    obs[..., :o8.shape[2]] = o8
    return kind, obs, g[f"A_{name}_rew"], g[f"A_{name}_reset"], g[f"A_{name}_thr"], g[f"A_{name}_levels"]


def golden_channel(g, prefix, c):
    return dict(first_thr=g[f"{prefix}_first_thr"][c], first_thr2=g[f"{prefix}_first_thr2"][c],
                stay=g[f"{prefix}_stay"][c], under=g[f"{prefix}_under"][c])


def assert_channel(got, want, msg=""):
    for k in ("first_thr", "first_thr2", "stay", "under"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{msg} {k}")
