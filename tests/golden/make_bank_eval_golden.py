"""Generate tests/golden/bank_eval_golden.npz: the per-model numbers of the REFERENCE's
omniisaacgymenvs/scripts/multi_model_eval.py (eval_multi_agents) on synthetic traces of two groups of envs.

Run only where the reference tree exists (make_golden.REF) and pandas is installed:
    python tests/golden/make_bank_eval_golden.py

The traces are the synthetic sets of task_eval_golden.npz ("pose": GoToPose rows, "track": TrackXYOVelocity rows;
T = 24, n = 70) read as two groups of 35 envs, plus motion columns obs[..., 0:3] and actions written here.
 * Success tables per group: the reference's utils/eval_metrics.py build_distance_dataframe and check_stay, loaded
   by file path and CALLED on each group's error traces (make_task_eval_golden.reference_channel).
 * ALV / AAV / AAC per group: eval_multi_agents' inline expressions (:107-113) in the same words, applied to the
   USV's columns (body velocity obs[0], obs[1], yaw rate obs[2]; the reference indexes the floating platform's) on
   the [T][n][obs] float32 array as the tool holds it, and again on its float64 copy.
 * Trace content: values at the +-12 clip, an env whose actions are all zero (group 0), and a NaN step in one env
   of group 1 -- the reference's means of that group are NaN, and so are the device's.
 * Asserted here: the float32 figure is within 32 x 2^-24 x mean|v| of the float64 one (numpy's pairwise sum over
   840 terms plus the rounding of the terms): the tolerance the tests use against the float32 numbers.
The fixture holds arrays only and is written with fixed zip timestamps: a rerun reproduces the file byte for byte."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_task_eval_golden import load_reference, reference_channel, write_npz  # noqa: E402

from tests import bank_restate as B  # noqa: E402
from tests import task_eval_restate as R  # noqa: E402

F = np.float32
T, N, G = B.T, B.N, B.GROUP
ZERO_ACT_ENV, NAN_ENV, NAN_STEP = 3, G + 5, 6


def motion_traces(rng):
    vel = np.clip(rng.normal(0, 1.5, (T, N, 3)), -12.0, 12.0).astype(F)
    vel[2, 0], vel[3, 1], vel[4, G + 1] = (F(12.0), F(-12.0), F(12.0)), (F(-12.0), F(0.0), F(-12.0)), F(12.0)
    vel[NAN_STEP, NAN_ENV] = F(np.nan)
    act = np.clip(rng.uniform(-1.3, 1.3, (T, N, 2)), -1.0, 1.0).astype(F)   # clamp(mu): some at the bounds
    act[:, ZERO_ACT_ENV] = 0.0
    return vel, act


def reference_figures(obs, act):
    """eval_multi_agents :107-113 on ep_data['obs'] [T][n][obs], ep_data['act'] [T][n][2], with the USV's columns
    (and the env axis kept: the reference's [:, 2:3] slices it)."""
    lin_vel_x = obs[:, :, 0:1]
    lin_vel_y = obs[:, :, 1:2]
    lin_vel = np.linalg.norm(np.array([lin_vel_x, lin_vel_y]), axis=0)
    alv = np.mean(lin_vel.mean(axis=1))
    ang_vel_z = np.absolute(obs[:, :, 2:3][:, :, 0])
    aav = np.mean(ang_vel_z.mean(axis=1))
    aac = np.mean(act)
    return np.array([alv, aav, aac]), lin_vel[:, :, 0], ang_vel_z


def main():
    M = load_reference()
    tg = R.load_golden()
    rng = np.random.default_rng(20241021)
    out = {}
    for name in ("pose", "track"):
        kind, obs, rew, reset, thr, levels = R.synthetic(tg, name)
        assert obs.shape[:2] == (T, N)
        vel, act = motion_traces(rng)
        obs[..., 0:3] = vel
        x_all = R.errors(kind, obs)
        rates, tu, f32, f64 = [], [], [], []
        for g in range(N // G):
            sl = slice(g * G, (g + 1) * G)
            res = [reference_channel(M, x_all[c][:, sl], float(thr[c]), levels[c]) for c in range(2)]
            for c in range(2):   # the group's per-env results are the whole set's
                for k in ("first_thr", "first_thr2", "stay"):
                    np.testing.assert_array_equal(res[c][k], tg[f"A_{name}_{k}"][c][sl])
            rates.append(np.stack([r["rates"] for r in res]))
            tu.append(np.stack([r["time_under"] for r in res]))
            with np.errstate(invalid="ignore"):
                a32, lv, av = reference_figures(obs[:, sl], act[:, sl])
                a64, _, _ = reference_figures(obs[:, sl].astype(np.float64), act[:, sl].astype(np.float64))
            assert lv.dtype == F and av.dtype == F and a32.dtype == F and a64.dtype == np.float64
            a32 = a32.astype(np.float64)   # the float32 figures, held exactly
            np.testing.assert_array_equal(lv.view(np.int32), B.speed(obs[:, sl]).view(np.int32))
            mean_abs = np.array([np.nanmean(lv.astype(np.float64)), np.nanmean(av.astype(np.float64)),
                                 np.mean(np.abs(act[:, sl].astype(np.float64)))])
            if g == 0:
                assert np.isfinite(a32).all() and (np.abs(a32 - a64) <= 32 * 2.0 ** -24 * mean_abs).all(), (a32, a64)
            else:
                assert np.isnan(a32[:2]).all() and np.isnan(a64[:2]).all() and np.isfinite(a32[2])
                assert abs(a32[2] - a64[2]) <= 32 * 2.0 ** -24 * mean_abs[2]
            f32.append(a32)
            f64.append(a64)
        out[f"{name}_vel"], out[f"{name}_act"] = vel, act
        out[f"{name}_rates"], out[f"{name}_time_under"] = np.stack(rates), np.stack(tu)
        out[f"{name}_figures_f32"], out[f"{name}_figures_f64"] = np.stack(f32), np.stack(f64)
        assert (act[:, ZERO_ACT_ENV] == 0).all() and (np.abs(vel[np.isfinite(vel)]) <= 12).all()
        print(name, "rates", out[f"{name}_rates"].tolist(), "figures", out[f"{name}_figures_f32"].tolist())
    path = os.path.join(HERE, "bank_eval_golden.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
