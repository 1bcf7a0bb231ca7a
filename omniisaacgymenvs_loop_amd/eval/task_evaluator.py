"""TaskTraceEvaluator: fixed-horizon success-rate evaluation of the kinds without obstacles (GoToXY, KeepXY,
GoToPose, TrackXYVelocity, TrackXYOVelocity) on the device (usv_teval_begin / _step / _summary, include/usv_hip.h),
hooked into USVVirtual.env_step(evaluator=...) like EpisodeEvaluator.

The reference's tool (scripts/evaluate_policy.py with utils/eval_metrics.py) copies every step's observation to the
host and lets pandas compute first-time-under-threshold, reached-and-stayed and time-under shares from the stacked
trace.  Each of those is a streaming function of the per-step error: here every env keeps its 19 doubles on the
device and nothing synchronises with the host while stepping."""
from __future__ import annotations

import math
from typing import Any, Callable, Dict, Optional, Sequence

import numpy as np
import torch

from .. import _capi
from .._abi import DEFINES, UsvTEval
from .report import task_records_from_table, task_summary_from_device

TEV_ROWS, TEVS_N = DEFINES["USV_TEV_ROWS"], DEFINES["USV_TEVS_N"]
TEV_CH, TEV_LEVELS = DEFINES["USV_TEV_CH"], DEFINES["USV_TEV_LEVELS"]
# channel names per kind: the group keys of the reference's tables (eval_metrics.py)
CHANNELS = {DEFINES["USV_TASK_GO_TO_XY"]: ("position",), DEFINES["USV_TASK_KEEP_XY"]: ("position",),
            DEFINES["USV_TASK_GO_TO_POSE"]: ("position", "heading"), DEFINES["USV_TASK_TRACK_XY"]: ("xy_velocity",),
            DEFINES["USV_TASK_TRACK_XYO"]: ("xy_velocity", "omega_velocity")}
# the reference functions' default thresholds (floating-platform values): used where the kind has no tolerance
REFERENCE_THRESHOLDS = {"position": 0.02, "heading": 0.087, "xy_velocity": 0.15, "omega_velocity": 0.3}


def default_thresholds(cfg) -> tuple:
    """The task's own tolerances from usv_cfg_t (position_tolerance, tk_tol[0], tk_tol[1]) per channel of its kind;
    the reference function's default where the kind has none (GoToPose's heading, a KeepXY without one).  The
    config holds float32: each is returned as the shortest decimal that rounds to it (0.01, not 0.00999999977...),
    which names the report's columns as the yaml wrote it."""
    def short(v):
        return float(str(np.float32(v)))
    own = {"position": short(cfg.position_tolerance), "heading": 0.0, "xy_velocity": short(cfg.tk_tol[0]),
           "omega_velocity": short(cfg.tk_tol[1])}
    return tuple(own[c] if math.isfinite(own[c]) and own[c] > 0.0 else REFERENCE_THRESHOLDS[c]
                 for c in CHANNELS[int(cfg.task_kind)])


def default_levels(thr: float) -> tuple:
    """(2.5 thr, thr, thr / 2): the reference's 5 / 2 / 1 cm and 5 / 2 / 1 degrees at thr = 2 cm / 2 degrees."""
    return (2.5 * thr, thr, thr / 2.0)


class TaskTraceEvaluator:
    """Streaming success metrics of every env of `task` (any kind but CaptureXY) over `horizon` steps.
    thresholds: one per channel of the kind (default: default_thresholds(task.cfg)); levels: three time-under
    levels per channel (default: default_levels of the threshold).  The device compares in float32: a threshold is
    rounded to float32 first, and thr / 2, thr * 7.5 and the default levels derive from the rounded value.
    Policy-agnostic: it reads only the observation, reward and reset buffers the env step leaves."""

    def __init__(self, task, horizon: int, thresholds: Optional[Sequence[float]] = None,
                 levels: Optional[Sequence[Sequence[float]]] = None):
        self.task = task
        self.n = int(task.num_envs)
        self.horizon = int(horizon)
        kind = int(task.cfg.task_kind)
        if kind not in CHANNELS:
            raise ValueError("TaskTraceEvaluator is for the kinds without obstacles; CaptureXY has EpisodeEvaluator "
                             "(eval.episodes_per_env)")
        self.channels = CHANNELS[kind]
        nch = len(self.channels)
        assert _capi.lib().usv_teval_channels(_capi.byref(task.cfg)) == nch
        given = default_thresholds(task.cfg) if thresholds is None else tuple(float(v) for v in thresholds)
        if len(given) != nch:
            raise ValueError(f"{nch} threshold(s) expected for channels {self.channels}, got {len(given)}")
        self.thresholds_given = given
        self.thresholds = tuple(float(np.float32(v)) for v in given)
        if levels is None:
            lv = [default_levels(t) for t in self.thresholds]
        else:
            lv = [tuple(float(v) for v in row) for row in levels]
            if len(lv) != nch or any(len(row) != TEV_LEVELS for row in lv):
                raise ValueError(f"levels: {nch} row(s) of {TEV_LEVELS} expected")
        self.levels = tuple(tuple(float(np.float32(v)) for v in row) for row in lv)
        dev = task.device
        self.table = torch.zeros((TEV_ROWS, self.n), device=dev, dtype=torch.float64)
        self._summary = torch.zeros(TEVS_N, device=dev, dtype=torch.float64)
        tv = UsvTEval()
        tv.table, tv.horizon = _capi.ptr(self.table), self.horizon
        for c in range(nch):
            tv.thr[c] = self.thresholds[c]
            for l in range(TEV_LEVELS):
                tv.level[c][l] = self.levels[c][l]
        self._tv = tv
        self._call("usv_teval_begin")   # also the argument check (horizon, thresholds, levels)

    def _call(self, name: str, *args) -> None:
        t = self.task
        _capi.call(name, _capi.byref(t.cfg), _capi.byref(t._bufs), _capi.byref(self._tv), *args, _capi.stream_ptr())

    def begin(self) -> None:
        """Forget the records and put every env into reset (as task.reset()): the next env_step spawns every env
        and its observation is trace index 0."""
        self._call("usv_teval_begin")
        self.task.reset()

    def mark(self) -> None:
        """Nothing to snapshot at a spawn (kept so that USVVirtual.env_step(evaluator=...) treats both evaluators
        alike)."""

    def step(self, actions=None) -> None:
        """After the env step; the actions are not part of any metric."""
        self._call("usv_teval_step")

    def records(self) -> Dict[str, np.ndarray]:
        """Per-env numpy arrays: steps, return_raw, resets and, per channel, <channel>_first_thr / _first_thr2 /
        _stay / _under0..2 / _err_mean / _err_last."""
        return task_records_from_table(self.table.cpu().numpy(), self.channels, self.horizon)

    def summary_raw(self) -> torch.Tensor:
        """usv_teval_summary's [USV_TEVS_N] doubles (device tensor, rewritten by the next call)."""
        self._call("usv_teval_summary", _capi.ptr(self._summary))
        return self._summary

    def summary(self) -> Dict[str, Any]:
        return task_summary_from_device(self.summary_raw().cpu().numpy(), self.channels, self.thresholds_given,
                                        self.thresholds, self.levels, self.horizon)


def rollout_horizon(task, policy: Callable[[torch.Tensor], torch.Tensor], evaluator: TaskTraceEvaluator) -> int:
    """One zero-action step for the first observation (VecEnvRLGames.reset), evaluator.begin(), then exactly
    evaluator.horizon steps with actions = policy(obs); no host sync inside the loop.  Returns the step count.
    For the reference's fixed-horizon protocol the task runs with fixed_horizon_eval on and maxEpisodeLength =
    horizon + 2 (scripts/evaluate_policy.py sets both); otherwise the resets inside the horizon are counted and
    reported.  policy is any callable from the observation tensor to an action tensor: a PpoPlayerContinuous's
    get_action, or loopz.LoopzTeacher's lz_play callable as it is."""
    task.reset()
    obs, _, _ = task.env_step(torch.zeros((task.num_envs, task.num_actions), device=task.device))
    evaluator.begin()
    for _ in range(evaluator.horizon):
        obs, _, _ = task.env_step(policy(obs), evaluator=evaluator)
    return evaluator.horizon
