"""BankTraceEvaluator: the fixed-horizon evaluation of M checkpoints in one rollout of n = M x G envs (envs
[m G, (m + 1) G) under checkpoint m, rl_games.model_bank.ModelBank), with the reference's per-model motion figures
of scripts/multi_model_eval.py (ALV, AAV, AAC) beside the success tables of TaskTraceEvaluator.

Paired (the default): env m G + i receives the random words and the env origin of env i of a G-env run with the
same seed (usv_bank_uniforms), so every model faces the same G scenarios and group m equals a stand-alone run of
model m on G envs bit for bit -- except the RETURN of TrackXYOVelocity, whose reward holds a sum over all envs of the
run (M x G here, as it would be in the reference).

The reference indexes the floating platform's observation columns (and slices the env axis of its [T][n][obs]
array); as for the success tables, the metric definitions are fed the USV's columns:
    ALV  mean over all (step, env) pairs of the float32 norm(obs[0], obs[1])   (body-frame linear velocity)
    AAV  mean of |obs[2]|                                                       (yaw rate)
    AAC  mean of the actions handed to the env, over steps, envs and both components."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import _capi
from .._abi import DEFINES, UsvBank
from ..tasks.usv_config import env_origins
from .report import task_records_from_table, task_summary_from_device
from .task_evaluator import TaskTraceEvaluator

BEV_ROWS, BEVS_N, TEVS_N = DEFINES["USV_BEV_ROWS"], DEFINES["USV_BEVS_N"], DEFINES["USV_TEVS_N"]
NU_STEP, NU_RESET = DEFINES["USV_NU_STEP"], DEFINES["USV_NU_RESET"]


def motion_figures(row: np.ndarray) -> Dict[str, float]:
    """ALV, AAV, AAC from one row of usv_bank_summary's output (NaN without a pair)."""
    pairs = float(row[DEFINES["USV_BEVS_PAIRS"]])
    if pairs <= 0.0:
        return {"ALV": float("nan"), "AAV": float("nan"), "AAC": float("nan")}
    return {"ALV": float(row[DEFINES["USV_BEVS_SPEED_SUM"]]) / pairs,
            "AAV": float(row[DEFINES["USV_BEVS_YAWRATE_SUM"]]) / pairs,
            "AAC": float(row[DEFINES["USV_BEVS_ACT_SUM"]]) / (2.0 * pairs)}


class BankTraceEvaluator:
    """Streaming success metrics and motion sums of `models` groups of `group` envs of `task` over `horizon`
    steps; thresholds / levels as TaskTraceEvaluator's.  The same begin / mark / step(actions) hooks, for
    USVVirtual.env_step(evaluator=...)."""

    def __init__(self, task, horizon: int, models: int, group: int, thresholds: Optional[Sequence[float]] = None,
                 levels: Optional[Sequence[Sequence[float]]] = None, paired: bool = True):
        self.models, self.group, self.paired = int(models), int(group), bool(paired)
        if self.models < 1 or self.group < 1 or self.models * self.group != int(task.num_envs):
            raise ValueError(f"{self.models} groups of {self.group} envs expected, the task has {task.num_envs} envs")
        self.inner = TaskTraceEvaluator(task, horizon, thresholds=thresholds, levels=levels)
        self.task, self.n, self.horizon, self.channels = task, self.inner.n, self.inner.horizon, self.inner.channels
        dev = task.device
        self.motion = torch.zeros((BEV_ROWS, self.n), device=dev, dtype=torch.float64)
        self._summary = torch.zeros((self.models, BEVS_N), device=dev, dtype=torch.float64)
        bk = UsvBank()
        bk.motion, bk.models, bk.group, bk.horizon = _capi.ptr(self.motion), self.models, self.group, self.horizon
        self._bk = bk
        self._call("usv_bank_begin", _capi.byref(bk))   # also the argument check
        self.u_step = self.u_reset = None
        if self.paired:
            self.u_step = torch.zeros((self.n, NU_STEP), device=dev, dtype=torch.float32)
            self.u_reset = torch.zeros((self.n, NU_RESET), device=dev, dtype=torch.float32)
            task.set_env_origins(torch.from_numpy(np.tile(env_origins(self.group), (1, self.models))))

    @property
    def table(self) -> torch.Tensor:
        return self.inner.table

    def _call(self, name: str, *args) -> None:
        t = self.task
        _capi.call(name, _capi.byref(t.cfg), _capi.byref(t._bufs), *args, _capi.stream_ptr())

    def draws(self) -> Dict[str, torch.Tensor]:
        """The u_step / u_reset keywords of the task's next env_step: the paired run's words for the step index it
        is about to use ({} when unpaired: the in-kernel draws, keyed by the env index of the whole run)."""
        if not self.paired:
            return {}
        t = self.task
        _capi.call("usv_bank_uniforms", _capi.byref(t.cfg), _capi.byref(t._bufs), self.group, t.seed, t._step_index,
                   _capi.ptr(self.u_step), _capi.ptr(self.u_reset), _capi.stream_ptr())
        return {"u_step": self.u_step, "u_reset": self.u_reset}

    def begin(self) -> None:
        self.inner.begin()
        self._call("usv_bank_begin", _capi.byref(self._bk))

    def mark(self) -> None:
        self.inner.mark()

    def step(self, actions) -> None:
        self.inner.step(actions)
        self._call("usv_bank_step", _capi.byref(self._bk), _capi.ptr(actions))

    def records(self) -> Dict[str, np.ndarray]:
        """TaskTraceEvaluator.records() plus model (the group index of the env) and the per-env speed_mean,
        yawrate_mean, action_mean."""
        rec = task_records_from_table(self.table.cpu().numpy(), self.channels, self.horizon)
        mo = self.motion.cpu().numpy()
        seen = np.maximum(np.minimum(mo[DEFINES["USV_BEV_STEPS"]], self.horizon), 1.0)
        rec["model"] = (np.arange(self.n) // self.group).astype(np.int32)
        rec["speed_mean"] = mo[DEFINES["USV_BEV_SPEED_SUM"]] / seen
        rec["yawrate_mean"] = mo[DEFINES["USV_BEV_YAWRATE_SUM"]] / seen
        rec["action_mean"] = mo[DEFINES["USV_BEV_ACT_SUM"]] / (2.0 * seen)
        return rec

    def summary_raw(self) -> torch.Tensor:
        """usv_bank_summary's [models][USV_BEVS_N] doubles (device tensor, rewritten by the next call)."""
        self._call("usv_bank_summary", _capi.byref(self.inner._tv), _capi.byref(self._bk), _capi.ptr(self._summary))
        return self._summary

    def summaries(self) -> List[Dict[str, Any]]:
        """One dict per model: task_summary_from_device of its row, plus ALV, AAV, AAC."""
        out = []
        ev = self.inner
        for row in self.summary_raw().cpu().numpy():
            s = task_summary_from_device(row[:TEVS_N], self.channels, ev.thresholds_given, ev.thresholds, ev.levels,
                                         self.horizon)
            s.update(motion_figures(row))
            out.append(s)
        return out


def rollout_bank(task, bank, evaluator: BankTraceEvaluator) -> int:
    """rollout_horizon's protocol with a ModelBank: one zero-action step for the first observation,
    evaluator.begin(), then exactly evaluator.horizon steps with actions = bank.get_action(obs); no host sync inside
    the loop.  A paired evaluator's words go into every env_step (the zero-action one included)."""
    task.reset()
    obs, _, _ = task.env_step(torch.zeros((task.num_envs, task.num_actions), device=task.device), **evaluator.draws())
    evaluator.begin()
    for _ in range(evaluator.horizon):
        obs, _, _ = task.env_step(bank.get_action(obs), evaluator=evaluator, **evaluator.draws())
    return evaluator.horizon
