"""EpisodeEvaluator: the device buffers of the batched evaluation and its four kernels (usv_eval_begin / _mark /
_step / _summary, include/usv_hip.h), hooked into USVVirtual.env_step(evaluator=...).

Nothing here synchronises with the host while stepping: the records stay on the device until episodes() or
summary() copies them back."""
from __future__ import annotations

from typing import Any, Callable, Dict, Optional, Tuple

import numpy as np
import torch

from .. import _capi
from .._abi import DEFINES, UsvEval
from .report import summary_from_device, table_to_episodes

EV_ROWS, EVA_ROWS, EVS_N = DEFINES["USV_EV_ROWS"], DEFINES["USV_EVA_ROWS"], DEFINES["USV_EVS_N"]
# rollout(): steps between two completion checks (one 4-byte read-back each).  The host runs ahead of the device
# by up to this many steps, so the device never idles on the check, and a finished evaluation overruns by at
# most CHECK_EVERY - 1 steps: under 8 % of one 200-step episode, for a sync every 16th step.
CHECK_EVERY = 16


class EpisodeEvaluator:
    """Per-episode metrics of every env of a CaptureXY `task`, `episodes_per_env` records kept per env (further
    episodes are counted as dropped).  action_scale: the policy's action bound (the reference's clipActions)
    for the saturation rate.  Policy-agnostic: it sees only the actions the env steps consume."""

    def __init__(self, task, episodes_per_env: int = 1, action_scale: float = 1.0):
        self.task = task
        self.n = int(task.num_envs)
        self.max_episodes = int(episodes_per_env)
        if self.max_episodes < 1:
            raise ValueError(f"episodes_per_env must be >= 1, got {episodes_per_env}")
        dev = task.device
        f64 = dict(device=dev, dtype=torch.float64)
        cols = self.max_episodes * self.n
        self.acc = torch.zeros((EVA_ROWS, self.n), **f64)
        self.table = torch.zeros((EV_ROWS, cols), **f64)
        self.ep_count = torch.zeros(self.n, device=dev, dtype=torch.int32)
        self._summary = torch.zeros(EVS_N, **f64)
        # simulated seconds per env_step, from the config as the reference takes it (sim.dt x controlFrequencyInv,
        # play_loopz.py:911-920): the step kernel integrates cfg.substeps = controlFrequencyInv substeps of cfg.dt
        tc = task._task_cfg
        self.control_dt = float(tc["sim"]["dt"]) * float(max(int(tc["env"].get("controlFrequencyInv", 10)), 1))
        assert int(task.cfg.substeps) == max(int(tc["env"].get("controlFrequencyInv", 10)), 1)
        assert abs(self.control_dt - float(task.cfg.dt) * int(task.cfg.substeps)) <= 1e-6 * self.control_dt
        self.action_scale = float(action_scale)
        ev = UsvEval()
        ev.acc, ev.episodes, ev.ep_count = _capi.ptr(self.acc), _capi.ptr(self.table), _capi.ptr(self.ep_count)
        ev.max_episodes, ev.action_scale, ev.control_dt = self.max_episodes, self.action_scale, self.control_dt
        self._ev = ev
        self._call("usv_eval_begin")   # also the argument check: a task kind without obstacles is refused here

    def _call(self, name: str, *args) -> None:
        t = self.task
        _capi.call(name, _capi.byref(t.cfg), _capi.byref(t._bufs), _capi.byref(self._ev), *args, _capi.stream_ptr())

    def begin(self) -> None:
        """Forget every record and put every env into reset (as task.reset()): the next env_step starts one
        episode per env."""
        self._call("usv_eval_begin")
        self.task.reset()

    def mark(self) -> None:
        """Between the reset kernels and the env step: the envs just reset start an episode."""
        self._call("usv_eval_mark")

    def step(self, actions: torch.Tensor) -> None:
        """After the env step that consumed `actions` (float32 [n][2], contiguous)."""
        self._call("usv_eval_step", _capi.ptr(actions))

    def min_finished(self) -> int:
        """Finished episodes of the env that has the fewest (one small read-back: a host sync)."""
        return int(self.ep_count.min().item())

    def episodes(self) -> Dict[str, np.ndarray]:
        """The kept records as numpy arrays, one entry per finished episode (episode-major, then env)."""
        return table_to_episodes(self.table.cpu().numpy(), self.ep_count.cpu().numpy(), self.max_episodes)

    def summary_raw(self) -> torch.Tensor:
        """usv_eval_summary's [USV_EVS_N] doubles (device tensor, rewritten by the next call)."""
        self._call("usv_eval_summary", _capi.ptr(self._summary))
        return self._summary

    def summary(self) -> Dict[str, Any]:
        return summary_from_device(self.summary_raw().cpu().numpy())


def rollout(task, policy: Callable[[torch.Tensor], torch.Tensor], evaluator: EpisodeEvaluator,
            max_steps: Optional[int] = None, check_every: int = CHECK_EVERY) -> Tuple[int, bool]:
    """Step `task` with actions = policy(obs) until every env has evaluator.max_episodes finished episodes or
    max_steps steps were taken; returns (steps taken, complete).  The observations start from one zero-action
    step (VecEnvRLGames.reset); begin() then resets every env again, so as in training the first action of an
    episode is computed from the last observation before its reset.  max_steps defaults to
    episodes_per_env x maxEpisodeLength + check_every."""
    task.reset()
    obs, _, _ = task.env_step(torch.zeros((task.num_envs, task.num_actions), device=task.device))
    evaluator.begin()
    if max_steps is None:
        max_steps = evaluator.max_episodes * int(task._max_episode_length) + check_every
    steps, complete = 0, False
    while steps < max_steps and not complete:
        obs, _, _ = task.env_step(policy(obs), evaluator=evaluator)
        steps += 1
        if steps % check_every == 0 or steps == max_steps:
            complete = evaluator.min_finished() >= evaluator.max_episodes
    return steps, complete
