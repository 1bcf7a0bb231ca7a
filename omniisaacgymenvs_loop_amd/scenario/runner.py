"""ScenarioRunner: play every (scenario, rollout) pair of a table as one env's episode and fold the evaluator's
records per scenario on the device (usv_scn_fold, csrc/usv_scenario.hip).

Playlist: row p = s R + r is scenario s, rollout r (S R rows; rows past S R repeat row p mod S R, they only keep
idle envs busy and are not folded).  Env e plays rows e K .. e K + K - 1 with K = ceil(S R / n), so the record of
row p is column (p % K) n + p / K of the evaluator's table.

Pairing: two runs with the same task seed, n, table and R give every (env, episode 0) the same scene and the same
reset draws, whatever the policy (the draws are keyed by seed, env and step, and episode 0 of every env starts at
the same step).  Later episodes of an env (K > 1) start when the policy's earlier episodes end: they share the
scene only.

Scenes are applied by the reset kernel's scene-replay path (float32 yaw through its sincos); every rollout of a
scenario is its own env with its own randomisation draws, where the reference re-runs env 0."""
from __future__ import annotations

from typing import Callable, Dict, Optional

import numpy as np
import torch

from .. import _capi
from .._abi import DEFINES
from ..tasks.usv_config import COLLISION_THRESHOLD
from ..eval.evaluator import CHECK_EVERY, EpisodeEvaluator
from .table import check_table, to_scene_rows

SCF_ROWS = DEFINES["USV_SCF_ROWS"]
FOLD_KEYS = {"rollouts_present": "USV_SCF_PRESENT", "success_rate": "USV_SCF_SUCCESS_RATE",
             "collision_rate": "USV_SCF_COLL_RATE", "out_of_bounds_rate": "USV_SCF_OOB_RATE",
             "collision_any": "USV_SCF_COLL_ANY", "out_of_bounds_any": "USV_SCF_OOB_ANY", "reason": "USV_SCF_REASON",
             "steps": "USV_SCF_STEPS", "ep_return_raw": "USV_SCF_RETURN", "final_dist_to_goal": "USV_SCF_FINAL_DIST",
             "min_obs_dist_min": "USV_SCF_MIN_OBS", "min_margin_min": "USV_SCF_MIN_MARGIN",
             "verdict": "USV_SCF_VERDICT", "difficulty": "USV_SCF_DIFFICULTY"}
INT_KEYS = ("rollouts_present", "collision_any", "out_of_bounds_any", "reason", "steps", "verdict")


def fold_to_dict(out: np.ndarray) -> Dict[str, np.ndarray]:
    """usv_scn_fold's [USV_SCF_ROWS][S] doubles by name (counts, flags, codes and steps as int64)."""
    d = {k: np.array(out[DEFINES[row]]) for k, row in FOLD_KEYS.items()}
    for k in INT_KEYS:
        d[k] = d[k].astype(np.int64)
    return d


class ScenarioRunner:
    """Plays `table` on a CaptureXY `task`, `rollouts` episodes per scenario; run(policy) returns the per-scenario
    arrays of fold_to_dict.  policy: any callable obs -> actions (a LoopzTeacher, a SysIDStudent, an rl_games
    player's clamp(mu))."""

    def __init__(self, task, table, rollouts: int = 1, action_scale: float = 1.0, easy_steps_max: int = 80,
                 easy_margin_min: float = 0.8):
        self.task = task
        self.n = int(task.num_envs)
        self.S = check_table(table)
        self.R = int(rollouts)
        if self.R < 1:
            raise ValueError(f"rollouts must be >= 1, got {rollouts}")
        pairs = self.S * self.R
        self.K = (pairs + self.n - 1) // self.n
        self.easy_steps_max, self.easy_margin_min = int(easy_steps_max), float(easy_margin_min)
        self.max_steps_episode = int(task._max_episode_length)
        # the Python float the reference subtracts, not the float32 the kernels compare with
        self.collision_threshold = float(COLLISION_THRESHOLD)
        dev = task.device
        scenes = torch.from_numpy(to_scene_rows(table)).to(dev)
        p = torch.arange(self.K * self.n, device=dev)
        self.rows = scenes[((p % pairs) // self.R)].contiguous()   # [K n][USV_SCENE_STRIDE]
        self.first_row = (torch.arange(self.n, device=dev, dtype=torch.int32) * self.K).contiguous()
        self.evaluator = EpisodeEvaluator(task, episodes_per_env=self.K, action_scale=action_scale)
        self._out = torch.zeros((SCF_ROWS, self.S), device=dev, dtype=torch.float64)

    def fold_raw(self) -> torch.Tensor:
        """usv_scn_fold of the evaluator's table as it stands: [USV_SCF_ROWS][S] doubles (device, rewritten by
        the next call)."""
        _capi.call("usv_scn_fold", _capi.byref(self.evaluator._ev), self.n, self.S, self.R, self.K,
                   self.collision_threshold, self.easy_steps_max, self.easy_margin_min, self.max_steps_episode,
                   _capi.ptr(self._out), _capi.stream_ptr())
        return self._out

    def run(self, policy: Callable[[torch.Tensor], torch.Tensor], max_steps: Optional[int] = None,
            allow_incomplete: bool = False, check_every: int = CHECK_EVERY) -> Dict[str, np.ndarray]:
        """eval.rollout with the playlist installed: after evaluator.begin() and before the first evaluated step
        every env's next scene is set to its first playlist row (the warm-up reset and zero-action step consume
        scene indices before that)."""
        task, ev = self.task, self.evaluator
        task.set_scene_table(self.rows, self.first_row)
        task.reset()
        obs, _, _ = task.env_step(torch.zeros((task.num_envs, task.num_actions), device=task.device))
        ev.begin()
        task._touch()
        task.scene_next.copy_(self.first_row)
        if max_steps is None:
            max_steps = self.K * self.max_steps_episode + check_every
        steps, complete = 0, False
        while steps < max_steps and not complete:
            obs, _, _ = task.env_step(policy(obs), evaluator=ev)
            steps += 1
            if steps % check_every == 0 or steps == max_steps:
                complete = ev.min_finished() >= self.K
        self.steps_taken = steps
        out = fold_to_dict(self.fold_raw().cpu().numpy())
        missing = int((out["rollouts_present"] < self.R).sum())
        if missing and not allow_incomplete:
            raise RuntimeError(f"{missing} of {self.S} scenarios have a rollout without a record after {steps} steps "
                               "(raise max_steps, or pass allow_incomplete=True)")
        return out
