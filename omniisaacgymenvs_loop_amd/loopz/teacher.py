"""LoopzTeacher: a loopz actor played deterministically on the device (lz_play, csrc/loopz.hip):
actions = tanh(architecture(obs)) * action_scale, the reference's teacher rollout
(scripts/teacher_filter_scenario_table.py:446-450).  No draw, no rollout storage, no critic."""
from __future__ import annotations

import torch

from .. import _capi
from .._abi import LzCfg
from .module import Actor, SquashedGaussianDiagonalCovariance


class LoopzTeacher:
    """A callable obs [n][obs_dim] (device) -> actions [n][2] (device, rewritten by the next call), so
    eval.rollout and scenario.ScenarioRunner play it unchanged."""

    def __init__(self, actor: Actor, device: str = "cuda:0"):
        self.actor = actor
        self.obs_dim = int(actor.obs_shape[0])
        # lz_act's parameter order without the critic, which lz_play does not read: actor net | std
        self.params = torch.cat([actor.architecture.flat().detach().cpu().float(),
                                 actor.distribution.std.detach().cpu().float()]).to(device).contiguous()
        if actor.distribution.dim != 2 or self.params.numel() != actor.architecture.numel() + 2:
            raise RuntimeError(f"loopz actor layout mismatch: {self.params.numel()} host parameters")
        self.scale = [float(v) for v in actor.distribution.action_scale]
        self._cfg = None
        self.actions = None

    @classmethod
    def from_checkpoint(cls, path: str, obs_dim: int, action_scale=1.0, device: str = "cuda:0", **arch):
        """The actor of a loopz `full_<update>.pt` (key actor_architecture_state_dict; the std and action scale
        from actor_distribution_state_dict when present)."""
        from ..sysid.dagger import load_teacher
        architecture = load_teacher(path, obs_dim, **arch)
        dist = SquashedGaussianDiagonalCovariance(2, 1.0, action_scale)
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        if "actor_distribution_state_dict" in ckpt:
            dist.load_state_dict(ckpt["actor_distribution_state_dict"])
        return cls(Actor(architecture, dist, device), device)

    def _cfg_for(self, n: int) -> LzCfg:
        if self._cfg is None or self._cfg.n_envs != n:
            c = LzCfg()
            c.n_envs, c.horizon, c.obs_dim, c.mini_batches, c.epochs = n, 1, self.obs_dim, 1, 1
            c.action_scale[0], c.action_scale[1] = self.scale
            self._cfg = c
            self.actions = torch.zeros((n, 2), device=self.params.device, dtype=torch.float32)
        return self._cfg

    def __call__(self, obs: torch.Tensor) -> torch.Tensor:
        if obs.dim() != 2 or obs.shape[1] != self.obs_dim:
            raise ValueError(f"obs must be [n][{self.obs_dim}], got {tuple(obs.shape)}")
        if obs.dtype != torch.float32 or obs.device != self.params.device or not obs.is_contiguous():
            obs = obs.to(self.params.device, torch.float32).contiguous()
        cfg = self._cfg_for(int(obs.shape[0]))
        _capi.call("lz_play", _capi.byref(cfg), _capi.ptr(self.params), _capi.ptr(obs), _capi.ptr(self.actions),
                   _capi.stream_ptr())
        return self.actions
