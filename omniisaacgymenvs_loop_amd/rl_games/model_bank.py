"""ModelBank: M checkpoints of the 128 x 128 MLP stacked on the device and served by one launch
(ppo_policy_bank_step, include/usv_hip.h): rows [m G, (m + 1) G) of the observation batch run under checkpoint m
and its own observation statistics.  The reference's scripts/multi_model_eval.py restores one model after the
other into one player; here every model of a sweep plays at once."""
from __future__ import annotations

from typing import Sequence

import torch

from .. import _capi
from .._abi import DEFINES, PpoCfg
from . import checkpoint as ckpt

NIN, NA, NPARAM = DEFINES["PPO_NIN"], DEFINES["PPO_NA"], DEFINES["PPO_NPARAM"]


def checkpoint_input_width(sd, path: str) -> int:
    """The input width of the checkpoint's network; ValueError naming the file when it is not the 128 x 128 MLP
    of PPO_NPARAM's layout."""
    for k, shape in ckpt.PARAM_LAYOUT:
        if k not in sd:
            raise ValueError(f"{path}: no tensor {k}: not a checkpoint of the {ckpt.NH} x {ckpt.NH} MLP")
        got = tuple(sd[k].shape)
        ok = (len(got) == 2 and got[0] == ckpt.NH and 1 <= got[1] <= NIN) if k == ckpt.W1_KEY else got == tuple(shape)
        if not ok:
            raise ValueError(f"{path}: tensor {k} has shape {got}: not a checkpoint of the {ckpt.NH} x {ckpt.NH} MLP "
                             f"with at most {NIN} inputs")
    return int(sd[ckpt.W1_KEY].shape[1])


class ModelBank:
    """paths: the checkpoints, in group order; obs_dim: the task's observation width (every checkpoint's input
    width).  normalize_input as the train config's (the statistics of a checkpoint are applied when it is on)."""

    def __init__(self, paths: Sequence[str], obs_dim: int, device: str = "cuda:0", normalize_input: bool = True):
        self.paths = [str(p) for p in paths]
        if not self.paths:
            raise ValueError("ModelBank: no checkpoint given")
        self.models, self.obs_dim, self.device = len(self.paths), int(obs_dim), device
        params = torch.zeros((self.models, NPARAM), dtype=torch.float32)
        obs_rms = torch.zeros((self.models, 2 * NIN + 1), dtype=torch.float64)
        obs_rms[:, NIN:] = 1.0
        val_rms = torch.zeros(3, dtype=torch.float64)
        for m, path in enumerate(self.paths):
            sd = ckpt.load_checkpoint(path)["model"]
            width = checkpoint_input_width(sd, path)
            if width != self.obs_dim:
                raise ValueError(f"{path}: the network has {width} inputs, the bank's "
                                 f"{'task' if m == 0 else 'other checkpoints'} have {self.obs_dim}")
            ckpt.load_model_state_dict(sd, params[m], obs_rms[m], val_rms, self.obs_dim)
        self.params, self.obs_rms = params.to(device), obs_rms.to(device)
        self.cfg = PpoCfg()
        self.cfg.horizon, self.cfg.minibatch = 1, 64
        self.cfg.normalize_input = int(bool(normalize_input))
        self.cfg.rms_eps = 1e-5
        self._actions = None
        self._obs_pad = None

    def get_action(self, obs: torch.Tensor, grid_cap: int = 0) -> torch.Tensor:
        """clamp(mu, -1, 1) of obs [M * G][obs_dim] (G a multiple of 32), row e under model e // G; the returned
        tensor is rewritten by the next call."""
        n = int(obs.shape[0])
        if n % self.models != 0:
            raise ValueError(f"{n} observation rows do not split into {self.models} groups")
        if self._actions is None or self._actions.shape[0] != n:
            self._actions = torch.zeros((n, NA), device=self.device, dtype=torch.float32)
            pad = self.obs_dim < NIN   # k-input network: zero-padded to the kernels' NIN inputs
            self._obs_pad = torch.zeros((n, NIN), device=self.device, dtype=torch.float32) if pad else None
        if self._obs_pad is not None:
            self._obs_pad[:, :self.obs_dim].copy_(obs)
            obs = self._obs_pad
        self.cfg.n_envs = n
        c = _capi
        c.call("ppo_policy_bank_step", c.byref(self.cfg), c.ptr(self.params), c.ptr(self.obs_rms),
               c.ptr(obs.contiguous()), self.models, n // self.models, c.ptr(self._actions), int(grid_cap),
               c.stream_ptr())
        return self._actions
