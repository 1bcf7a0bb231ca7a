"""USVSysIDVecEnv (omniisaacgymenvs/envs/usv_raisim_vecenv.py:387-611) on top of loopz.vecenv.USVRaisimVecEnv:
the non-privileged observation, its history of `history_len` frames and the privileged tail.

The reference API is numpy (observe_sysid_obs / observe_history / observe_nonpriv) with get_priv_tail a device
tensor; the *_device twins return device tensors without the host copy.  The history lives in a HistoryStream
(a ring of frames on the device, history.py); `horizon` > 1 makes room for a USVSysIDTrainer, which trains on
the ring directly.

Two things follow the reference as it behaves, not as its comments read:
  * fill_history_on_reset = "zeros" (the default): reset() empties the window, but a done env's window is NOT
    cleared -- the reference zeroes a copy (`self._history_torch[done_mask].zero_()`, boolean-mask indexing
    returns a new tensor) -- so the window slides on across the episode boundary;
  * fill_history_on_reset = "repeat": reset() and every done fill the whole window with the current frame."""
from __future__ import annotations

from typing import Any, Tuple

import numpy as np
import torch

from ..loopz.vecenv import USVRaisimVecEnv
from .history import HistoryStream


class USVSysIDVecEnv(USVRaisimVecEnv):
    def __init__(self, base_env: Any, *, history_len: int = 50, priv_dim: int = 4,
                 fill_history_on_reset: str = "zeros", reward_info_size: int = 16, device=None,
                 horizon: int = 1) -> None:
        super().__init__(base_env, reward_info_size=reward_info_size, device=device)
        self.history_len = int(history_len)
        self.priv_dim = int(priv_dim)
        if self.history_len <= 0:
            raise ValueError(f"history_len must be > 0, got {self.history_len}")
        if self.priv_dim <= 0:
            raise ValueError(f"priv_dim must be > 0, got {self.priv_dim}")
        self.obs_nonpriv_dim = int(self.num_obs - self.priv_dim)
        if self.obs_nonpriv_dim <= 0:
            raise ValueError(f"Invalid dims: num_obs={self.num_obs}, priv_dim={self.priv_dim}")
        if fill_history_on_reset not in {"repeat", "zeros"}:
            raise ValueError("fill_history_on_reset must be 'repeat' or 'zeros'")
        if self.priv_dim != 8:
            raise NotImplementedError(f"the sysid kernels implement priv_dim 8 (mass, CoM, k_drag, thruster gains, "
                                      f"k_Iz), got {self.priv_dim}")
        self._fill_history_on_reset = fill_history_on_reset
        self.history = HistoryStream(self.num_envs, self.num_obs, history_len=self.history_len, horizon=horizon,
                                     fill_history_on_reset=fill_history_on_reset, device=self._device)
        self._pending = False   # the last observation is not in the ring yet

    # ----------------------------------------------------------------- stepping
    def reset_device(self) -> torch.Tensor:
        obs = super().reset_device()
        self.history.reset()
        self._pending = True
        return obs

    def step_device(self, action: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        self._flush()   # the frame this action was computed from is part of the history
        out = super().step_device(action)
        self._pending = True
        return out

    def _flush(self) -> None:
        """Append the last observation to the ring.  Deferred until the history is next needed (or the env stepped),
        so that after the last step of an update its rows stay intact until the trainer has used them."""
        if self._last_obs is None:
            self.reset_device()
        if self._pending:
            self.history.append(self._last_obs, self._last_dones)
            self._pending = False

    # ------------------------------------------------------------------- device
    def observe_nonpriv_device(self) -> torch.Tensor:
        return self.observe_device()[:, :self.obs_nonpriv_dim]

    def observe_history_device(self) -> torch.Tensor:
        self._flush()
        return self.history.window().reshape(self.num_envs, -1)

    def observe_sysid_obs_device(self) -> torch.Tensor:
        return torch.cat([self.observe_history_device(), self.observe_nonpriv_device()], dim=1)

    def get_priv_tail(self) -> torch.Tensor:
        """The current observation's privileged tail (encoded), [N, priv_dim] on the device."""
        return self.observe_device()[:, -self.priv_dim:]

    def get_priv_tail_from_obs(self, obs_full) -> torch.Tensor:
        obs_t = obs_full if torch.is_tensor(obs_full) else torch.from_numpy(np.asarray(obs_full))
        obs_t = obs_t.to(self._device, dtype=torch.float32)
        if obs_t.ndim != 2 or obs_t.shape[1] < self.priv_dim:
            raise ValueError(f"obs_full must be [N, >=priv_dim], got {tuple(obs_t.shape)} priv_dim={self.priv_dim}")
        return obs_t[:, -self.priv_dim:]

    # ------------------------------------------------------- reference (numpy)
    def observe_nonpriv(self) -> np.ndarray:
        return self.observe_nonpriv_device().detach().cpu().numpy().astype(np.float32, copy=False)

    def observe_history(self) -> np.ndarray:
        return self.observe_history_device().detach().cpu().numpy().astype(np.float32, copy=False)

    def observe_sysid_obs(self) -> np.ndarray:
        return np.concatenate([self.observe_history(), self.observe_nonpriv()], axis=1)
