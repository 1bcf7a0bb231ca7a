"""HistoryStream: the device buffers behind USVSysIDVecEnv's history and USVSysIDTrainer's storage
(include/usv_hip.h "sysid").

The reference keeps a [n][T][D] window per env and copies every window into the trainer's storage
(horizon x n x T x D floats).  Here the non-privileged observations are a ring of R = T - 1 + horizon frames
[R][n][D]; the window of storage row (s, env) is the T ring slots from base + s on, so the storage of an update
is the stream itself and the last T - 1 frames carry over to the next update without a copy.  valid_rows
[horizon][n] holds what fill_history_on_reset = "repeat" needs: the number of trailing frames that are the
row's own (earlier positions read the first own frame)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _capi
from .._abi import DEFINES

T, LAT, PRIV = DEFINES["SY_T"], DEFINES["SY_LAT"], DEFINES["SY_PRIV"]
FILL = {"zeros": DEFINES["SY_FILL_ZEROS"], "repeat": DEFINES["SY_FILL_REPEAT"]}


class HistoryStream:
    def __init__(self, num_envs: int, obs_dim: int, *, history_len: int = T, horizon: int = 1,
                 fill_history_on_reset: str = "zeros", device="cuda:0"):
        if fill_history_on_reset not in FILL:
            raise ValueError("fill_history_on_reset must be 'repeat' or 'zeros'")
        self.n, self.obs_dim, self.T, self.H = int(num_envs), int(obs_dim), int(history_len), int(horizon)
        if _capi.lib().sysid_nparam(self.obs_dim) <= 0 or self.T != T:
            raise NotImplementedError(f"the sysid kernels implement history_len {T} and 33..36 observations with a "
                                      f"privileged tail of {PRIV}, got history_len {history_len}, obs {obs_dim}")
        if self.H < 1:
            raise ValueError(f"horizon must be >= 1, got {horizon}")
        self.D = self.obs_dim - PRIV
        self.R = self.T - 1 + self.H
        self.fill = FILL[fill_history_on_reset]
        self.device = torch.device(device)
        self.stream = torch.zeros((self.R, self.n, self.D), device=self.device)
        self.valid_rows = torch.full((self.H, self.n), self.T, device=self.device, dtype=torch.int32)
        self.valid_cur = torch.zeros(self.n, device=self.device, dtype=torch.int32)
        self.zstar = torch.zeros((self.H, self.n, LAT), device=self.device)
        self.teacher: Optional[torch.Tensor] = None   # flat teacher parameters: z* is recorded with each frame
        self.base, self.s, self.row = 0, 0, -1
        self._fresh = True

    def geometry(self):
        return self.n, self.obs_dim, self.T, self.H, self.base

    def reset(self) -> None:
        """As the reference's reset(): the window is empty (zeros, or in "repeat" mode filled by the next frame)."""
        self.stream.zero_()
        self.base, self.s, self.row = 0, 0, -1
        self._fresh = True

    @property
    def full(self) -> bool:
        """Every row of the current update has its frame."""
        return self.s == self.H

    def append(self, obs: torch.Tensor, dones: Optional[torch.Tensor]) -> None:
        """The observation the next action is computed from (and the dones of the env step that produced it)."""
        if self.s == self.H:   # the rows of the finished update are free: its last T - 1 frames stay in the ring
            self.base = (self.base + self.H) % self.R
            self.s = 0
        obs = obs.contiguous()
        assert obs.shape == (self.n, self.obs_dim) and obs.dtype == torch.float32
        if dones is not None:
            dones = dones.contiguous()
            assert dones.dtype == torch.int64 and dones.numel() == self.n
        _capi.call("sysid_append", _capi.ptr(obs), _capi.ptr(None if self._fresh else dones), _capi.ptr(self.teacher),
                   self.n, self.obs_dim, self.T, self.H, self.base, self.s, self.fill, int(self._fresh),
                   _capi.ptr(self.stream), _capi.ptr(self.valid_rows), _capi.ptr(self.valid_cur),
                   _capi.ptr(self.zstar), _capi.stream_ptr())
        self.row, self.s, self._fresh = self.s, self.s + 1, False

    def window(self, row: Optional[int] = None) -> torch.Tensor:
        """The [n][T][D] window of storage row `row` (default: the current one), gathered into a new tensor."""
        row = self.row if row is None else int(row)
        if row < 0:
            raise RuntimeError("no frame yet: reset the env first")
        k = torch.arange(self.T, device=self.device)[None, :]
        kk = torch.maximum(k, self.T - self.valid_rows[row].long()[:, None])
        slot = (self.base + row + kk) % self.R
        return self.stream[slot, torch.arange(self.n, device=self.device)[:, None]]

    def current(self) -> torch.Tensor:
        """The newest frame [n][D] (a view of the ring)."""
        return self.stream[(self.base + self.row + self.T - 1) % self.R]
