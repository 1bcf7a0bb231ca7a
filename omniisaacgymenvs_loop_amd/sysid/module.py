"""StateHistoryEncoder (omniisaacgymenvs/algo/ppo/module.py:392-448, tsteps = 50): the parameter container of
the student's history encoder.  The HIP kernels of csrc/usv_sysid.hip evaluate and train it on one flat vector
in state_dict order; this class keeps the reference's constructor arguments, PyTorch's default initialisation
of nn.Linear / nn.Conv1d (the reference applies no other) and the state_dict keys

    encoder.0.{weight,bias}  conv_layers.{0,2,4}.{weight,bias}  linear_output.0.{weight,bias}

so exported students are interchangeable with the reference's.  torch_mirror() is the same network as plain
torch.nn modules on the CPU, for TorchScript export and for checking the kernels."""
from __future__ import annotations

from typing import Dict, List

import numpy as np
import torch
from torch import nn

from .._abi import DEFINES

T, LAT, CH = DEFINES["SY_T"], DEFINES["SY_LAT"], DEFINES["SY_CH"]


class EncoderNN(nn.Module):
    """Linear(D -> 32) per frame, the [bs * T, 32] projection reshaped raw to [bs, 32, T] (no transpose), three
    Conv1d(32, 32) with (kernel, stride) (8, 4), (5, 1), (5, 1), flatten, Linear(96 -> L); LeakyReLU(0.01) after each."""

    def __init__(self, input_size: int, tsteps: int, output_size: int):
        super().__init__()
        self.tsteps = int(tsteps)
        self.encoder = nn.Sequential(nn.Linear(input_size, CH), nn.LeakyReLU())
        self.conv_layers = nn.Sequential(nn.Conv1d(CH, CH, kernel_size=DEFINES["SY_K1"], stride=DEFINES["SY_S1"]),
                                         nn.LeakyReLU(),
                                         nn.Conv1d(CH, CH, kernel_size=DEFINES["SY_K2"], stride=1), nn.LeakyReLU(),
                                         nn.Conv1d(CH, CH, kernel_size=DEFINES["SY_K2"], stride=1), nn.LeakyReLU(),
                                         nn.Flatten())
        self.linear_output = nn.Sequential(nn.Linear(CH * DEFINES["SY_L3"], output_size), nn.LeakyReLU())

    def forward(self, obs):
        bs = obs.shape[0]
        proj = self.encoder(obs.reshape(bs * self.tsteps, -1))
        return self.linear_output(self.conv_layers(proj.reshape(bs, -1, self.tsteps)))


def action_head_nn(in_dim: int, hidden: int = 128, out_dim: int = 2) -> nn.Sequential:
    """The teacher's `architecture.action_mlp` (keys 0, 2, 4): LeakyReLU hidden layers, Tanh output."""
    return nn.Sequential(nn.Linear(in_dim, hidden), nn.LeakyReLU(), nn.Linear(hidden, hidden), nn.LeakyReLU(),
                         nn.Linear(hidden, out_dim), nn.Tanh())


class StateHistoryEncoder:
    """StateHistoryEncoder(activation_fn, input_size, tsteps, output_size).  The kernels implement tsteps 50,
    output_size 8, LeakyReLU and input_size 25..28 (obs 33..36 less the privileged tail of 8)."""

    KEYS = ["encoder.0.weight", "encoder.0.bias"] + \
           [f"conv_layers.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")] + \
           ["linear_output.0.weight", "linear_output.0.bias"]

    def __init__(self, activation_fn, input_size: int, tsteps: int, output_size: int, seed: int = 0):
        name = getattr(activation_fn, "__name__", str(activation_fn))
        if "LeakyReLU" not in name:
            raise NotImplementedError(f"the sysid kernels implement LeakyReLU, got {name}")
        if int(tsteps) != T:
            raise NotImplementedError(f"the sysid kernels implement tsteps {T}, got {tsteps}")
        if int(output_size) != LAT:
            raise NotImplementedError(f"the sysid kernels implement output_size {LAT}, got {output_size}")
        self.activation_fn = activation_fn
        self.tsteps = int(tsteps)
        self.input_size = int(input_size)
        self.input_shape = self.input_size * self.tsteps
        self.output_shape = int(output_size)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(int(seed))
            net = EncoderNN(self.input_size, self.tsteps, self.output_shape)
        self._sd: Dict[str, torch.Tensor] = {k: v.detach().clone() for k, v in net.state_dict().items()}
        assert list(self._sd) == self.KEYS
        self._bound = None

    def shapes(self) -> List:
        return [(k, tuple(self._sd[k].shape)) for k in self.KEYS]

    def numel(self) -> int:
        return sum(int(np.prod(s)) for _, s in self.shapes())

    def flat(self) -> torch.Tensor:
        return torch.cat([self._sd[k].reshape(-1) for k in self.KEYS])

    def bind(self, flat: torch.Tensor) -> None:
        """From now on the parameters live in `flat` (a device vector the kernels train in place)."""
        self._bound = flat

    def state_dict(self) -> Dict[str, torch.Tensor]:
        if self._bound is None:
            return {k: v.clone() for k, v in self._sd.items()}
        host, out, p = self._bound.detach().cpu(), {}, 0
        for k, s in self.shapes():
            n = int(np.prod(s))
            out[k] = host[p:p + n].reshape(s).clone()
            p += n
        return out

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        for k, s in self.shapes():
            if tuple(sd[k].shape) != s:
                raise RuntimeError(f"size mismatch for {k}: {tuple(sd[k].shape)} vs {s}")
        self._sd = {k: sd[k].detach().float().cpu().clone() for k in self.KEYS}
        if self._bound is not None:
            self._bound.copy_(self.flat().to(self._bound.device))

    def parameters(self):
        return [self._sd[k] for k in self.KEYS]

    def torch_mirror(self) -> EncoderNN:
        """The current parameters as a torch.nn module on the CPU."""
        net = EncoderNN(self.input_size, self.tsteps, self.output_shape)
        net.load_state_dict(self.state_dict())
        return net.eval()
