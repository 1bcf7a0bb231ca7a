"""USVSysIDAgent / USVSysIDTrainer (omniisaacgymenvs/algo/ppo/dagger.py:13-195) on the kernels of
csrc/usv_sysid.hip, and SysIDStudent, the deployable policy as a callable obs -> action.

    z*  = teacher mass_encoder(priv tail)              (frozen)
    z^  = id_encoder(history of non-privileged obs)    (trained: MSE against z*)
    a   = teacher action_mlp([obs_nonpriv, z^])        (frozen)

One update = num_learning_epochs x num_mini_batches in-order minibatches of the time-major rows (t * n + env),
Adam(lr) with torch's defaults, StepLR(step_size 200, gamma 0.1) stepped once per update on the host (lr is a
kernel argument).  Nothing synchronises with the host inside an update; update() reads the metrics back once."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from .. import _capi
from .._abi import DEFINES
from ..loopz.module import MLPEncode_wrap
from .history import HistoryStream
from .module import StateHistoryEncoder, action_head_nn

LAT, MET_N = DEFINES["SY_LAT"], DEFINES["SY_MET_N"]
PLAY_ZERO_LATENT, PLAY_SCALAR = DEFINES["SY_PLAY_ZERO_LATENT"], DEFINES["SY_PLAY_SCALAR"]
# sysid_play's encoder kernels by name; DEFAULT_PLAY_KERNEL is the one the A/B of profiles/compare_measure.py
# favours
PLAY_KERNELS = ("default", "scalar")
DEFAULT_PLAY_KERNEL = "default"


def load_teacher(path: str, obs_dim: int, act_dim: int = 2, *, policy_net=(128, 128), speed_dim: int = 3,
                 mass_dim: int = 8, mass_latent_dim: int = 8, mass_encoder_shape=(64, 16)) -> MLPEncode_wrap:
    """The teacher actor's architecture from a loopz `full_<update>.pt` (actor_architecture_state_dict)."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if not (isinstance(ckpt, dict) and "actor_architecture_state_dict" in ckpt):
        raise RuntimeError(f"Checkpoint is not in loopz .pt dict format (missing actor_architecture_state_dict): {path}")
    arch = MLPEncode_wrap(list(policy_net), torch.nn.LeakyReLU, obs_dim, act_dim, torch.nn.Tanh, False,
                          speed_dim=speed_dim, mass_dim=mass_dim, mass_latent_dim=mass_latent_dim,
                          mass_encoder_shape=tuple(mass_encoder_shape))
    arch.load_state_dict(ckpt["actor_architecture_state_dict"])
    return arch


def action_head_mirror(teacher: MLPEncode_wrap) -> torch.nn.Sequential:
    """The teacher's frozen action head as torch.nn modules on the CPU (TorchScript export)."""
    net = action_head_nn(teacher.obs_dim - teacher.mass_dim + LAT, out_dim=teacher.output_size)
    sd = teacher.state_dict()
    net.load_state_dict({k[len("architecture.action_mlp."):]: v for k, v in sd.items() if ".action_mlp." in k})
    return net.eval()


class USVSysIDAgent:
    """teacher: the loopz actor's MLPEncode_wrap (its mass_encoder and action_mlp are used, frozen: the agent
    holds its own device copy); id_encoder: the StateHistoryEncoder to train, bound to a device vector here."""

    def __init__(self, *, teacher: MLPEncode_wrap, id_encoder: StateHistoryEncoder, history_len: int,
                 obs_nonpriv_dim: int, device: str) -> None:
        self.history_len = int(history_len)
        self.obs_nonpriv_dim = int(obs_nonpriv_dim)
        self.history_dim = self.history_len * self.obs_nonpriv_dim
        self.device = torch.device(device)
        if not teacher.out_tanh:
            raise NotImplementedError("the sysid kernels implement the teacher's Tanh action head")
        if teacher.obs_dim - teacher.mass_dim != self.obs_nonpriv_dim or id_encoder.input_size != self.obs_nonpriv_dim \
                or id_encoder.tsteps != self.history_len:
            raise ValueError("teacher, id_encoder and (history_len, obs_nonpriv_dim) do not describe the same observation")
        self.obs_dim = teacher.obs_dim
        self.teacher = teacher
        self.id_encoder = id_encoder
        self.teacher_flat = teacher.flat().to(self.device).contiguous()   # frozen
        self.enc_flat = id_encoder.flat().to(self.device).contiguous()
        assert self.enc_flat.numel() == _capi.lib().sysid_nparam(self.obs_dim)
        id_encoder.bind(self.enc_flat)

    @classmethod
    def from_checkpoint(cls, path: str, *, obs_dim: int, id_encoder: StateHistoryEncoder, history_len: int = 50,
                        device: str = "cuda:0", **teacher_kw) -> "USVSysIDAgent":
        teacher = load_teacher(path, obs_dim, **teacher_kw)
        return cls(teacher=teacher, id_encoder=id_encoder, history_len=history_len,
                   obs_nonpriv_dim=obs_dim - teacher.mass_dim, device=device)

    def set_itr(self, _itr):
        return

    def action_head_mirror(self) -> torch.nn.Sequential:
        return action_head_mirror(self.teacher)

    # the three networks on a HistoryStream
    def student_step(self, hs: HistoryStream, zhat: torch.Tensor, actions: torch.Tensor) -> None:
        _capi.call("sysid_student_step", _capi.ptr(self.enc_flat), _capi.ptr(self.teacher_flat), *hs.geometry(), hs.row,
                   _capi.ptr(hs.stream), _capi.ptr(hs.valid_rows), _capi.ptr(zhat), _capi.ptr(actions),
                   _capi.stream_ptr())

    def play_step(self, hs: HistoryStream, zhat: torch.Tensor, actions: torch.Tensor, zero_latent: bool = False,
                  scalar: bool = False) -> None:
        """The deployment step (sysid_play): forward only; zero_latent feeds the action head z^ = 0 and skips the
        encoder (dagger_usv_viz_loopz.py: sysid.zero_latent), scalar selects the scalar-FMA encoder kernel."""
        flags = (PLAY_ZERO_LATENT if zero_latent else 0) | (PLAY_SCALAR if scalar else 0)
        _capi.call("sysid_play", _capi.ptr(self.enc_flat), _capi.ptr(self.teacher_flat), *hs.geometry(), hs.row, flags,
                   _capi.ptr(hs.stream), _capi.ptr(hs.valid_rows), _capi.ptr(zhat), _capi.ptr(actions),
                   _capi.stream_ptr())

    def encode_rows(self, hs: HistoryStream, row0: int, rows: int, zhat: torch.Tensor) -> None:
        _capi.call("sysid_encode", _capi.ptr(self.enc_flat), *hs.geometry(), int(row0), int(rows), _capi.ptr(hs.stream),
                   _capi.ptr(hs.valid_rows), _capi.ptr(zhat), _capi.stream_ptr())


class SysIDStudent:
    """The student as a policy: actions = student(obs), obs [n][obs_dim] device tensor (the privileged tail is
    ignored).  It keeps its own history of the observations it was called with, so eval.rollout(task, student,
    evaluator) scores it unchanged.  A policy sees no done flags: the window slides across episode boundaries,
    as the env wrapper's default mode does; reset() empties it.  zero_latent: the ablation that feeds the action
    head z^ = 0; kernel: one of PLAY_KERNELS."""

    def __init__(self, agent: USVSysIDAgent, num_envs: int, zero_latent: bool = False,
                 kernel: str = DEFAULT_PLAY_KERNEL):
        if kernel not in PLAY_KERNELS:
            raise ValueError(f"kernel must be one of {PLAY_KERNELS}, got {kernel!r}")
        self.agent = agent
        self.zero_latent, self.kernel = bool(zero_latent), kernel
        self.history = HistoryStream(num_envs, agent.obs_dim, history_len=agent.history_len, horizon=1,
                                     device=agent.device)
        self.zhat = torch.zeros((num_envs, LAT), device=agent.device)
        self.actions = torch.zeros((num_envs, agent.teacher.output_size), device=agent.device)

    @classmethod
    def from_files(cls, teacher_pt: str, id_encoder_pth: str, *, num_envs: int, obs_dim: int, history_len: int = 50,
                   device: str = "cuda:0", zero_latent: bool = False, kernel: str = DEFAULT_PLAY_KERNEL,
                   **teacher_kw) -> "SysIDStudent":
        """The student of a loopz `full_<update>.pt` and the `id_encoder_<update>.pth` state dict sysid_distill
        wrote beside it."""
        teacher = load_teacher(teacher_pt, obs_dim, **teacher_kw)
        enc = StateHistoryEncoder(torch.nn.LeakyReLU, input_size=obs_dim - teacher.mass_dim, tsteps=history_len,
                                  output_size=LAT)
        sd = torch.load(id_encoder_pth, map_location="cpu", weights_only=True)
        enc.load_state_dict(sd.get("id_encoder_state_dict", sd) if isinstance(sd, dict) else sd)
        agent = USVSysIDAgent(teacher=teacher, id_encoder=enc, history_len=history_len,
                              obs_nonpriv_dim=obs_dim - teacher.mass_dim, device=device)
        return cls(agent, num_envs, zero_latent=zero_latent, kernel=kernel)

    def reset(self) -> None:
        self.history.reset()

    def __call__(self, obs: torch.Tensor) -> torch.Tensor:
        self.history.append(torch.nan_to_num(obs.float(), nan=0.0, posinf=0.0, neginf=0.0), None)
        self.agent.play_step(self.history, self.zhat, self.actions, zero_latent=self.zero_latent,
                             scalar=self.kernel == "scalar")
        return self.actions


def step_lr(lr0: float, updates_done: int, step_size: int = 200, gamma: float = 0.1) -> float:
    """torch.optim.lr_scheduler.StepLR's closed form after `updates_done` scheduler steps."""
    return float(lr0) * float(gamma) ** (int(updates_done) // int(step_size))


class USVSysIDTrainer:
    """The reference's constructor arguments plus `env`: the USVSysIDVecEnv (built with horizon =
    num_transitions_per_env) whose frame ring is the storage."""

    def __init__(self, *, actor: USVSysIDAgent, num_envs: int, num_transitions_per_env: int, history_dim: int,
                 latent_dim: int, num_learning_epochs: int = 4, num_mini_batches: int = 4, device: str,
                 learning_rate: float = 5e-4, env=None) -> None:
        self.actor = actor
        self.device = torch.device(device)
        self.history_dim, self.latent_dim = int(history_dim), int(latent_dim)
        self.num_envs, self.num_transitions_per_env = int(num_envs), int(num_transitions_per_env)
        self.num_learning_epochs, self.num_mini_batches = int(num_learning_epochs), int(num_mini_batches)
        if self.latent_dim != LAT or self.history_dim != actor.history_dim:
            raise NotImplementedError(f"the sysid kernels implement latent_dim {LAT} and the agent's history_dim")
        if env is None:
            raise ValueError("USVSysIDTrainer needs env=<USVSysIDVecEnv>: its frame ring is the trainer's storage")
        self.env = env
        hs: HistoryStream = env.history
        if hs.n != self.num_envs or hs.H != self.num_transitions_per_env:
            raise ValueError(f"env history is {hs.n} envs x horizon {hs.H}; the trainer was given "
                             f"{self.num_envs} x {self.num_transitions_per_env}")
        B = self.num_envs * self.num_transitions_per_env
        if B % self.num_mini_batches:
            raise ValueError("num_envs x num_transitions_per_env must be a multiple of num_mini_batches")
        self.hs = hs
        hs.teacher = actor.teacher_flat   # from now on every appended frame records z*
        self.learning_rate = float(learning_rate)
        self.itr = 0          # updates done (the scheduler's step count)
        self.adam_step = 0
        dev = self.device
        npar = actor.enc_flat.numel()
        self.adam_m = torch.zeros(npar, device=dev)
        self.adam_v = torch.zeros(npar, device=dev)
        self.grad = torch.zeros(npar, device=dev)
        self.partials = torch.zeros(_capi.lib().sysid_partials_floats(actor.obs_dim, B // self.num_mini_batches),
                                    device=dev)
        self._max_rows = B // self.num_mini_batches
        self.losses = torch.zeros(self.num_learning_epochs * self.num_mini_batches, device=dev)
        self.zhat = torch.zeros((self.num_envs, LAT), device=dev)
        self.actions = torch.zeros((self.num_envs, actor.teacher.output_size), device=dev)
        self.zhat_all = torch.zeros((B, LAT), device=dev)
        self.metrics_dev = torch.zeros(MET_N, device=dev, dtype=torch.float64)
        self.metrics_work = torch.zeros(_capi.lib().sysid_metrics_work_doubles(), device=dev, dtype=torch.float64)
        self._steps = 0

    @property
    def lr(self) -> float:
        return step_lr(self.learning_rate, self.itr)

    # ------------------------------------------------------------------ rollout
    def observe_device(self) -> torch.Tensor:
        """The student's actions for the env's current observation (a buffer rewritten by the next call)."""
        self.env._flush()
        self.actor.student_step(self.hs, self.zhat, self.actions)
        return self.actions

    def observe(self, sysid_obs_np=None) -> np.ndarray:
        """Reference signature; the window is read from the ring, the argument is not needed."""
        return self.observe_device().detach().cpu().numpy()

    def step(self, sysid_obs_np=None, priv_tail_torch=None) -> None:
        """Reference signature.  (window, z*) of the current row are already in the ring: the frame and
        z* = mass_encoder(priv tail) were recorded by one kernel when the observation arrived."""
        self.env._flush()
        self._steps += 1

    # ------------------------------------------------------------------- update
    def minibatch(self, row0: int, rows: int, *, apply: bool = True, loss_slot: int = 0) -> None:
        if rows > self._max_rows:
            raise ValueError(f"minibatch of {rows} rows: the partial-gradient scratch holds {self._max_rows}")
        if apply:
            self.adam_step += 1
        a = self.actor
        _capi.call("sysid_minibatch", _capi.ptr(a.enc_flat), _capi.ptr(self.adam_m), _capi.ptr(self.adam_v),
                   *self.hs.geometry(), int(row0), int(rows), self.lr, self.adam_step, int(apply),
                   _capi.ptr(self.hs.stream), _capi.ptr(self.hs.valid_rows), _capi.ptr(self.hs.zstar),
                   _capi.ptr(self.partials), _capi.ptr(self.grad),
                   self.losses.data_ptr() + 4 * int(loss_slot), _capi.stream_ptr())

    def update_device(self) -> torch.Tensor:
        """The update without the read-back: returns the [SY_MET_N] doubles on the device."""
        if not self.hs.full:
            raise RuntimeError(f"update() after {self.hs.s} of {self.hs.H} steps")
        B = self.num_envs * self.num_transitions_per_env
        M = B // self.num_mini_batches
        for ep in range(self.num_learning_epochs):
            for mb in range(self.num_mini_batches):
                self.minibatch(mb * M, M, loss_slot=ep * self.num_mini_batches + mb)
        hs = self.hs
        _capi.call("sysid_metrics", _capi.ptr(self.actor.enc_flat), *hs.geometry(), _capi.ptr(hs.stream),
                   _capi.ptr(hs.valid_rows), _capi.ptr(hs.zstar), _capi.ptr(self.losses), self.losses.numel(),
                   self.num_mini_batches, _capi.ptr(self.zhat_all), _capi.ptr(self.metrics_work),
                   _capi.ptr(self.metrics_dev), _capi.stream_ptr())
        self.itr += 1
        self._steps = 0
        return self.metrics_dev

    def update(self) -> Dict[str, float]:
        return metrics_dict(self.update_device().cpu().numpy())


def metrics_dict(m: np.ndarray) -> Dict[str, float]:
    """sysid_metrics' doubles under the reference's names."""
    D = DEFINES
    out = {"mse": float(m[D["SY_MET_MSE"]]), "zstar_var_mean": float(m[D["SY_MET_ZSTAR_VAR"]]),
           "zhat_var_mean": float(m[D["SY_MET_ZHAT_VAR"]])}
    for i in range(LAT):
        out[f"r2_dim{i}"] = float(m[D["SY_MET_R2_DIM"] + i])
    out["r2_total"] = float(m[D["SY_MET_R2_TOTAL"]])
    return out
