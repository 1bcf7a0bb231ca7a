"""Torch-CPU restatement of the reference's SysID distillation (scripts/dagger_usv_sysid_loopz.py:337-349 with
algo/ppo/dagger.py USVSysIDAgent / USVSysIDTrainer, module.py:392-448 StateHistoryEncoder(tsteps=50),
envs/usv_raisim_vecenv.py:583-610 the history buffer), with autograd and torch.optim.Adam.

tests/test_sysid_cpu.py validates it against tests/golden/sysid_golden.npz, which the reference's own classes
produced; the GPU tests use it for shapes the fixture cannot hold.  dtype float32 is the reference's arithmetic;
float64 gives the conditioning yardstick of the parameter checks."""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

T, LAT, PRIV, CH = 50, 8, 8, 32
ENC_KEYS = ["encoder.0.weight", "encoder.0.bias", "conv_layers.0.weight", "conv_layers.0.bias",
            "conv_layers.2.weight", "conv_layers.2.bias", "conv_layers.4.weight", "conv_layers.4.bias",
            "linear_output.0.weight", "linear_output.0.bias"]
TEACHER_KEYS = [f"architecture.mass_encoder.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")] + \
               [f"architecture.action_mlp.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]


def enc_shapes(D: int):
    return [(CH, D), (CH,), (CH, CH, 8), (CH,), (CH, CH, 5), (CH,), (CH, CH, 5), (CH,), (LAT, CH * 3), (LAT,)]


def teacher_shapes(D: int):
    return [(64, 8), (64,), (16, 64), (16,), (8, 16), (8,), (128, D + LAT), (128,), (128, 128), (128,), (2, 128), (2,)]


def unflatten(flat, keys, shapes) -> Dict[str, torch.Tensor]:
    flat = torch.as_tensor(np.asarray(flat))
    out, p = {}, 0
    for k, s in zip(keys, shapes):
        n = int(np.prod(s))
        out[k] = flat[p:p + n].reshape(s).clone()
        p += n
    assert p == flat.numel()
    return out


def flatten(sd, keys) -> np.ndarray:
    return torch.cat([sd[k].detach().reshape(-1) for k in keys]).numpy()


def random_enc(D: int, seed: int) -> Dict[str, torch.Tensor]:
    """PyTorch's default nn.Linear / nn.Conv1d init: U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weight and bias."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, s in zip(ENC_KEYS, enc_shapes(D)):
        if k.endswith("weight"):
            bound = 1.0 / np.sqrt(int(np.prod(s[1:])))
        out[k] = (torch.rand(s, generator=g) * 2 - 1) * bound
    return out


def random_teacher(D: int, seed: int) -> Dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, s in zip(TEACHER_KEYS, teacher_shapes(D)):
        if k.endswith("weight"):
            bound = 1.5 / np.sqrt(s[1])
        out[k] = (torch.rand(s, generator=g) * 2 - 1) * bound
    return out


def encoder_forward(sd, hist_flat):
    bs = hist_flat.shape[0]
    proj = F.leaky_relu(F.linear(hist_flat.reshape(bs * T, -1), sd[ENC_KEYS[0]], sd[ENC_KEYS[1]]))
    x = proj.reshape(bs, -1, T)   # the raw reshape: conv input (c, t) = projection element c * T + t
    x = F.leaky_relu(F.conv1d(x, sd[ENC_KEYS[2]], sd[ENC_KEYS[3]], stride=4))
    x = F.leaky_relu(F.conv1d(x, sd[ENC_KEYS[4]], sd[ENC_KEYS[5]]))
    x = F.leaky_relu(F.conv1d(x, sd[ENC_KEYS[6]], sd[ENC_KEYS[7]]))
    return F.leaky_relu(F.linear(x.flatten(1), sd[ENC_KEYS[8]], sd[ENC_KEYS[9]]))


def teacher_latent(tsd, priv):
    x = priv
    for i in (0, 2, 4):
        x = F.leaky_relu(F.linear(x, tsd[f"architecture.mass_encoder.{i}.weight"], tsd[f"architecture.mass_encoder.{i}.bias"]))
    return x


def action_head(tsd, x):
    for i in (0, 2):
        x = F.leaky_relu(F.linear(x, tsd[f"architecture.action_mlp.{i}.weight"], tsd[f"architecture.action_mlp.{i}.bias"]))
    return torch.tanh(F.linear(x, tsd["architecture.action_mlp.4.weight"], tsd["architecture.action_mlp.4.bias"]))


class History:
    """[n][T][D]; reset: zeros + current in the last frame ("repeat": all frames = current); update: roll by one,
    current in the last frame; on done envs "repeat" refills the window, "zeros" changes NOTHING (the reference
    zeroes a copy)."""

    def __init__(self, n, D, mode, dtype=torch.float32):
        assert mode in ("zeros", "repeat")
        self.h = torch.zeros((n, T, D), dtype=dtype)
        self.mode = mode

    def reset(self, cur):
        if self.mode == "repeat":
            self.h[:] = cur[:, None, :]
        else:
            self.h.zero_()
            self.h[:, -1] = cur

    def update(self, cur, dones):
        self.h = torch.roll(self.h, -1, 1)
        self.h[:, -1] = cur
        if self.mode == "repeat":
            m = torch.as_tensor(np.asarray(dones)).bool()
            self.h[m] = cur[m][:, None, :].expand(-1, T, -1)

    def flat(self):
        return self.h.reshape(self.h.shape[0], -1).clone()


def metrics_of(zhat, zstar) -> Dict[str, float]:
    out = {"zstar_var_mean": float(torch.var(zstar, 0, unbiased=False).mean()),
           "zhat_var_mean": float(torch.var(zhat, 0, unbiased=False).mean())}
    sse = ((zhat - zstar) ** 2).sum(0)
    sst = ((zstar - zstar.mean(0, keepdim=True)) ** 2).sum(0)
    r2 = 1.0 - sse / (sst + 1e-8)
    for i in range(LAT):
        out[f"r2_dim{i}"] = float(r2[i])
    out["r2_total"] = float(1.0 - sse.sum() / (sst.sum() + 1e-8))
    return out


def step_lr(lr0, updates_done):
    return lr0 * 0.1 ** (updates_done // 200)


def run(obs, dones, teacher, enc, mode="zeros", horizon=16, epochs=4, mini_batches=4, lr=5e-4,
        dtype=torch.float32, forced: Optional[List[np.ndarray]] = None, keep_hist=False, n_updates=None):
    """obs [S + 1][n][obs_dim] (obs[0]: after reset), dones [S][n].  forced: flat encoder parameters loaded before
    each Adam step (teacher forcing: the step's gradient is then a function of the given parameters alone).
    Returns per-step zhat / zstar / actions, per-minibatch losses, gradients and the parameters each was taken at
    ("pre") [updates][epochs * mini_batches], the flat parameters after each update and each update's metrics."""
    obs = torch.as_tensor(np.asarray(obs)).to(dtype)
    S, n, D = len(dones), obs.shape[1], obs.shape[2] - PRIV
    tsd = {k: v.to(dtype) for k, v in teacher.items()}
    params = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in enc.items()}
    opt = torch.optim.Adam([params[k] for k in ENC_KEYS], lr=lr)
    hist = History(n, D, mode, dtype)
    hist.reset(obs[0, :, :D])
    out = {"zhat": [], "zstar": [], "actions": [], "hist": [], "losses": [], "grads": [], "pre": [], "params": [],
           "metrics": []}
    st_h, st_z, updates, k_forced = [], [], 0, 0
    for k in range(S):
        cur, h = obs[k, :, :D], hist.flat()
        with torch.no_grad():
            zh = encoder_forward(params, h)
            act = action_head(tsd, torch.cat([cur, zh], 1))
            zs = teacher_latent(tsd, obs[k, :, D:])[:, :LAT]
        out["zhat"].append(zh.numpy()), out["zstar"].append(zs.numpy()), out["actions"].append(act.numpy())
        if keep_hist:
            out["hist"].append(h.numpy())
        st_h.append(h), st_z.append(zs)
        hist.update(obs[k + 1, :, :D], dones[k])
        if len(st_h) == horizon:
            H_all, Z_all = torch.cat(st_h), torch.cat(st_z)   # time-major rows t * n + env
            M = H_all.shape[0] // mini_batches
            for g in opt.param_groups:
                g["lr"] = step_lr(lr, updates)
            losses, grads, pre = [], [], []
            for _ in range(epochs):
                for mb in range(mini_batches):
                    if forced is not None:
                        with torch.no_grad():
                            f = unflatten(forced[k_forced], ENC_KEYS, enc_shapes(D))
                            for kk in ENC_KEYS:
                                params[kk].copy_(f[kk].to(dtype))
                        k_forced += 1
                    pre.append(flatten(params, ENC_KEYS).copy())
                    loss = F.mse_loss(encoder_forward(params, H_all[mb * M:(mb + 1) * M]), Z_all[mb * M:(mb + 1) * M])
                    opt.zero_grad()
                    loss.backward()
                    grads.append(torch.cat([params[kk].grad.reshape(-1) for kk in ENC_KEYS]).numpy().copy())
                    opt.step()
                    losses.append(float(loss.detach()))
            with torch.no_grad():
                m = metrics_of(encoder_forward(params, H_all), Z_all)
            m["mse"] = float(np.mean(losses[-mini_batches:]))
            out["losses"].append(losses), out["grads"].append(grads), out["pre"].append(pre), out["metrics"].append(m)
            out["params"].append(flatten(params, ENC_KEYS).copy())
            st_h, st_z, updates = [], [], updates + 1
            if n_updates is not None and updates >= n_updates:
                break
    for kk in ("zhat", "zstar", "actions", "hist"):
        out[kk] = np.stack(out[kk]) if out[kk] else None
    return out


def make_stream(n, steps, obs_dim=33, seed=0, done_rate=0.04, forced_dones=()):
    """A scripted observation stream: obs [steps + 1][n][obs_dim] float32, dones [steps][n] int64; the privileged
    tail is constant within an episode and redrawn where the env is done."""
    g = np.random.default_rng(seed)
    D = obs_dim - PRIV
    obs = g.normal(0, 1, (steps + 1, n, obs_dim)).astype(np.float32)
    dones = (g.random((steps, n)) < done_rate).astype(np.int64)
    for s, e in forced_dones:
        dones[s, e] = 1
    priv = g.normal(0, 1, (n, PRIV)).astype(np.float32)
    for k in range(steps + 1):
        if k > 0:
            m = dones[k - 1].astype(bool)
            priv[m] = g.normal(0, 1, (int(m.sum()), PRIV)).astype(np.float32)
        obs[k, :, D:] = priv
    return obs, dones
