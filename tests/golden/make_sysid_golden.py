"""Generate tests/golden/sysid_golden.npz: the reference's SysID distillation on a scripted observation stream.

Run only where the reference tree exists (make_golden.REF):
    python tests/golden/make_sysid_golden.py

The reference's OWN classes run here, on the CPU: StateHistoryEncoder and MLPEncode_wrap (algo/ppo/module.py),
USVSysIDAgent / USVSysIDTrainer with ObsStorage (algo/ppo/dagger.py, storage.py) and USVSysIDVecEnv
(envs/usv_raisim_vecenv.py) over a scripted base env that replays a recorded stream of observations and dones
(make_golden.ScriptedVecEnv is the precedent).  The loop is scripts/dagger_usv_sysid_loopz.py:337-349, which is
inline in its hydra main: observe_sysid_obs, get_priv_tail, trainer.observe, trainer.step, env.step, and
trainer.update every 16 steps.  Per-minibatch losses and the first gradient are read off the reference trainer
through its own loss_fn / optimizer objects.

n = 6 envs, 80 steps (5 updates), both fill_history_on_reset modes.  The fixture holds arrays and name lists only."""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_golden import REF  # noqa: E402

from tests import sysid_restate as R  # noqa: E402

N, STEPS, H, OBS = 6, 80, 16, 33
D = OBS - R.PRIV
FORCED_DONES = ((3, 1), (20, 4), (60, 2))
HIST_STEPS = (0, 1, 4, 21, 49, 50, 61, 79)   # first frames, after a done (3+1, 20+1, 60+1), first full window, last


def _load(name, path, package=None):
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=None)
    mod = importlib.util.module_from_spec(spec)
    if package:
        mod.__package__ = package
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    base = os.path.join(REF, "omniisaacgymenvs")
    pkg = types.ModuleType("refppo")
    pkg.__path__ = [os.path.join(base, "algo", "ppo")]
    sys.modules["refppo"] = pkg
    module = _load("refppo.module", os.path.join(base, "algo", "ppo", "module.py"), "refppo")
    _load("refppo.storage", os.path.join(base, "algo", "ppo", "storage.py"), "refppo")
    dagger = _load("refppo.dagger", os.path.join(base, "algo", "ppo", "dagger.py"), "refppo")
    vecenv = _load("ref_usv_raisim_vecenv", os.path.join(base, "envs", "usv_raisim_vecenv.py"))
    return module, dagger, vecenv


class ScriptedBaseEnv:
    """Replays obs [S + 1][n][obs] / dones [S][n]; what USVRaisimVecEnv touches of a VecEnvRLGames."""

    def __init__(self, obs, dones):
        self.obs, self.dones, self.k = torch.as_tensor(obs), torch.as_tensor(dones), 0
        self.num_envs = obs.shape[1]
        self._task = types.SimpleNamespace(num_observations=obs.shape[2], num_actions=2, num_envs=obs.shape[1],
                                           rl_device="cpu", device="cpu")
        self.actions = []

    def reset(self):
        self.k = 0
        return {"obs": {"state": self.obs[0].clone()}}

    def step(self, actions):
        self.actions.append(actions.clone())
        k = self.k
        self.k += 1
        return {"obs": {"state": self.obs[k + 1].clone()}}, torch.zeros(self.num_envs), self.dones[k].clone(), {}


def run_reference(mode, obs, dones, teacher_sd, enc_sd):
    module, dagger, vecenv = load_reference()
    nn = torch.nn
    teacher = module.MLPEncode_wrap([128, 128], nn.LeakyReLU, OBS, 2, nn.Tanh, False, speed_dim=3, mass_dim=R.PRIV,
                                    mass_latent_dim=R.LAT, mass_encoder_shape=(64, 16))
    teacher.load_state_dict(teacher_sd, strict=True)
    enc = module.StateHistoryEncoder(nn.LeakyReLU, input_size=D, tsteps=R.T, output_size=R.LAT)
    keys = [(k, tuple(v.shape)) for k, v in enc.state_dict().items()]
    enc.load_state_dict(enc_sd, strict=True)
    env = vecenv.USVSysIDVecEnv(ScriptedBaseEnv(obs, dones), history_len=R.T, priv_dim=R.PRIV,
                                fill_history_on_reset=mode)
    agent = dagger.USVSysIDAgent(teacher_mass_encoder=teacher.architecture.mass_encoder, id_encoder=enc,
                                 frozen_action_head=teacher.architecture.action_mlp, history_len=R.T,
                                 obs_nonpriv_dim=D, device="cpu")
    trainer = dagger.USVSysIDTrainer(actor=agent, num_envs=N, num_transitions_per_env=H, history_dim=R.T * D,
                                     latent_dim=R.LAT, num_learning_epochs=4, num_mini_batches=4, device="cpu",
                                     learning_rate=5e-4)
    losses, grads = [], []
    inner_loss = trainer.loss_fn

    def loss_fn(pred, target):
        v = inner_loss(pred, target)
        losses.append(float(v.item()))
        return v
    trainer.loss_fn = loss_fn
    inner_step = trainer.optimizer.step

    def opt_step(*a, **k):
        grads.append(torch.cat([p.grad.reshape(-1) for p in enc.parameters()]).numpy().copy())
        return inner_step(*a, **k)
    trainer.optimizer.step = opt_step

    out = {"zhat": [], "zstar": [], "actions": [], "hist": {}, "params": {}, "metrics": []}
    env.reset()
    for k in range(STEPS):
        sysid_obs = env.observe_sysid_obs()
        priv_tail = env.get_priv_tail()
        if k in HIST_STEPS:
            out["hist"][k] = env.observe_history().copy()
        with torch.no_grad():
            out["zhat"].append(agent.get_history_encoding(torch.from_numpy(sysid_obs)).numpy().copy())
            out["zstar"].append(agent.teacher_latent(priv_tail)[:, :R.LAT].numpy().copy())
        actions = trainer.observe(sysid_obs)
        out["actions"].append(actions.copy())
        trainer.step(sysid_obs, priv_tail)
        env.step(actions)
        if (k + 1) % H == 0:
            out["metrics"].append(trainer.update())
            out["params"][(k + 1) // H] = torch.cat([p.detach().reshape(-1) for p in enc.parameters()]).numpy().copy()
    out["losses"], out["grads"], out["keys"] = np.asarray(losses, np.float64), grads, keys
    assert len(losses) == 5 * 16 and trainer.scheduler.get_last_lr()[0] == 5e-4
    return out


def metric_names():
    return ["mse", "zstar_var_mean", "zhat_var_mean"] + [f"r2_dim{i}" for i in range(R.LAT)] + ["r2_total"]


def main():
    obs, dones = R.make_stream(N, STEPS, OBS, seed=11, forced_dones=FORCED_DONES)
    teacher_sd, enc_sd = R.random_teacher(D, seed=21), R.random_enc(D, seed=22)
    fx = {"obs": obs, "dones": dones, "teacher": R.flatten(teacher_sd, R.TEACHER_KEYS),
          "enc0": R.flatten(enc_sd, R.ENC_KEYS), "hist_steps": np.asarray(HIST_STEPS),
          "metric_names": np.asarray(metric_names())}
    for mode in ("zeros", "repeat"):
        o = run_reference(mode, obs, dones, teacher_sd, enc_sd)
        fx["enc_keys"] = np.asarray([k for k, _ in o["keys"]])
        fx["enc_shapes"] = np.asarray([",".join(str(v) for v in s) for _, s in o["keys"]])
        for k in ("zhat", "zstar", "actions"):
            fx[f"{mode}_{k}"] = np.stack(o[k]).astype(np.float32)
        fx[f"{mode}_hist"] = np.stack([o["hist"][k] for k in HIST_STEPS]).astype(np.float32)
        fx[f"{mode}_losses"] = o["losses"]
        fx[f"{mode}_metrics"] = np.asarray([[m[k] for k in metric_names()] for m in o["metrics"]], np.float64)
        fx[f"{mode}_params5"] = o["params"][5]
        if mode == "zeros":
            fx["zeros_params1"] = o["params"][1]
            fx["zeros_grad0"] = o["grads"][0]
    path = os.path.join(HERE, "sysid_golden.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
