"""SysID student distillation entry: the reference's stage 2 (omniisaacgymenvs/scripts/dagger_usv_sysid_loopz.py)
on the MI355X kernels (csrc/usv_sysid.hip) and this package's USV env.

    python -m omniisaacgymenvs_loop_amd.scripts.sysid_distill \
        task=USV/IROS2024/USV_Virtual_CaptureXY_SysID-TEST train=USV/USV_MLP \
        num_envs=4096 seed=42 checkpoint=runs/USV/nn/full_2000.pt max_iterations=1000 [cfg_dir=...]

The student encoder (StateHistoryEncoder over the last `history_len` non-privileged observations) is regressed
onto the frozen teacher's latent z* = mass_encoder(priv tail) while the student itself drives the env through the
teacher's frozen action_mlp (dagger_usv_sysid_loopz.py:337-349): one update every horizon_length steps, the env
not reset in between.  environment / architecture keys (history_len, speed_dim, mass_dim, sysid_eval_every_n,
policy_net, mass_latent_dim, ...) come from task/USV/IROS2024/cfg.yaml, as for loopz_train.  Written under
runs/dagger_<name>/<time>/nn/: export_meta.yaml, and at update 1 and every sysid_eval_every_n updates
id_encoder_<n>.pt and action_mlp_<n>.pt (TorchScript, traced on the CPU from a torch.nn mirror of the device
parameters: what the reference's ROS players load) and id_encoder_<n>.pth (the encoder's state_dict).
Single process; per update one line: update mse r2 zstar_var zhat_var fps."""
from __future__ import annotations

import os
import sys
import time

import torch
import yaml

from .loopz_train import merge_loopz_overrides
from .rlgames_train import build_config, parse_overrides


def export_meta(ckpt_dir: str, *, history_len: int, priv_dim: int, speed_dim: int, obs_nonpriv_dim: int,
                mass_latent_dim: int, checkpoint: str, device: str, eval_every_n: int) -> dict:
    """export_meta.yaml (dagger_usv_sysid_loopz.py:287-300): the dims the deployment side wires with."""
    meta = {"history_len": int(history_len), "priv_dim": int(priv_dim), "mass_dim": int(priv_dim),
            "speed_dim": int(speed_dim), "obs_nonpriv_dim": int(obs_nonpriv_dim),
            "history_dim": int(history_len * obs_nonpriv_dim), "mass_latent_dim": int(mass_latent_dim),
            "action_in_dim": int(obs_nonpriv_dim + mass_latent_dim), "checkpoint": str(checkpoint),
            "device": str(device), "eval_every_n": int(eval_every_n)}
    os.makedirs(ckpt_dir, exist_ok=True)
    with open(os.path.join(ckpt_dir, "export_meta.yaml"), "w") as f:
        yaml.safe_dump(meta, f, sort_keys=False)
    return meta


def export_student(ckpt_dir: str, updates: int, id_encoder, teacher) -> tuple:
    """id_encoder_<n>.pt / action_mlp_<n>.pt (torch.jit.trace of the CPU mirrors) and id_encoder_<n>.pth."""
    from ..sysid import action_head_mirror
    os.makedirs(ckpt_dir, exist_ok=True)
    enc, act = id_encoder.torch_mirror(), action_head_mirror(teacher)
    id_path = os.path.join(ckpt_dir, f"id_encoder_{updates}.pt")
    act_path = os.path.join(ckpt_dir, f"action_mlp_{updates}.pt")
    with torch.no_grad():
        torch.jit.save(torch.jit.trace(enc, torch.rand(1, id_encoder.input_shape), check_trace=False), id_path)
        torch.jit.save(torch.jit.trace(act, torch.rand(1, act[0].in_features), check_trace=False), act_path)
    torch.save(id_encoder.state_dict(), os.path.join(ckpt_dir, f"id_encoder_{updates}.pth"))
    return id_path, act_path


def build(cfg, ckpt_dir):
    from ..envs.vec_env_rlgames import VecEnvRLGames
    from ..sysid import StateHistoryEncoder, USVSysIDAgent, USVSysIDTrainer, USVSysIDVecEnv
    from ..utils.task_util import initialize_task
    ec, ac = cfg.get("environment", {}), cfg.get("architecture", {})
    eval_every_n = int(ec.get("sysid_eval_every_n", 100))
    history_len = int(ec.get("history_len", 50))
    speed_dim = int(ec.get("speed_dim", 3))
    te = cfg["task"]["env"]
    priv_dim = te.get("priv_dim", te.get("mass_dim", None))
    priv_dim = int(priv_dim) if priv_dim is not None else int(ec.get("mass_dim", 4))
    mass_latent_dim = int(ac.get("mass_latent_dim", 8))
    if not cfg.get("checkpoint"):
        raise SystemExit("sysid_distill needs checkpoint=<teacher full_N.pt> (scripts/loopz_train.py writes them)")
    device = cfg.get("rl_device", "cuda:0")
    rollout_steps = int(cfg["train"]["params"]["config"].get("horizon_length", 16))
    env_rlg = VecEnvRLGames(headless=True)
    initialize_task(cfg, env_rlg)
    env = USVSysIDVecEnv(env_rlg, history_len=history_len, priv_dim=priv_dim, horizon=rollout_steps)
    env.reset()
    id_encoder = StateHistoryEncoder(torch.nn.LeakyReLU, input_size=env.obs_nonpriv_dim, tsteps=history_len,
                                     output_size=mass_latent_dim, seed=int(cfg["seed"]))
    agent = USVSysIDAgent.from_checkpoint(
        cfg["checkpoint"], obs_dim=env.num_obs, id_encoder=id_encoder, history_len=history_len, device=device,
        act_dim=env.num_acts, policy_net=ac.get("policy_net", [128, 128]), speed_dim=speed_dim, mass_dim=priv_dim,
        mass_latent_dim=mass_latent_dim, mass_encoder_shape=tuple(int(v) for v in (ac.get("mass_encoder_shape") or (64, 16))))
    export_meta(ckpt_dir, history_len=history_len, priv_dim=priv_dim, speed_dim=speed_dim,
                obs_nonpriv_dim=env.obs_nonpriv_dim, mass_latent_dim=mass_latent_dim, checkpoint=cfg["checkpoint"],
                device=device, eval_every_n=eval_every_n)
    trainer = USVSysIDTrainer(actor=agent, num_envs=env.num_envs, num_transitions_per_env=rollout_steps,
                              history_dim=history_len * env.obs_nonpriv_dim, latent_dim=mass_latent_dim,
                              num_learning_epochs=4, num_mini_batches=4, device=device, learning_rate=5e-4, env=env)
    return env, agent, trainer, rollout_steps, eval_every_n


def distill(cfg, max_updates=None, run_dir=None, log=print):
    name = cfg["train"]["params"]["config"]["name"]
    if run_dir is None:
        run_dir = os.path.join("runs", f"dagger_{name}", time.strftime("%Y-%m-%d-%H-%M-%S"))
    ckpt_dir = os.path.join(run_dir, "nn")
    env, agent, trainer, rollout_steps, eval_every_n = build(cfg, ckpt_dir)
    if max_updates is None:
        max_updates = int(cfg.get("max_iterations") or cfg["train"]["params"]["config"].get("max_epochs", 500000))
    history, start = [], time.time()
    env.reset()
    for updates in range(1, int(max_updates) + 1):
        for _ in range(rollout_steps):
            actions = trainer.observe_device()
            trainer.step()
            env.step_device(actions)
        m = trainer.update()
        if eval_every_n > 0 and (updates == 1 or updates % eval_every_n == 0):
            id_path, act_path = export_student(ckpt_dir, updates, agent.id_encoder, agent.teacher)
            env.save_scaling(ckpt_dir, str(updates))
            log(f"[sysid] saved: {id_path} {act_path}")
        fps = updates * rollout_steps * env.num_envs / max(1e-6, time.time() - start)
        m = dict(m, update=updates, fps=fps, lr=trainer.lr)
        history.append(m)
        log(f"[sysid] update={updates} mse={m['mse']:.6g} r2={m['r2_total']:.4f} "
            f"zstar_var={m['zstar_var_mean']:.3g} zhat_var={m['zhat_var_mean']:.3g} fps={fps:.1f}")
    return history, env, agent, trainer, ckpt_dir


def main(argv=None):
    ov = parse_overrides(sys.argv[1:] if argv is None else argv)
    ov.setdefault("train", "USV/USV_MLP")
    cfg_dir = ov.get("cfg_dir", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cfg"))
    cfg = build_config(ov)
    cfg = merge_loopz_overrides(cfg, cfg_dir)
    distill(cfg)


if __name__ == "__main__":
    main()
