"""SysID distillation timings: the HIP path (omniisaacgymenvs_loop_amd.sysid) against the reference's own method --
torch eager on the same GPU: a rolled [n][50][D] history buffer, every window flattened into a
[horizon][n][50 D] storage, nn.Module encoder / action head, torch.optim.Adam.

    python tools/sysid_bench.py --envs 4096 --torch [--updates 3] [--out profiles/sysid_4096.json]

--torch adds the torch-eager run; it completed at 4,096 envs only (at 32,768 and 131,072 envs it stayed inside
MIOpen's conv1d for minutes and did not finish: DESIGN.md section 13), so it is off by default.

Both drive the same USV env with the same random teacher.  Reported: student step (history update + encoder +
action head) in microseconds, one update (16 Adam steps + diagnostics) in milliseconds, and distillation
env-steps/s over whole updates (env steps included)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, T = 16, 50


def make_env(n, seed, sysid):
    from omniisaacgymenvs_loop_amd.envs.vec_env_rlgames import VecEnvRLGames
    from omniisaacgymenvs_loop_amd.loopz import USVRaisimVecEnv
    from omniisaacgymenvs_loop_amd.scripts import loopz_train as LT
    from omniisaacgymenvs_loop_amd.sysid import USVSysIDVecEnv
    from omniisaacgymenvs_loop_amd.utils.task_util import initialize_task
    cfg = LT.build_config({"num_envs": n, "seed": seed, "train": "USV/USV_MLP"})
    cfg = LT.merge_loopz_overrides(cfg, os.path.join(ROOT, "omniisaacgymenvs_loop_amd", "cfg"))
    rlg = VecEnvRLGames(headless=True)
    initialize_task(cfg, rlg)
    env = USVSysIDVecEnv(rlg, history_len=T, priv_dim=8, horizon=H) if sysid else USVRaisimVecEnv(rlg)
    env.reset()
    return env


def timed(fn, sync=torch.cuda.synchronize):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return time.perf_counter() - t0


def bench_hip(n, updates, teacher, enc):
    from omniisaacgymenvs_loop_amd.sysid import USVSysIDAgent, USVSysIDTrainer
    env = make_env(n, 1, True)
    agent = USVSysIDAgent(teacher=teacher, id_encoder=enc, history_len=T, obs_nonpriv_dim=env.obs_nonpriv_dim,
                          device="cuda:0")
    tr = USVSysIDTrainer(actor=agent, num_envs=n, num_transitions_per_env=H, history_dim=T * env.obs_nonpriv_dim,
                         latent_dim=8, device="cuda:0", env=env)
    step_s, upd_s, total = [], [], 0.0
    for u in range(updates + 1):   # update 0 warms up
        t_all = time.perf_counter()
        torch.cuda.synchronize()
        for _ in range(H):
            step_s.append(timed(lambda: tr.observe_device()))   # appends the frame (history update) first
            tr.step()
            env.step_device(tr.actions)
        upd_s.append(timed(lambda: tr.update_device()))
        if u > 0:
            total += time.perf_counter() - t_all
    mem = sum(t.numel() * t.element_size() for t in (env.history.stream, env.history.valid_rows, env.history.valid_cur,
                                                    env.history.zstar, tr.zhat_all))
    return {"student_step_us": 1e6 * min(step_s[H:]), "update_ms": 1e3 * min(upd_s[1:]),
            "env_steps_per_s": updates * H * n / total, "history_and_storage_bytes": mem}


def bench_torch(n, updates, teacher, enc):
    from omniisaacgymenvs_loop_amd.sysid import action_head_mirror
    env = make_env(n, 1, False)
    dev = "cuda:0"
    D = env.num_obs - 8
    net, head = enc.torch_mirror().to(dev).train(), action_head_mirror(teacher).to(dev)
    sd = teacher.state_dict()
    mass = torch.nn.Sequential(torch.nn.Linear(8, 64), torch.nn.LeakyReLU(), torch.nn.Linear(64, 16), torch.nn.LeakyReLU(),
                               torch.nn.Linear(16, 8), torch.nn.LeakyReLU()).to(dev)
    mass.load_state_dict({k[len("architecture.mass_encoder."):]: v for k, v in sd.items() if ".mass_encoder." in k})
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    hist = torch.zeros((n, T, D), device=dev)
    st_h = torch.zeros((H, n, T * D), device=dev)
    st_z = torch.zeros((H, n, 8), device=dev)
    hist[:, -1] = env.observe_device()[:, :D]
    state = {"hist": hist}

    def student(s):
        obs = env.observe_device()
        h = state["hist"].reshape(n, -1)
        with torch.no_grad():
            act = head(torch.cat([obs[:, :D], net(h)], 1))
            st_h[s].copy_(h)
            st_z[s].copy_(mass(obs[:, D:]))
        return act

    def roll():
        state["hist"] = torch.roll(state["hist"], -1, 1)
        state["hist"][:, -1] = env.observe_device()[:, :D]

    def update():
        Hh, Z = st_h.view(-1, T * D), st_z.view(-1, 8)
        M = Hh.shape[0] // 4
        for _ in range(4):
            for mb in range(4):
                loss = torch.nn.functional.mse_loss(net(Hh[mb * M:(mb + 1) * M]), Z[mb * M:(mb + 1) * M])
                opt.zero_grad()
                loss.backward()
                opt.step()
        with torch.no_grad():
            zh = net(Hh)
            sse = ((zh - Z) ** 2).sum(0)
            sst = ((Z - Z.mean(0, keepdim=True)) ** 2).sum(0)
            return torch.stack([torch.var(Z, 0, unbiased=False).mean(), torch.var(zh, 0, unbiased=False).mean(),
                                1 - sse.sum() / (sst.sum() + 1e-8)])

    step_s, upd_s, total = [], [], 0.0
    for u in range(updates + 1):
        t_all = time.perf_counter()
        torch.cuda.synchronize()
        for s in range(H):
            box = {}
            step_s.append(timed(lambda: box.update(a=student(s))))
            env.step_device(box["a"])
            step_s[-1] += timed(roll)
        upd_s.append(timed(update))
        if u > 0:
            total += time.perf_counter() - t_all
    return {"student_step_us": 1e6 * min(step_s[H:]), "update_ms": 1e3 * min(upd_s[1:]),
            "env_steps_per_s": updates * H * n / total,
            "history_and_storage_bytes": (hist.numel() + st_h.numel() + st_z.numel()) * 4,
            "peak_allocated_bytes": torch.cuda.max_memory_allocated()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--torch", action="store_true", help="also time the torch-eager method")
    a = ap.parse_args()
    from omniisaacgymenvs_loop_amd.loopz import MLPEncode_wrap
    from omniisaacgymenvs_loop_amd.sysid import StateHistoryEncoder
    teacher = MLPEncode_wrap([128, 128], torch.nn.LeakyReLU, 33, 2, torch.nn.Tanh, False, speed_dim=3, mass_dim=8,
                             mass_latent_dim=8, mass_encoder_shape=(64, 16), seed=1)
    res = {"envs": a.envs, "horizon": H, "updates_timed": a.updates}
    res["hip"] = bench_hip(a.envs, a.updates, teacher, StateHistoryEncoder(torch.nn.LeakyReLU, 25, T, 8, seed=2))
    print(json.dumps(res), flush=True)
    if a.torch:
        res["torch_eager"] = bench_torch(a.envs, a.updates, teacher,
                                         StateHistoryEncoder(torch.nn.LeakyReLU, 25, T, 8, seed=2))
        res["speedup"] = {k: (res["torch_eager"][k] / res["hip"][k] if k != "env_steps_per_s"
                              else res["hip"][k] / res["torch_eager"][k])
                          for k in ("student_step_us", "update_ms", "env_steps_per_s")}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
