"""Measurements of the policy-bank evaluation.  Recorded, not asserted.

    python profiles/bank_measure.py ckpts DIR [models]          # a tree DIR/exp<m>/nn/last_*.pth of default-initialised
                                                                # networks (what a sweep leaves), for the modes below
    python profiles/bank_measure.py forward [models] [group] [reps]   # k_policy_bank and k_policy_step<true> on the
        same models x group rows, alternating, for a kernel trace in a run of its own:
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o bank -- python profiles/bank_measure.py forward
    python profiles/bank_measure.py stats DIR/.../bank_kernel_stats.csv    # the two kernels' rows of that trace
    python profiles/bank_measure.py procs DIR [group] [horizon] [rounds]   # wall time of one multi_model_eval process
        over the tree against one evaluate_policy process per checkpoint, alternating, each a fresh process
Every mode prints one JSON line.  GoToPose, 16 models x 4,096 envs, horizon 500 by default."""
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TASK = "USV/USV_Virtual_GoToPose"


def ckpts(out_dir, models=16):
    import torch

    from omniisaacgymenvs_loop_amd.rl_games import checkpoint as ckpt
    from omniisaacgymenvs_loop_amd.rl_games.a2c_continuous import default_linear_init
    nin = ckpt.NIN
    for m in range(models):
        obs_rms = torch.zeros(2 * nin + 1, dtype=torch.float64)
        obs_rms[nin:] = 1.0
        sd = ckpt.model_state_dict(default_linear_init(100 + m), obs_rms,
                                   torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64))
        ckpt.save_checkpoint(os.path.join(out_dir, f"exp{m:02d}", "nn", f"last_exp{m:02d}_ep_{100 + m}_rew_0"),
                             {"model": sd, "epoch": 100 + m})
    print(json.dumps({"mode": "ckpts", "dir": out_dir, "models": models}))


def forward(models=16, group=4096, reps=200):
    import torch

    from omniisaacgymenvs_loop_amd import _capi as c
    from omniisaacgymenvs_loop_amd._abi import DEFINES as D
    from omniisaacgymenvs_loop_amd._abi import PpoCfg
    from omniisaacgymenvs_loop_amd.rl_games.a2c_continuous import default_linear_init
    dev, n, nin = "cuda:0", models * group, D["PPO_NIN"]
    params = torch.stack([default_linear_init(100 + m) for m in range(models)]).to(dev)
    rms = torch.zeros((models, 2 * nin + 1), dtype=torch.float64, device=dev)
    rms[:, nin:] = 1.0
    obs = torch.randn((n, nin), device=dev).clamp(-12, 12)
    cfg = PpoCfg()
    cfg.horizon, cfg.n_envs, cfg.minibatch, cfg.normalize_input, cfg.rms_eps = 1, n, 64, 1, 1e-5
    f = lambda *s: torch.zeros(s, device=dev)
    sc = [f(n, nin), f(n, 2), f(n), f(n), f(n, 2), f(n, 2)]
    done8, dones = torch.zeros(n, device=dev, dtype=torch.uint8), torch.zeros(n, device=dev, dtype=torch.int64)
    act_a, act_b = f(n, 2), f(n, 2)
    val_rms = torch.tensor([0.0, 1.0, 1.0], device=dev, dtype=torch.float64)
    for _ in range(reps):
        c.call("ppo_policy_bank_step", c.byref(cfg), c.ptr(params), c.ptr(rms), c.ptr(obs), models, group,
               c.ptr(act_a), 0, c.stream_ptr())
        c.call("ppo_policy_step", c.byref(cfg), c.ptr(params[0]), c.ptr(rms[0]), c.ptr(val_rms), c.ptr(obs), 0,
               *[c.ptr(t) for t in sc], c.ptr(done8), c.ptr(dones), c.ptr(act_b), 42, 0, None, None, c.stream_ptr())
    torch.cuda.synchronize()
    same = bool(torch.equal(act_a[:group], sc[4][:group].clamp(-1, 1)))   # group 0 is model 0 in both
    print(json.dumps({"mode": "forward", "models": models, "group": group, "rows": n, "reps": reps,
                      "group0_equals_single_model_step": same}))


def stats(path):
    keys = ("k_policy_bank", "k_policy_step")
    rows = [r for r in csv.DictReader(open(path)) if any(k in r.get("Name", "") for k in keys)]
    print(json.dumps({"mode": "stats", "kernels": [{k: r[k] for k in ("Name", "Calls", "AverageNs", "MinNs", "MaxNs")
                                                    if k in r} for r in rows]}))


def _timed(args, limit):
    """(process wall seconds, the rollout seconds the tool itself reports in its "... in X s" line)."""
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, "-m"] + args, cwd=ROOT, check=True, timeout=limit, stdout=subprocess.PIPE,
                         text=True).stdout
    wall = time.perf_counter() - t0
    told = [ln for ln in out.splitlines() if ln.startswith("[") and " steps" in ln and ln.rstrip().endswith(" s")]
    return wall, float(told[-1].split(" in ")[-1].split()[0])


def procs(load_dir, group=4096, horizon=500, rounds=2):
    """Fresh processes, one at a time: the bank run (one process, models x group envs) and one evaluate_policy run
    of group envs per checkpoint, alternating.  A failing or overrunning child ends the measurement."""
    found = sorted(glob.glob(os.path.join(load_dir, "*", "nn", "last_*.pth")))
    common = [f"task={TASK}", f"num_envs={group}", f"eval.horizon={horizon}"]
    bank, singles = [], []
    for _ in range(rounds):
        bank.append(_timed(["omniisaacgymenvs_loop_amd.scripts.multi_model_eval", f"bank.load_dir={load_dir}"] + common,
                           300))
        singles.append([_timed(["omniisaacgymenvs_loop_amd.scripts.evaluate_policy", f"checkpoint={p}"] + common, 120)
                        for p in found])
    print(json.dumps({"mode": "procs", "task": TASK, "models": len(found), "envs_per_model": group, "horizon": horizon,
                      "bank_process_seconds": [w for w, _ in bank], "bank_rollout_seconds": [r for _, r in bank],
                      "single_process_seconds": [[w for w, _ in s] for s in singles],
                      "all_singles_process_seconds": [sum(w for w, _ in s) for s in singles],
                      "all_singles_rollout_seconds": [sum(r for _, r in s) for s in singles]}))


if __name__ == "__main__":
    mode, args = sys.argv[1], sys.argv[2:]
    if mode == "ckpts":
        ckpts(args[0], *[int(a) for a in args[1:]])
    elif mode == "forward":
        forward(*[int(a) for a in args])
    elif mode == "stats":
        stats(args[0])
    elif mode == "procs":
        procs(args[0], *[int(a) for a in args[1:]])
