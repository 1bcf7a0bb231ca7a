"""Measurements of the scenario tables.  Recorded, not asserted.

    python profiles/scenario_measure.py [n] [candidates] [out.json]

n (default 131072): envs = (scenario, rollout) pairs of the teacher-filter pass and rows of the fold; candidates
(default 1048576): usv_scn_generate / usv_scn_metrics.  Writes one JSON object (default profiles/scenario_<n>.json):
  mining    generate and metrics as candidates per second (median of 9 launches, device events) beside the host
            numpy sampler at a count it finishes in a few seconds
  fold      usv_scn_fold at n rows
  lz_play   beside lz_act with zero eps_inject and NULL storage pointers, median of alternating blocks
  filter    one ScenarioRunner pass at n pairs with a default-initialised teacher, per step and in all (the
            runner's construction, runner_setup_s, apart), beside eval.rollout with the same policy at the same env
            count (they differ by the playlist and the fold)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def _median(v):
    return sorted(v)[len(v) // 2]


def _event_ms(torch, fn, reps=9):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return _median(out)


def mining(torch, count, host_count=2000):
    from omniisaacgymenvs_loop_amd.scenario.sampling import (SamplingParams, generate_device, metrics_device,
                                                             sample_numpy)
    p = SamplingParams()
    rows, _ = generate_device(0, count, 0, p, DEV)
    gen_ms = _event_ms(torch, lambda: generate_device(0, count, 0, p, DEV))
    met_ms = _event_ms(torch, lambda: metrics_device(rows, p.obstacle_radius))
    t0 = time.perf_counter()
    sample_numpy(host_count, 0, p)
    host_s = time.perf_counter() - t0
    return {"candidates": count, "generate_ms": gen_ms, "metrics_ms": met_ms,
            "generate_candidates_per_s": count / (gen_ms * 1e-3), "metrics_candidates_per_s": count / (met_ms * 1e-3),
            "host_numpy_candidates": host_count, "host_numpy_s": host_s,
            "host_numpy_candidates_per_s": host_count / host_s}


def _task(n):
    from omniisaacgymenvs_loop_amd.tasks.usv_config import load_yaml
    from omniisaacgymenvs_loop_amd.tasks.usv_virtual import USVVirtual
    yaml_path = os.path.join(ROOT, "omniisaacgymenvs_loop_amd", "cfg", "task", "USV", "IROS2024",
                             "USV_Virtual_CaptureXY_SysID-TEST.yaml")
    return USVVirtual(load_yaml(yaml_path), num_envs=n, device=DEV, seed=42)


def _actor(obs_dim):
    from torch import nn

    from omniisaacgymenvs_loop_amd.loopz import Actor, MLPEncode_wrap, SquashedGaussianDiagonalCovariance
    arch = MLPEncode_wrap([128, 128], nn.LeakyReLU, obs_dim, 2, nn.Tanh, False, speed_dim=3, mass_dim=8)
    return Actor(arch, SquashedGaussianDiagonalCovariance(2, 0.3, action_scale=1.0), DEV)


def fold(torch, n):
    from omniisaacgymenvs_loop_amd import _capi
    from omniisaacgymenvs_loop_amd._abi import DEFINES as D
    from omniisaacgymenvs_loop_amd.eval import EpisodeEvaluator
    ev = EpisodeEvaluator(_task(n), episodes_per_env=1)
    ev.table.uniform_(0.0, 3.0)
    ev.table[D["USV_EV_REASON"]].floor_()
    ev.ep_count.fill_(1)
    ms = {}
    for r in (1, 4):
        s = n // r
        out = torch.zeros((D["USV_SCF_ROWS"], s), device=DEV, dtype=torch.float64)
        ms[f"S={s},R={r}"] = _event_ms(torch, lambda: _capi.call(
            "usv_scn_fold", _capi.byref(ev._ev), n, s, r, 1, 1.2, 80, 0.8, 200, _capi.ptr(out), _capi.stream_ptr()))
    return {"rows": n, "fold_ms": ms}


def lz_play(torch, n, blocks=40, calls=20):
    from omniisaacgymenvs_loop_amd import _capi
    from omniisaacgymenvs_loop_amd._abi import LzCfg
    from omniisaacgymenvs_loop_amd.loopz import LoopzTeacher
    obs_dim = 33
    teacher = LoopzTeacher(_actor(obs_dim), DEV)
    nparam = int(_capi.lib().lz_nparam(obs_dim))
    params = torch.zeros(nparam, device=DEV)
    params[:teacher.params.numel()] = teacher.params
    obs = torch.randn((n, obs_dim), device=DEV)
    eps = torch.zeros((n, 2), device=DEV)
    act = torch.zeros((n, 2), device=DEV)
    cfg = LzCfg()
    cfg.n_envs, cfg.horizon, cfg.obs_dim, cfg.mini_batches, cfg.epochs = n, 1, obs_dim, 1, 1
    cfg.action_scale[0] = cfg.action_scale[1] = 1.0

    def act_zero():
        _capi.call("lz_act", _capi.byref(cfg), _capi.ptr(params), _capi.ptr(obs), 0, None, None, None, None,
                   _capi.ptr(act), 0, 0, _capi.ptr(eps), _capi.stream_ptr())

    arms = {"lz_play": lambda: teacher(obs), "lz_act_zero_eps": act_zero}
    for fn in arms.values():
        fn()
    same = bool(torch.equal(teacher(obs), act))
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(blocks):
        for k, fn in arms.items():
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / calls)
    return {"num_envs": n, "blocks": blocks, "calls_per_block": calls, "bit_identical": same,
            "median_ms_per_call": {k: _median(v) for k, v in ms.items()}}


def filter_pass(torch, n):
    from omniisaacgymenvs_loop_amd.eval import EpisodeEvaluator, rollout
    from omniisaacgymenvs_loop_amd.loopz import LoopzTeacher
    from omniisaacgymenvs_loop_amd.scenario import ScenarioRunner
    from omniisaacgymenvs_loop_amd.scenario.sampling import (METRIC_KEYS, SamplingParams, generate_device,
                                                             metrics_device, rows_to_candidates, table_of)
    p = SamplingParams()
    t0 = time.perf_counter()
    rows, quat = generate_device(0, n, 0, p, DEV)
    met = metrics_device(rows, p.obstacle_radius).cpu().numpy().astype("float64")
    cands = rows_to_candidates(rows.cpu().numpy(), quat.cpu().numpy(), p, {k: met[i] for i, k in enumerate(METRIC_KEYS)})
    table = table_of(cands, range(n), {"sampling": p.meta()})
    table_s = time.perf_counter() - t0
    out = {"pairs": n, "table_build_s": table_s}
    for name in ("rollout", "runner"):
        task = _task(n)
        teacher = LoopzTeacher(_actor(int(task.num_observations)), DEV)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "runner":
            runner = ScenarioRunner(task, table, rollouts=1)
            t1 = time.perf_counter()
            fold_out = runner.run(teacher)
            steps = runner.steps_taken
            out["runner_setup_s"] = t1 - t0
            out["verdicts"] = {str(v): int((fold_out["verdict"] == v).sum()) for v in range(4)}
        else:
            ev = EpisodeEvaluator(task, episodes_per_env=1)
            steps, _ = rollout(task, teacher, ev)
            ev.summary()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0 - out.get("runner_setup_s", 0.0) * (name == "runner")
        out[name] = {"steps": steps, "wall_s": wall, "ms_per_step": wall * 1e3 / steps}
    return out


def main(argv):
    import torch
    n = int(argv[0]) if len(argv) > 0 else 131072
    count = int(argv[1]) if len(argv) > 1 else 1048576
    path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", f"scenario_{n}.json")
    res = {"num_envs": n, "device": torch.cuda.get_device_name(0)}
    for name, fn in (("mining", lambda: mining(torch, count)), ("fold", lambda: fold(torch, n)),
                     ("lz_play", lambda: lz_play(torch, n)), ("filter", lambda: filter_pass(torch, n))):
        res[name] = fn()
        print(name, json.dumps(res[name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {path}")


if __name__ == "__main__":
    main(sys.argv[1:])
