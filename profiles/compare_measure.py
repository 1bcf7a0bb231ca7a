"""Measurements of the teacher-vs-student comparison on one MI355X.

    python profiles/compare_measure.py [--n 4096 131072] [--reps 7] [--iters 20] [--arms] [--out profiles]

Kernel A/B: sysid_play with the matrix-core encoder (default flags) against SY_PLAY_SCALAR (k_sy_net<false>, the
kernel of sysid_student_step), obs 33, full windows of random frames, the two interleaved in one process: `reps`
pairs of `iters` calls each between device events after a warm-up of both; min and median per kernel, whether the
matrix-core kernel won every pair, and whether the two give the same zhat bits.  The encoder's share alone
(sysid_encode against the play kernel without the action head) follows from the zero-latent time, which runs the
action head only.  --arms: the time per env step of each arm of a comparison at the same n (teacher, tails,
student, zero latent) on a random scenario table, with random weights.  Writes <out>/compare_<n>.json."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
ENC_FLOP_PER_WINDOW = 2 * (50 * 25 * 32 + 11 * 256 * 32 + 7 * 160 * 32 + 3 * 160 * 32 + 96 * 8)   # obs 33: D = 25
HEAD_FLOP_PER_ENV = 2 * (33 * 128 + 128 * 128 + 128 * 2)


def make_agent(obs_dim=33, seed=1):
    from omniisaacgymenvs_loop_amd.loopz import MLPEncode_wrap
    from omniisaacgymenvs_loop_amd.sysid import StateHistoryEncoder, USVSysIDAgent
    torch.manual_seed(seed)
    teacher = MLPEncode_wrap([128, 128], torch.nn.LeakyReLU, obs_dim, 2, torch.nn.Tanh, False, speed_dim=3, mass_dim=8,
                             mass_latent_dim=8, mass_encoder_shape=(64, 16), seed=seed)
    enc = StateHistoryEncoder(torch.nn.LeakyReLU, input_size=obs_dim - 8, tsteps=50, output_size=8)
    return teacher, USVSysIDAgent(teacher=teacher, id_encoder=enc, history_len=50, obs_nonpriv_dim=obs_dim - 8,
                                  device=DEV)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters   # ms per call


def kernel_ab(n, reps, iters):
    from omniisaacgymenvs_loop_amd.sysid import HistoryStream
    _, agent = make_agent()
    hs = HistoryStream(n, 33, horizon=1, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(n)
    hs.reset()
    for _ in range(50):   # full windows of distinct random frames
        hs.append(torch.randn((n, 33), device=DEV, generator=g), None)
    z = {k: torch.zeros((n, 8), device=DEV) for k in ("mfma", "scalar", "zero")}
    act = {k: torch.zeros((n, 2), device=DEV) for k in z}
    run = {"mfma": lambda: agent.play_step(hs, z["mfma"], act["mfma"]),
           "scalar": lambda: agent.play_step(hs, z["scalar"], act["scalar"], scalar=True),
           "zero": lambda: agent.play_step(hs, z["zero"], act["zero"], zero_latent=True)}
    for f in run.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    same_bits = bool(torch.equal(z["mfma"].view(torch.int32), z["scalar"].view(torch.int32)))
    max_diff = float((z["mfma"] - z["scalar"]).abs().max())
    same_actions = bool(torch.equal(act["mfma"].view(torch.int32), act["scalar"].view(torch.int32)))
    t = {k: [] for k in run}
    for _ in range(reps):
        for k in ("mfma", "scalar", "zero"):
            t[k].append(timed(run[k], iters))
    out = {"n": n, "obs_dim": 33, "reps": reps, "iters_per_rep": iters, "zhat_same_bits": same_bits,
           "zhat_max_abs_diff": max_diff, "actions_same_bits": same_actions,
           "mfma_faster_in_every_pair": all(a < b for a, b in zip(t["mfma"], t["scalar"]))}
    for k in run:
        out[f"{k}_ms"] = {"min": min(t[k]), "median": statistics.median(t[k]), "all": t[k]}
    head = out["zero_ms"]["median"]
    for k in ("mfma", "scalar"):
        enc_ms = max(out[f"{k}_ms"]["median"] - head, 1e-9)
        out[f"{k}_encoder_ms_median"] = enc_ms
        out[f"{k}_encoder_tflops"] = ENC_FLOP_PER_WINDOW * n / (enc_ms * 1e-3) / 1e12
    out["floor_ms_at_157_tflops"] = (ENC_FLOP_PER_WINDOW + HEAD_FLOP_PER_ENV) * n / 157e12 * 1e3
    out["window_read_bytes"] = n * 50 * 25 * 4
    return out


def random_table(S, seed=3):
    from omniisaacgymenvs_loop_amd.scenario import SamplingParams, build_candidates, table_of
    cand = build_candidates(S, seed, SamplingParams(), sampler="philox", device=DEV)
    return table_of(cand, np.arange(S), {"sampler": "philox", "seed": seed})


def arm_times(n, steps):
    """ms per env step (policy + env step + evaluator) of each arm over `steps` steps of a playlist with one
    scenario per env."""
    from omniisaacgymenvs_loop_amd.loopz import Actor, LoopzTeacher, SquashedGaussianDiagonalCovariance
    from omniisaacgymenvs_loop_amd.scenario import ScenarioRunner
    from omniisaacgymenvs_loop_amd.scenario import compare as C
    from omniisaacgymenvs_loop_amd.sysid import SysIDStudent
    from omniisaacgymenvs_loop_amd.tasks.usv_config import load_yaml
    from omniisaacgymenvs_loop_amd.tasks.usv_virtual import USVVirtual
    yaml = os.path.join(ROOT, "omniisaacgymenvs_loop_amd", "cfg", "task", "USV", "IROS2024",
                        "USV_Virtual_CaptureXY_SysID-TEST.yaml")
    table = random_table(n)
    teacher_arch, agent = make_agent()
    actor = Actor(teacher_arch, SquashedGaussianDiagonalCovariance(2, 0.3, action_scale=[1.0, 1.0]), DEV)

    def factory():
        return ScenarioRunner(USVVirtual(load_yaml(yaml), num_envs=n, device=DEV, seed=7), table, rollouts=1)

    arms = C.arm_factories(["teacher", "teacher_base_tail", "teacher_wrong_tail", "student", "student_zero_latent"],
                           lambda r: LoopzTeacher(actor, DEV),
                           lambda r, zl: SysIDStudent(agent, n, zero_latent=zl), seed=1)
    out = {}
    for name, make in arms.items():
        runner = factory()
        policy = make(runner)
        runner.run(policy, max_steps=16, allow_incomplete=True, check_every=10 ** 9)   # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runner.run(policy, max_steps=steps, allow_incomplete=True, check_every=10 ** 9)
        torch.cuda.synchronize()
        out[name] = {"steps": int(runner.steps_taken), "ms_per_step": 1e3 * (time.perf_counter() - t0) / runner.steps_taken}
        del runner, policy
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 131072])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--arms", action="store_true")
    ap.add_argument("--arm-steps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compare_measure needs the GPU: a time from anywhere else says nothing")
    os.makedirs(a.out, exist_ok=True)
    for n in a.n:
        res = {"device": torch.cuda.get_device_name(0), "kernel_ab": kernel_ab(n, a.reps, a.iters)}
        path = os.path.join(a.out, f"compare_{n}.json")

        def save():
            with open(path, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")

        save()
        if a.arms:
            res["arm_ms_per_step"] = arm_times(n, a.arm_steps)
            save()
        ab = res["kernel_ab"]
        print(f"n={n}: mfma {ab['mfma_ms']['median']:.4f} ms (min {ab['mfma_ms']['min']:.4f}), scalar "
              f"{ab['scalar_ms']['median']:.4f} ms (min {ab['scalar_ms']['min']:.4f}), head only "
              f"{ab['zero_ms']['median']:.4f} ms; mfma faster in every pair: {ab['mfma_faster_in_every_pair']}; "
              f"same zhat bits: {ab['zhat_same_bits']} (max diff {ab['zhat_max_abs_diff']:.3g}); encoder "
              f"{ab['mfma_encoder_tflops']:.1f} vs {ab['scalar_encoder_tflops']:.1f} Tflop/s")
        if a.arms:
            print("  arms:", {k: round(v["ms_per_step"], 4) for k, v in res["arm_ms_per_step"].items()})


if __name__ == "__main__":
    main()
