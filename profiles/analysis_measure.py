"""Measure the analysis stage (scenario.analysis.paired_bootstrap, csrc/usv_analysis.hip) on the device.

    python profiles/analysis_measure.py --S 131072 [--n-boot 2000 --calls 9 --restate-boot 200]
        writes profiles/analysis_<S>.json: paired_bootstrap timed between device events (warm-up, then the median
        and the minimum of --calls calls), usv_ana_bootstrap alone the same way (draws per second), and the numpy
        restatement of the same job (tests/analysis_restate.boot_mean_ci on the device's deltas, one run, on
        --restate-boot replicates and scaled to n_boot when fewer).
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- \
        python profiles/analysis_measure.py --S 131072 --profile-only
        a run of its own for the kernel split; then
    python profiles/analysis_measure.py --S 131072 --merge-stats DIR/.../t_kernel_stats.csv
        adds the split to the JSON (no device needed).

The job: S scenarios x R = 1 rollout in two arms (n = S envs, K = 1), synthetic evaluator tables from a seed,
the ten paired metrics, n_boot replicates.  There is no other implementation in the product package, so the
yardstick is the restatement on the same machine's CPU."""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def out_path(S):
    return os.path.join(ROOT, "profiles", f"analysis_{S}.json")


def make_arm(S, seed, p_succ, device):
    """An ArmTable stand-in: [USV_EV_ROWS][S] doubles, one record per env."""
    import torch

    from omniisaacgymenvs_loop_amd import _capi
    from omniisaacgymenvs_loop_amd._abi import DEFINES as D
    from omniisaacgymenvs_loop_amd._abi import UsvEval
    g = torch.Generator(device="cpu").manual_seed(seed)
    tab = torch.zeros((D["USV_EV_ROWS"], S), dtype=torch.float64)
    succ = (torch.rand(S, generator=g) < p_succ).double()
    steps = torch.randint(20, 400, (S,), generator=g).double()
    tab[D["USV_EV_SUCCESS"]] = succ
    tab[D["USV_EV_COLLISION"]] = (1.0 - succ) * (torch.rand(S, generator=g) < 0.5).double()
    tab[D["USV_EV_RETURN"]] = torch.randn(S, generator=g, dtype=torch.float64) * 12.0 + 30.0
    tab[D["USV_EV_PATH_LENGTH"]] = torch.rand(S, generator=g, dtype=torch.float64) * 9.0 + 2.0
    tab[D["USV_EV_PATH_EFF"]] = torch.rand(S, generator=g, dtype=torch.float64) * 0.5 + 0.5
    tab[D["USV_EV_LEN_STEPS"]] = steps
    tab[D["USV_EV_TIME_TO_GOAL"]] = torch.where(succ == 1.0, steps * 0.2, torch.full_like(steps, float("nan")))
    tab[D["USV_EV_MIN_OBS_EP"]] = torch.rand(S, generator=g, dtype=torch.float64) * 2.6 + 0.4

    class Arm:
        pass

    arm = Arm()
    arm.table, arm.ep_count = tab.to(device), torch.ones(S, dtype=torch.int32, device=device)
    ev = UsvEval()
    ev.acc, ev.episodes, ev.ep_count = None, _capi.ptr(arm.table), _capi.ptr(arm.ep_count)
    ev.max_episodes, ev.action_scale, ev.control_dt = 1, 1.0, 0.2
    arm.ev = ev
    return arm


def timed(fn, calls, warmup=2):
    """Milliseconds between device events around each of `calls` calls, after `warmup` calls."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def stat(ms):
    return {"calls": len(ms), "median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)),
            "max_ms": float(np.max(ms))}


def measure(args):
    import torch

    from omniisaacgymenvs_loop_amd.scenario import analysis as A
    from tests import analysis_restate as AR
    if not torch.cuda.is_available():
        raise SystemExit("analysis_measure needs the GPU: nothing is measured without one")
    S, B, dev = args.S, args.n_boot, "cuda:0"
    control, treat = make_arm(S, 1, 0.75, dev), make_arm(S, 2, 0.6, dev)

    def job():
        return A.paired_bootstrap(control, treat, S, S, 1, 1, 0.37, n_boot=B, seed=0)

    if args.profile_only:
        for _ in range(4):
            job()
        torch.cuda.synchronize()
        return
    rows = job()
    d = A.pair_deltas(control, treat, S, S, 1, 1, 0.37)
    finite = torch.isfinite(d)
    counts = finite.sum(1).cpu().numpy().astype(np.int64)
    values, seg_off = d[finite], np.concatenate([[0], np.cumsum(counts)])
    draws = int(counts.sum()) * B
    whole = stat(timed(job, args.calls))
    boot = stat(timed(lambda: A.bootstrap_means(values, seg_off, B, 0), args.calls))
    means = A.bootstrap_means(values, seg_off, B, 0)
    quant = stat(timed(lambda: A.quantiles(means, A.CI, A.NAN_PROPAGATE), args.calls))
    deltas = timed(lambda: A.pair_deltas(control, treat, S, S, 1, 1, 0.37), args.calls)
    # the yardstick: the reference's loop in numpy on this machine's CPU, one run
    host = d.cpu().numpy()
    rb = min(args.restate_boot, B)
    t0 = time.perf_counter()
    ref = [AR.boot_mean_ci(host[m], rb, np.random.default_rng(0)) for m in range(host.shape[0])]
    restate_s = time.perf_counter() - t0
    out = {"job": {"S": S, "R": 1, "n_boot": B, "metrics": len(rows), "n_pairs": [r["n_pairs"] for r in rows],
                   "draws_per_call": draws},
           "device": torch.cuda.get_device_name(0),
           "paired_bootstrap": whole,
           "usv_ana_bootstrap": {**boot, "draws_per_second_median": draws / (boot["median_ms"] * 1e-3),
                                 "draws_per_second_best": draws / (boot["min_ms"] * 1e-3)},
           "usv_ana_quantiles": quant, "usv_ana_pair_deltas": stat(deltas),
           "numpy_restatement": {"replicates_timed": rb, "seconds": restate_s,
                                 "seconds_scaled_to_n_boot": restate_s * B / rb,
                                 "what": "boot_mean_ci per metric on the device's deltas (the bootstrap and the "
                                         "percentiles; the reference's O(keys x rows) pairing loop is not timed)"},
           "speedup_vs_restatement_median": restate_s * B / rb / (whole["median_ms"] * 1e-3),
           "interval_check": {"metric": rows[3]["metric"], "device": [rows[3]["ci95_lo"], rows[3]["ci95_hi"]],
                              "restatement": [ref[3][2], ref[3][3]],
                              "note": "different index streams: the ends agree to the bootstrap's own noise"}}
    with open(out_path(S), "w") as f:
        json.dump(out, f, indent=2)
        f.write("\n")
    print(json.dumps(out))


def merge_stats(args):
    rows = list(csv.DictReader(open(args.merge_stats)))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    split = [{"kernel": r["Name"].replace("(anonymous namespace)::", "").split("(")[0][-60:], "calls": int(r["Calls"]),
              "avg_us": float(r["AverageNs"]) / 1e3, "total_ms": float(r["TotalDurationNs"]) / 1e6,
              "share": float(r["TotalDurationNs"]) / tot} for r in rows[:12]]
    path = out_path(args.S)
    out = json.load(open(path)) if os.path.exists(path) else {}
    out["kernel_split"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own (4 paired_bootstrap calls)",
                           "kernels": split}
    with open(path, "w") as f:
        json.dump(out, f, indent=2)
        f.write("\n")
    for k in split:
        print(f"{k['kernel']:60s} {k['calls']:5d} {k['avg_us']:10.1f} us {100 * k['share']:5.1f} %")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=4096)
    ap.add_argument("--n-boot", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--restate-boot", type=int, default=2000)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--merge-stats", default="")
    args = ap.parse_args()
    if args.merge_stats:
        merge_stats(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
