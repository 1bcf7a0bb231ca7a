"""Evaluate the checkpoints of a sweep at once: one rollout of M x num_envs envs, group m under checkpoint m, one
CSV row per model (the reference's omniisaacgymenvs/scripts/multi_model_eval.py, which restores one model after
the other into one player and copies every observation to the host).

    python -m omniisaacgymenvs_loop_amd.scripts.multi_model_eval \
        task=USV/USV_Virtual_GoToPose train=USV/USV_PPOcontinuous_MLP num_envs=4096 \
        bank.load_dir=runs [bank.pattern='nn/last_*_ep_*_rew_*.pth'] | bank.checkpoints=[a.pth,b.pth] \
        [bank.models_per_pass=8] [bank.paired=True] eval.horizon=500 [eval.thresholds=[...]] [eval.levels=[[...]]] \
        [eval.output_csv=bank.csv eval.summary_json=bank.json eval.per_env_csv=bank_envs.csv]

num_envs is the number of envs per model (a multiple of 32).  bank.load_dir holds one directory per experiment;
the model of an experiment is its file matching bank.pattern with the highest epoch, its name the experiment
directory (as in the reference); an experiment without a match is skipped.  Paired (the default): every model faces
the same num_envs scenarios -- the spawns, randomisation draws and noise of a num_envs-env run with this seed -- so
the rows compare scenario by scenario and each equals the stand-alone evaluation of that checkpoint.  With
bank.models_per_pass the checkpoints run in several passes over those same scenarios.

task.env.fixed_horizon_eval=True and task.env.maxEpisodeLength = horizon + 2 are set unless given, as
evaluate_policy does.  Not reproduced from the reference: its filter of all-zero-action envs (an Isaac bug), its
hard-coded task overrides (mass, kill_dist, ...: give them on the command line) and its plots.  TrackXYOVelocity's
reward holds a sum over all envs of the run, so its return column depends on which models share a pass."""
from __future__ import annotations

import glob
import os
import re
import sys
import time
from typing import List, Sequence, Tuple

from .evaluate_policy import _floats, _is_capture
from .rlgames_train import build_config, parse_overrides

BANK_DEFAULTS = {"bank.load_dir": "", "bank.pattern": "nn/last_*_ep_*_rew_*.pth", "bank.checkpoints": "",
                 "bank.models_per_pass": "", "bank.paired": True, "eval.horizon": 500, "eval.thresholds": "",
                 "eval.levels": "", "eval.output_csv": "", "eval.summary_json": "", "eval.per_env_csv": ""}
_EPOCH = re.compile(r"_ep_(\d+)_")


def _epoch_of(path: str) -> int:
    m = _EPOCH.search(os.path.basename(path))
    return int(m.group(1)) if m else -1


def discover_checkpoints(load_dir: str, pattern: str = BANK_DEFAULTS["bank.pattern"]) -> List[Tuple[str, str]]:
    """(experiment name, checkpoint path) per experiment directory of load_dir in name order: the match of
    <load_dir>/<experiment>/<pattern> with the highest epoch (_ep_<N>_ of the file name; ties by name)."""
    if not os.path.isdir(load_dir):
        raise SystemExit(f"bank.load_dir={load_dir}: not a directory")
    out = []
    for exp in sorted(os.listdir(load_dir)):
        if not os.path.isdir(os.path.join(load_dir, exp)):
            continue
        found = sorted(glob.glob(os.path.join(load_dir, exp, pattern)))
        if found:
            out.append((exp, max(found, key=_epoch_of)))
    return out


def named_checkpoints(paths: Sequence[str]) -> List[Tuple[str, str]]:
    """bank.checkpoints: the name of <experiment>/nn/<file>.pth is the experiment, of any other path the file
    stem; a repeated name gets its position appended."""
    out = []
    for i, p in enumerate(paths):
        p = str(p)
        d = os.path.dirname(os.path.abspath(p))
        name = os.path.basename(os.path.dirname(d)) if os.path.basename(d) == "nn" else \
            os.path.splitext(os.path.basename(p))[0]
        if any(name == n for n, _ in out):
            name = f"{name}#{i}"
        out.append((name, p))
    return out


def evaluate_bank(cfg, models: Sequence[Tuple[str, str]], group: int, horizon: int, thresholds=None, levels=None,
                  paired: bool = True, models_per_pass: int = 0):
    """The passes: returns (names, summaries, records, seconds) with the records of all passes concatenated and the
    wall time of the rollouts with their summaries and records read back (as evaluate_policy reports its own)."""
    import numpy as np

    from ..eval.bank_evaluator import BankTraceEvaluator, rollout_bank
    from ..rl_games.model_bank import ModelBank
    from ..tasks.usv_virtual import USVVirtual
    device = cfg.get("rl_device", "cuda:0")
    per = len(models) if models_per_pass < 1 else min(int(models_per_pass), len(models))
    normalize = bool(cfg["train"]["params"]["config"].get("normalize_input", False))
    names, summaries, records, wall = [], [], [], 0.0
    for first in range(0, len(models), per):
        part = models[first:first + per]
        task = USVVirtual(cfg["task"], num_envs=len(part) * group, device=device, seed=int(cfg["seed"]))
        bank = ModelBank([p for _, p in part], task.num_observations, device, normalize_input=normalize)
        ev = BankTraceEvaluator(task, horizon, len(part), group, thresholds=thresholds, levels=levels, paired=paired)
        t0 = time.perf_counter()
        rollout_bank(task, bank, ev)
        names += [n for n, _ in part]
        summaries += ev.summaries()
        rec = ev.records()   # (the read-backs synchronise)
        wall += time.perf_counter() - t0
        rec["model"] = rec["model"] + first
        rec["env"] = rec["env"] % group
        records.append(rec)
    return names, summaries, {k: np.concatenate([r[k] for r in records]) for k in records[0]}, wall


def main(argv=None):
    ov = parse_overrides(sys.argv[1:] if argv is None else argv)
    given = {k: ov.pop(k) for k in list(ov) if k.startswith("eval.") or k.startswith("bank.")}
    opt = dict(BANK_DEFAULTS)
    for k, v in given.items():
        if k not in opt:
            raise SystemExit(f"unknown override {k}")
        opt[k] = v
    horizon = int(opt["eval.horizon"])
    if horizon < 1:
        raise SystemExit(f"eval.horizon must be >= 1, got {horizon}")
    ov.setdefault("task.env.fixed_horizon_eval", True)
    ov.setdefault("task.env.maxEpisodeLength", horizon + 2)
    cfg = build_config(ov)
    if _is_capture(cfg):
        raise SystemExit("multi_model_eval evaluates the tasks without obstacles over a fixed horizon; CaptureXY is "
                         "evaluated per episode, one checkpoint at a time: evaluate_policy.py eval.episodes_per_env")
    if opt["bank.checkpoints"] != "":
        if opt["bank.load_dir"] != "":
            raise SystemExit("give bank.load_dir (with bank.pattern) or bank.checkpoints, not both")
        paths = opt["bank.checkpoints"]
        models = named_checkpoints(paths if isinstance(paths, (list, tuple)) else [paths])
    elif opt["bank.load_dir"] != "":
        models = discover_checkpoints(str(opt["bank.load_dir"]), str(opt["bank.pattern"]))
    else:
        raise SystemExit("bank.load_dir=<dir of experiments> or bank.checkpoints=[a.pth,...] expected")
    if not models:
        raise SystemExit(f"no checkpoint matches {opt['bank.pattern']} under {opt['bank.load_dir']}")
    group = int(cfg["num_envs"])
    if group < 32 or group % 32 != 0:
        raise SystemExit(f"num_envs (the envs per model) must be a multiple of 32, got {group}")
    per = int(opt["bank.models_per_pass"]) if opt["bank.models_per_pass"] != "" else 0
    import torch

    from ..eval import write_summary_json
    from ..eval.bank_report import format_bank_summary, write_bank_csv
    try:
        names, summaries, records, wall = evaluate_bank(cfg, models, group, horizon,
                                                        thresholds=_floats(opt["eval.thresholds"], "eval.thresholds"),
                                                        levels=_floats(opt["eval.levels"], "eval.levels"),
                                                        paired=bool(opt["bank.paired"]), models_per_pass=per)
    except ValueError as exc:   # a checkpoint of another network: the message names the file
        raise SystemExit(str(exc))
    torch.cuda.synchronize()
    print(format_bank_summary(names, summaries))
    print(f"[bank] {len(names)} models x {group} envs x {horizon} steps in {wall:.3f} s")
    if summaries[0]["channels"] == ["xy_velocity", "omega_velocity"]:
        print("[bank] TrackXYOVelocity: the reward holds a sum over all envs of a pass, so return_mean / return_std "
              "differ from a stand-alone evaluation of the checkpoint; every other column equals it")
    if opt["eval.output_csv"]:
        write_bank_csv(str(opt["eval.output_csv"]), names, summaries)
        print(f"[bank] wrote {len(names)} rows to {opt['eval.output_csv']}")
    report = {"models": {n: dict(s, checkpoint=p) for (n, p), s in zip(models, summaries)},   # in CSV row order
              "envs_per_model": group, "horizon": horizon, "paired": bool(opt["bank.paired"]),
              "models_per_pass": per if per > 0 else len(models), "wall_seconds": wall}
    if opt["eval.summary_json"]:
        write_summary_json(str(opt["eval.summary_json"]), report)
    if opt["eval.per_env_csv"]:
        import csv

        from ..eval.report import _fmt
        cols = ["model", "env"] + [k for k in records if k not in ("model", "env")]
        with open(str(opt["eval.per_env_csv"]), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(cols)
            for i in range(int(records["env"].shape[0])):
                w.writerow([names[int(records["model"][i])] if k == "model" else _fmt(records[k][i]) for k in cols])
    return names, summaries, report


if __name__ == "__main__":
    main()
