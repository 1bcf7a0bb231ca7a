"""Build a scenario table (the reference's omniisaacgymenvs/scripts/build_usv_scenario_table.py): unique
candidates of the task's sampling law with geometry-only difficulty metrics, a 1:3:1 preselection over the
density-score quantiles (the teacher filter's input) and an optional geometry-only final selection.

    python -m omniisaacgymenvs_loop_amd.scripts.scenario_table --n-candidates 500 --n-preselect 300 \
        --out-dir runs/scenarios [--sampler numpy|philox] [--n-selected 0] [--save-candidates] [--seed 0]

The arguments and defaults are the reference's, plus --sampler: numpy replays the reference's generator stream
(its tables bit for bit, on the host); philox draws the candidates and computes their metrics on the device
(usv_scn_generate / usv_scn_metrics), so --n-candidates can be 10^6 and beyond.  The quantile bins and the
per-bin rng.choice stay on the host with either.  Writes candidates_<n>_unique.npz (--save-candidates),
preselect_<n>.npz, selected_<n>.npz (--n-selected > 0) and scenario_table.meta.json."""
from __future__ import annotations

import argparse
import json
import os
import re


def load_task_cfg_value(task_yaml: str, dotted_key: str, default: float) -> float:
    """A numeric scalar of a task YAML by the last segment of its key (first match), else the default."""
    key = dotted_key.split(".")[-1]
    try:
        with open(task_yaml, "r", encoding="utf-8") as f:
            text = f.read()
    except OSError:
        return float(default)
    num = r"([-+]?(?:\d+(?:\.\d*)?|\.\d+)(?:[eE][-+]?\d+)?)"
    m = re.search(rf"^\s*{re.escape(key)}\s*:\s*{num}\s*$", text, re.MULTILINE)
    return float(m.group(1)) if m else float(default)


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--task-yaml", type=str, default="", help="Optional task YAML path to read scalar params from")
    p.add_argument("--out-dir", type=str, default="runs/scenarios", help="Output directory")
    p.add_argument("--n-candidates", type=int, default=500)
    p.add_argument("--n-preselect", type=int, default=300, help="Teacher input size")
    p.add_argument("--n-selected", type=int, default=0,
                   help="Optional geometry-only final selection size (0 disables; the teacher filter does it)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", type=str, default="cuda:0", help="device of the philox sampler")
    p.add_argument("--sampler", type=str, default="numpy", choices=["numpy", "philox"])
    p.add_argument("--big", type=int, default=16)
    p.add_argument("--goal-random-position", type=float, default=None)
    p.add_argument("--min-spawn-dist", type=float, default=None)
    p.add_argument("--max-spawn-dist", type=float, default=None)
    p.add_argument("--box-half-range", type=float, default=15.0)
    p.add_argument("--min-dist-safe", type=float, default=2.0)
    p.add_argument("--max-iterations", type=int, default=20)
    p.add_argument("--obstacle-radius", type=float, default=0.5)
    p.add_argument("--quant-m", type=float, default=0.05)
    p.add_argument("--init-vel-mode", type=str, default="zero", choices=["zero", "rand"],
                   help="zero = fixed (0, 0); rand = mimic the env reset")
    p.add_argument("--ratio", type=str, default="1:3:1", help="sparse:mid:dense ratio")
    p.add_argument("--save-candidates", action="store_true", help="Also save the candidates file")
    return p


def main(argv=None):
    from ..scenario import SamplingParams, build_candidates, preselect, save_table, select_from_pre, table_of
    args = parser().parse_args(argv)
    task_defaults = {"goal_random_position": 5.0, "min_spawn_dist": 0.5, "max_spawn_dist": 5.0}
    law = {}
    for k, dflt in task_defaults.items():
        v = getattr(args, k)
        if v is None and args.task_yaml:
            v = load_task_cfg_value(args.task_yaml, f"env.task_parameters.{k}", dflt)
        law[k] = float(dflt if v is None else v)
    try:
        ratio = tuple(int(x) for x in str(args.ratio).split(":"))
        if len(ratio) != 3:
            raise ValueError
    except ValueError:
        raise SystemExit(f"Invalid --ratio '{args.ratio}', expected like 1:3:1")
    params = SamplingParams(big=args.big, box_half_range=args.box_half_range, min_dist_safe=args.min_dist_safe,
                            max_iterations=args.max_iterations, obstacle_radius=args.obstacle_radius,
                            quant_m=args.quant_m, init_vel_mode=args.init_vel_mode, **law)
    params.check()
    meta = {"script": "omniisaacgymenvs_loop_amd/scripts/scenario_table.py", "seed": int(args.seed),
            "sampler": args.sampler, "sampling": params.meta(),
            "selection": {"n_candidates": int(args.n_candidates), "n_preselect": int(args.n_preselect),
                          "n_selected": int(args.n_selected), "ratio_sparse_mid_dense": list(ratio)},
            "notes": {"frame": "local (env origin)", "z_in_positions": "0.0 (to be set by sim reset if needed)",
                      "target_rot": "identity (task returns unchanged targets_orientation)"}}
    cands = build_candidates(args.n_candidates, args.seed, params, sampler=args.sampler, device=args.device)
    n_cand = int(cands["obstacles_xy"].shape[0])
    pre_idx, pre_summary = preselect(cands["metrics"]["density_score"], args.n_preselect, ratio, seed=args.seed + 1)
    meta["summary"] = {"preselect": pre_summary}
    sel_idx = None
    if args.n_selected > 0:
        sel_idx, sel_summary = select_from_pre(cands["metrics"]["density_score"][pre_idx], args.n_selected,
                                               seed=args.seed + 2)
        meta["summary"]["selected"] = sel_summary
    os.makedirs(args.out_dir, exist_ok=True)
    files = []
    if args.save_candidates:
        files.append(f"candidates_{n_cand}_unique.npz")
        save_table(os.path.join(args.out_dir, files[-1]), table_of(cands, range(n_cand), meta))
    files.append(f"preselect_{len(pre_idx)}.npz")
    save_table(os.path.join(args.out_dir, files[-1]), table_of(cands, pre_idx, meta, {"source_candidate_id": pre_idx}))
    if sel_idx is not None:
        files.append(f"selected_{len(sel_idx)}.npz")
        save_table(os.path.join(args.out_dir, files[-1]), table_of(cands, pre_idx[sel_idx], meta))
    files.append("scenario_table.meta.json")
    with open(os.path.join(args.out_dir, files[-1]), "w", encoding="utf-8") as f:
        json.dump(meta, f, ensure_ascii=False, indent=2)
    print("[scenario_table] done")
    print(f"  candidates: {n_cand}\n  preselect:  {len(pre_idx)}")
    if sel_idx is not None:
        print(f"  selected:   {len(sel_idx)}")
    print(f"  out_dir:    {args.out_dir}\n  files:")
    for name in files:
        print(f"    - {name}")
    return files


if __name__ == "__main__":
    main()
