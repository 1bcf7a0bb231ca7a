"""Generate tests/golden/scenario_golden.npz and tests/golden/scenario_pre20.npz: what the REFERENCE's scenario
scripts compute (omniisaacgymenvs/scripts/build_usv_scenario_table.py and teacher_filter_scenario_table.py).

Run only where the reference tree exists (make_golden.REF), on the CPU:
    python tests/golden/make_scenario_golden.py

build_usv_scenario_table.py needs only numpy and is loaded by file path; teacher_filter_scenario_table.py is
imported behind make_golden.install_stubs.  Their functions are CALLED (build_candidates, preselect_scenarios,
select_scenarios_from_pre, _compute_metrics, _save_npz, _save_subset_npz, _select_keep_indices); the per-scenario
aggregation of the filter is inline in its hydra main and cannot be imported, so aggregate() below restates it
(:712-759).  The fixtures hold arrays only.

  candidates   the 40 candidates of seed 0 at the reference defaults, preselect (20, ratio 1:3:1, seed + 1) and
               selected (10, seed + 2) with their summaries; scenario_pre20.npz is the preselect table as the
               reference writes it (object-dtype obstacles_hash), with a subset of it by _save_subset_npz
  metrics      _compute_metrics of the 40 candidates and 27 crafted scenarios (67: not a multiple of 4)
  fold         two synthetic evaluator tables for S = 7, R = 3, n = 8 (K = 3, three pad rows) with the aggregate
               rows and _select_keep_indices' output"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_golden import REF, install_stubs  # noqa: E402

from omniisaacgymenvs_loop_amd._abi import DEFINES  # noqa: E402

F = np.float32
SEED, N_CAND, N_PRE, N_SEL, RATIO = 0, 40, 20, 10, (1, 3, 1)
DEFAULTS = dict(big=16, goal_random_position=5.0, min_spawn_dist=0.5, max_spawn_dist=5.0, box_half_range=15.0,
                min_dist_safe=2.0, obstacle_radius=0.5, quant_m=0.05, max_iterations=20, init_vel_mode="zero")
FOLD = dict(S=7, R=3, n=8, K=3, collision_threshold=0.5, easy_steps_max=80, easy_margin_min=0.75, max_steps=200,
            n_keep=3, n_final=2)
REASONS = {"collision": DEFINES["USV_EV_REASON_COLLISION"], "out_of_bounds": DEFINES["USV_EV_REASON_OOB"],
           "goal_tolerance": DEFINES["USV_EV_REASON_GOAL"], "other": DEFINES["USV_EV_REASON_OTHER"],
           "mixed": DEFINES["USV_EV_REASON_MIXED"]}
VERDICTS = {"keep": DEFINES["USV_SCV_KEEP"], "hard": DEFINES["USV_SCV_HARD_REJECT"],
            "easy": DEFINES["USV_SCV_EASY_REJECT"], "incomplete": DEFINES["USV_SCV_INCOMPLETE"]}


def load_build():
    path = os.path.join(REF, "omniisaacgymenvs", "scripts", "build_usv_scenario_table.py")
    spec = importlib.util.spec_from_file_location("ref_build_usv_scenario_table", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_filter():
    install_stubs()
    tb = types.ModuleType("torch.utils.tensorboard")   # as make_eval_golden.load_reference
    tb.SummaryWriter = type("SummaryWriter", (), {"__init__": lambda self, *a, **k: None})
    sys.modules["torch.utils.tensorboard"] = tb
    import omniisaacgymenvs.scripts.teacher_filter_scenario_table as T
    return T


def scen_arrays(prefix, scen):
    out = {f"{prefix}_{k}": np.stack([getattr(s, k) for s in scen]) for k in (
        "obstacles_xy", "spawn_root_pos", "spawn_root_rot", "target_pos", "target_rot", "init_root_vel_xy")}
    out[f"{prefix}_scenario_id"] = np.array([s.scenario_id for s in scen], np.int64)
    out[f"{prefix}_obstacles_hash"] = np.array([s.obstacles_hash for s in scen], dtype="U40")
    for k in ("d_spawn", "d_goal", "d_corr", "d_oo", "density_score"):
        out[f"{prefix}_{k}"] = np.array([getattr(s, k) for s in scen], np.float64)   # the Python floats
    return out


def crafted():
    """27 scenarios (obstacles [27][16][2], spawn [27][2], goal [27][2]) for the metrics' branches."""
    rng = np.random.default_rng(20240607)
    obs = np.full((27, 16, 2), 999.0, F)
    spawn = np.tile(np.array([-3.0, 1.0], F), (27, 1))
    goal = np.tile(np.array([4.0, -2.0], F), (27, 1))
    # 0: all limbo
    obs[1, 5] = (2.5, 3.25)                                   # exactly one valid obstacle
    obs[2, 0], obs[2, 15] = (2.5, 3.25), (-7.0, 0.125)        # exactly two
    obs[3, :6] = rng.uniform(-10, 10, (6, 2)).astype(F)       # spawn == goal
    goal[3] = spawn[3]
    obs[4, 3] = (-9.0, 4.0)                                   # projection before the spawn (t < 0)
    obs[5, 3] = (9.5, -6.0)                                   # past the goal (t > 1)
    obs[6, 3] = (0.5, 1.5)                                    # inside the segment
    obs[7, :4] = [(100.0, 0.0), (1.0, 2.0), (0.0, -100.0), (-4.0, 6.0)]      # a coordinate of exactly +-100: limbo
    obs[8, :3] = [(-100.0, 3.0), (5.0, 100.0), (7.0, 7.0)]
    obs[9, :3] = [(99.99, 0.0), (-99.99, 99.99), (6.0, -3.0)]               # 99.99: valid
    for i in range(10, 27):                                   # 1 .. 16 valid obstacles at random slots
        k = 1 + (i - 10) % 16
        slots = rng.choice(16, size=k, replace=False)
        spawn[i] = rng.uniform(-5, 5, 2).astype(F)
        goal[i] = rng.uniform(-5, 5, 2).astype(F)
        obs[i, slots] = (goal[i] + rng.uniform(-15, 15, (k, 2))).astype(F)
    goal[20] = spawn[20]
    return obs, spawn, goal


def aggregate(rollouts, thr):
    """The filter's per-scenario aggregate (:712-759) of a list of (reason, steps, ep_return_raw, final_dist,
    min_obs_dist_episode) records; min_obs / margin per rollout as _rollout_one_episode keeps them (:463-467)."""
    reasons = [r[0] for r in rollouts]
    success_rate = float(np.mean([1.0 if r == "goal_tolerance" else 0.0 for r in reasons]))
    collision_rate = float(np.mean([1.0 if r == "collision" else 0.0 for r in reasons]))
    out_of_bounds_rate = float(np.mean([1.0 if r == "out_of_bounds" else 0.0 for r in reasons]))
    collision_any = 1 if any(r == "collision" for r in reasons) else 0
    out_of_bounds_any = 1 if any(r == "out_of_bounds" for r in reasons) else 0
    if collision_any:
        done_reason = "collision"
    elif out_of_bounds_any:
        done_reason = "out_of_bounds"
    elif success_rate >= 1.0 - 1e-9:
        done_reason = "goal_tolerance"
    elif success_rate > 0.0:
        done_reason = "mixed"
    else:
        done_reason = "other"
    mins = [float(r[4]) if np.isfinite(r[4]) else float("inf") for r in rollouts]
    margins = [float(r[4]) - float(thr) if np.isfinite(r[4]) else float("inf") for r in rollouts]
    return {"done_reason": done_reason, "success_rate": success_rate, "collision_rate": collision_rate,
            "out_of_bounds_rate": out_of_bounds_rate, "collision_any": collision_any,
            "out_of_bounds_any": out_of_bounds_any, "steps": int(np.mean([r[1] for r in rollouts])),
            "ep_return_raw": float(np.mean([r[2] for r in rollouts])),
            "final_dist_to_goal": float(np.mean([r[3] for r in rollouts])),
            "min_obs_dist_min": float(np.min(mins)), "min_margin_min": float(np.min(margins))}


def fold_case(T, name, scenarios, out):
    """One synthetic evaluator table: scenarios = per scenario a list of R records or None (a missing rollout)."""
    S, R, n, K = FOLD["S"], FOLD["R"], FOLD["n"], FOLD["K"]
    assert len(scenarios) == S and K == -(-S * R // n)
    rng = np.random.default_rng(5)
    table = rng.uniform(-50, 50, (DEFINES["USV_EV_ROWS"], K * n))   # unused columns and rows hold noise
    count = np.zeros(n, np.int32)

    def put(p, rec):
        col = (p % K) * n + p // K
        table[DEFINES["USV_EV_REASON"], col] = REASONS[rec[0]]
        table[DEFINES["USV_EV_LEN_STEPS"], col] = rec[1]
        table[DEFINES["USV_EV_RETURN"], col] = rec[2]
        table[DEFINES["USV_EV_DIST_TO_GOAL"], col] = rec[3]
        table[DEFINES["USV_EV_MIN_OBS_EP"], col] = float(F(rec[4]))
        return (rec[0], rec[1], rec[2], rec[3], float(F(rec[4])))

    kept = []
    for s, recs in enumerate(scenarios):
        kept.append([put(s * R + r, rec) for r, rec in enumerate(recs) if rec is not None])
    for p in range(S * R, K * n):   # pad rows: records that must not be folded
        put(p, ("collision", 3, -99.0, 77.0, 0.01))
    for e in range(n):   # an env's records are its first ep_count: a missing rollout ends its env's list
        have = [scenarios[p // R][p % R] is not None if p < S * R else True for p in range(e * K, e * K + K)]
        count[e] = have.index(False) if False in have else K
        assert all(not h for h in have[count[e]:]), "a missing rollout must be the last of its env"
    rows, agg, verdict, diff = [], [], [], []
    for s, recs in enumerate(kept):
        a = aggregate(recs, FOLD["collision_threshold"])
        a.update(scenario_id=s, source_preselect_id=s, max_steps=FOLD["max_steps"])
        agg.append(a)
        if len(recs) < R:
            verdict.append(VERDICTS["incomplete"])
        else:
            _, _, one = T._select_keep_indices([a], n_keep=1, n_final=1, easy_steps_max=FOLD["easy_steps_max"],
                                               easy_margin_min=FOLD["easy_margin_min"])
            verdict.append(VERDICTS["hard"] if one["n_hard_reject"] else VERDICTS["easy"] if one["n_easy_reject"]
                           else VERDICTS["keep"])
            rows.append(a)
        steps_n = float(a["steps"]) / max(1.0, float(FOLD["max_steps"]))
        diff.append(float(steps_n + 0.3 * float(np.clip((0.5 - a["min_margin_min"]) / 0.5, -2.0, 2.0))))
    keep_idx, final_idx, summary = T._select_keep_indices(
        rows, n_keep=FOLD["n_keep"], n_final=FOLD["n_final"], easy_steps_max=FOLD["easy_steps_max"],
        easy_margin_min=FOLD["easy_margin_min"])
    kept_diff = [diff[s] for s in range(S) if verdict[s] == VERDICTS["keep"]]
    assert len(set(kept_diff)) == len(kept_diff), "two kept scenarios tie in difficulty (np.argsort is not stable)"
    out[f"{name}_table"], out[f"{name}_ep_count"] = table, count
    out[f"{name}_present"] = np.array([len(r) for r in kept], np.int64)
    out[f"{name}_reason"] = np.array([REASONS[a["done_reason"]] for a in agg], np.int64)
    for k in ("collision_any", "out_of_bounds_any", "steps"):
        out[f"{name}_{k}"] = np.array([a[k] for a in agg], np.int64)
    for k in ("success_rate", "collision_rate", "out_of_bounds_rate", "ep_return_raw", "final_dist_to_goal",
              "min_obs_dist_min", "min_margin_min"):
        out[f"{name}_{k}"] = np.array([a[k] for a in agg], np.float64)
    out[f"{name}_verdict"] = np.array(verdict, np.int64)
    out[f"{name}_difficulty"] = np.array(diff, np.float64)
    out[f"{name}_keep_idx"], out[f"{name}_final_idx"] = keep_idx.astype(np.int64), final_idx.astype(np.int64)
    out[f"{name}_select_summary"] = np.array(json.dumps(summary))
    out[f"{name}_select_rows"] = np.array(json.dumps(rows))
    return {v: verdict.count(v) for v in set(verdict)}


def main():
    B = load_build()
    T = load_filter()
    out = {}
    # ---- candidates, preselect, selected -------------------------------------------------------------
    cands = B.build_candidates(n_candidates=N_CAND, seed=SEED, device="cpu", **DEFAULTS)
    pre, pre_src, pre_sum = B.preselect_scenarios(candidates=cands, n_preselect=N_PRE, ratio_sparse_mid_dense=RATIO,
                                                  seed=SEED + 1)
    sel, sel_sum = B.select_scenarios_from_pre(preselected=pre, n_selected=N_SEL, seed=SEED + 2)
    out.update(scen_arrays("cand", cands))
    out.update(scen_arrays("pre", pre))
    out.update(scen_arrays("sel", sel))
    out["pre_source_candidate_id"] = np.asarray(pre_src, np.int64)
    out["pre_summary"] = np.array(json.dumps(pre_sum))
    out["sel_summary"] = np.array(json.dumps(sel_sum))
    out["defaults"] = np.array(json.dumps(dict(DEFAULTS, seed=SEED, n_candidates=N_CAND, n_preselect=N_PRE,
                                               n_selected=N_SEL, ratio=list(RATIO))))
    meta = {"seed": SEED, "sampling": {k: v for k, v in DEFAULTS.items()},
            "selection": {"n_candidates": N_CAND, "n_preselect": N_PRE, "n_selected": N_SEL,
                          "ratio_sparse_mid_dense": list(RATIO)},
            "summary": {"preselect": pre_sum}}
    pre_path = os.path.join(HERE, "scenario_pre20.npz")
    B._save_npz(pre_path, pre, meta, extra_arrays={"source_candidate_id": pre_src})
    # a subset of it, as the filter writes it
    keep = np.array([3, 0, 7, 19], np.int64)
    extra = {"scenario_npz": "scenario_pre20.npz", "checkpoint": "full_0.pt", "n_rollouts": 1, "n_keep": 4}
    with tempfile.TemporaryDirectory() as tmp:
        sub_path = os.path.join(tmp, "sub.npz")
        T._save_subset_npz(T._load_scenario_npz(pre_path), keep, sub_path, reindex_scenario_id=True, extra_meta=extra)
        with np.load(sub_path, allow_pickle=True) as sub:
            for k in sub.files:
                v = sub[k]
                out[f"sub_{k}"] = np.array(v.tolist(), dtype="U40") if v.dtype == object else np.array(v)
    out["sub_keep_idx"], out["sub_extra_meta"] = keep, np.array(json.dumps(extra))
    # ---- metrics: the 40 candidates and 27 crafted scenarios -------------------------------------------
    c_obs, c_spawn, c_goal = crafted()
    m_obs = np.concatenate([out["cand_obstacles_xy"], c_obs]).astype(F)
    m_spawn = np.concatenate([out["cand_spawn_root_pos"][:, :2], c_spawn]).astype(F)
    m_goal = np.concatenate([out["cand_target_pos"][:, :2], c_goal]).astype(F)
    keys = ("d_spawn", "d_goal", "d_corr", "d_oo", "density_score")
    m = [B._compute_metrics(obstacles_xy=m_obs[i], spawn_xy=m_spawn[i], goal_xy=m_goal[i],
                            obstacle_radius=DEFAULTS["obstacle_radius"]) for i in range(m_obs.shape[0])]
    out["m_obstacles_xy"], out["m_spawn_xy"], out["m_goal_xy"] = m_obs, m_spawn, m_goal
    out["m_out"] = np.array([[q[k] for q in m] for k in keys], np.float64)   # the Python floats; float32 on save
    assert m_obs.shape[0] == 67 and np.isinf(out["m_out"][:, 40]).all() and np.isinf(out["m_out"][3, 41])
    for i in range(N_CAND):
        assert all(out["m_out"][j, i] == out[f"cand_{k}"][i] for j, k in enumerate(keys))
    # ---- fold -------------------------------------------------------------------------------------------
    g, c, o, x = "goal_tolerance", "collision", "out_of_bounds", "other"
    nx = float(np.nextafter(F(1.25), F(0)))   # margin just below easy_margin_min = 0.75 at threshold 0.5
    case_a = [
        [(g, 90, 10.5, 0.08, 0.9), (g, 100, 11.25, 0.09, 0.7), (g, 110, 9.0, 0.07, 1.1)],      # keep
        [(g, 60, 8.0, 0.05, 1.4), (c, 33, -4.0, 3.5, 0.31), (g, 70, 7.5, 0.06, 1.3)],          # collision
        [(g, 60, 8.0, 0.05, 1.4), (g, 61, 8.1, 0.04, 1.5), (o, 150, -2.0, 21.0, 2.5)],         # out of bounds
        [(g, 120, 6.0, 0.09, 0.8), (x, 200, 1.0, 2.5, 0.6), (g, 130, 5.5, 0.08, 0.9)],         # mixed: keep
        [(x, 200, 0.5, 1.5, 0.9), (x, 200, 0.25, 2.5, 1.0), (x, 200, 0.75, 3.5, 1.1)],         # other: hard reject
        [(g, 80, 12.0, 0.05, 1.5), (g, 80, 12.5, 0.06, 1.6), (g, 81, 12.25, 0.07, 1.7)],       # easy reject
        [(g, 95, 10.0, 0.05, 0.85), (g, 96, 10.1, 0.06, 0.95), None],                          # a missing rollout
    ]
    case_b = [
        [(g, 80, 1.0, 0.05, 1.25), (g, 80, 1.1, 0.05, 1.5), (g, 80, 1.2, 0.05, 2.0)],          # at both limits: easy
        [(g, 81, 1.0, 0.05, 1.4), (g, 81, 1.1, 0.05, 1.5), (g, 81, 1.2, 0.05, 2.0)],           # one step over: keep
        [(g, 80, 1.0, 0.05, nx), (g, 80, 1.1, 0.05, 1.5), (g, 80, 1.2, 0.05, 2.0)],            # margin just under: keep
        [(g, 79, 1.0, 0.05, 1.3), (g, 79, 1.1, 0.05, 1.5), (g, 79, 1.2, 0.05, 2.0)],           # under, over: easy
        [(g, 80, 1.0, 0.05, 2.0), (g, 80, 1.1, 0.05, 2.5), (g, 82, 1.2, 0.05, 3.0)],           # mean 80.67 -> 80: easy
        [(g, 200, 1.0, 0.09, 0.51), (g, 199, 1.1, 0.09, 0.6), (g, 198, 1.2, 0.09, 0.7)],       # tight and long: keep
        [(g, 120, 1.0, 0.05, np.inf), (g, 121, 1.1, 0.05, np.inf), (g, 122, 1.2, 0.05, np.inf)],   # no obstacle: keep
    ]
    va = fold_case(T, "fold_a", case_a, out)
    vb = fold_case(T, "fold_b", case_b, out)
    assert set(va) == set(VERDICTS.values()) and vb[VERDICTS["easy"]] == 3 and vb[VERDICTS["keep"]] == 4
    assert set(out["fold_a_reason"]) == set(REASONS.values())
    out["fold_params"] = np.array(json.dumps(FOLD))
    path = os.path.join(HERE, "scenario_golden.npz")
    np.savez_compressed(path, **out)
    for q in (path, pre_path):
        print(f"wrote {q} ({os.path.getsize(q)} bytes)")


if __name__ == "__main__":
    main()
