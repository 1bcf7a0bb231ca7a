"""Generate tests/golden/eval_golden.npz: the per-episode evaluation records of the REFERENCE's play tool
(omniisaacgymenvs/scripts/rlgames_play_loopz.py) for three recorded trajectories.

Run only where the reference tree exists (make_golden.REF), after __graft_entry__.build():
    python tests/golden/make_eval_golden.py

The reference's _compute_step_metrics and _infer_done_reason are IMPORTED and called, one env and one step at a
time, on a SimpleNamespace stand-in task holding that env's current_state, _target_positions, xunlian_pos,
collision_threshold, _task_parameters and _goal_reached.  Its accumulation loop is inline in its hydra main and
cannot be imported, so episode_records() below restates that loop (play_loopz.py:1144-1321) with the numpy
installed here -- the float32 action delta norm and the float32 saturation comparison included.

Trajectories:
  A  episode_A.npz (64 steps x 16 envs);
  S  episode_S.npz with scenes_S.npz (spawn and goal from the scene rows);
  C  a synthetic set written into the fixture (70 envs x 24 steps) in which every branch of the record occurs.
The episode fixtures do not record the spawn positions, so those come from the project's CPU oracle replaying the
fixture's recorded reset draws (oracle/oracle.py; for S they are asserted equal to the scene rows) and are stored
as inputs (<name>_start_x / _start_y).  The fixture holds arrays only."""
from __future__ import annotations

import json
import math
import os
import sys
import types
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_golden import install_stubs  # noqa: E402

from tests import eval_restate as R  # noqa: E402

K = R.K_EPISODES
MARGIN = 1e-6   # every distance compared with a threshold stays at least this far from it


def load_reference():
    install_stubs()
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = type("SummaryWriter", (), {"__init__": lambda self, *a, **k: None})
    sys.modules["torch.utils.tensorboard"] = tb
    import omniisaacgymenvs.scripts.rlgames_play_loopz as P
    return P


def step_metrics(P, torch, px, py, yaw, gx, gy, obst, thr):
    """The reference's _compute_step_metrics on one env's state (float32 tensors, as the task holds them)."""
    f = torch.float32
    inner = SimpleNamespace(
        _target_positions=torch.tensor([[gx, gy]], dtype=f), xunlian_pos=torch.tensor(np.asarray(obst)[None], dtype=f),
        collision_threshold=thr["collision_threshold"],
        _task_parameters=SimpleNamespace(kill_dist=thr["kill_dist"], position_tolerance=thr["position_tolerance"]),
        _goal_reached=torch.zeros(1, dtype=torch.long))
    base = SimpleNamespace(task=inner, current_state={
        "position": torch.tensor([[px, py]], dtype=f),
        "orientation": torch.tensor([[math.cos(float(yaw)), math.sin(float(yaw))]], dtype=f),
        "linear_velocity": torch.zeros((1, 2), dtype=f), "angular_velocity": torch.zeros(1, dtype=f)})
    return P._compute_step_metrics(base)


def episode_records(P, torch, tr, thr, control_dt, action_scale=1.0):
    """The play loop (play_loopz.py:1144-1321) for every env of trajectory tr, each env on its own as the
    reference runs env 0; records in table order (episode-major), and the count of episodes past K per env."""
    T, n = tr["px"].shape
    keys = R.INT_KEYS + R.F32_KEYS + R.F64_KEYS
    recs, dropped, margins = {}, 0, []
    for e in range(n):
        k_done, running = 0, False
        for t in range(T):
            if tr["started"][t][e]:
                m0 = step_metrics(P, torch, tr["start_x"][t][e], tr["start_y"][t][e], 0.0, tr["start_gx"][t][e],
                                  tr["start_gy"][t][e], tr["obst"][t][e], thr)
                start_pos = (m0.get("pos_x"), m0.get("pos_y"))
                goal_pos = (m0.get("goal_x"), m0.get("goal_y"))
                prev_pos = start_pos
                path_length, ep_return_raw, step = 0.0, 0.0, 0
                prev_action0, action_delta_sum, action_delta_count, sat_count, sat_total = None, 0.0, 0, 0, 0
                min_ep, running = np.float32(np.inf), True
            if not running:
                continue
            action0 = np.asarray(tr["actions"][t][e], np.float32)
            if prev_action0 is not None:
                da = action0 - prev_action0
                nrm = np.linalg.norm(da)
                # the form the kernel and the tests restate: float32 products, sum and sqrt
                assert nrm.dtype == np.float32 and nrm == np.sqrt(da[0] * da[0] + da[1] * da[1])
                action_delta_sum += float(nrm)
                action_delta_count += 1
            prev_action0 = action0.copy()
            sat_total += int(action0.size)
            sat_count += int(np.sum(np.abs(action0) > (0.95 * float(action_scale))))
            ep_return_raw += float(np.float32(tr["rew"][t][e]))
            m = step_metrics(P, torch, tr["px"][t][e], tr["py"][t][e], tr["yaw"][t][e], tr["tgt_x"][t][e],
                             tr["tgt_y"][t][e], tr["obst"][t][e], thr)
            px, py = float(m["pos_x"]), float(m["pos_y"])
            dx, dy = float(px - float(prev_pos[0])), float(py - float(prev_pos[1]))
            path_length += float(math.sqrt(dx * dx + dy * dy))
            prev_pos = (px, py)
            step += 1
            min_ep = min(min_ep, np.float32(m["min_obs_dist"]))
            if not tr["done"][t][e]:
                continue
            m_end = m
            reason = P._infer_done_reason(m_end)
            collision = 1 if float(m_end.get("collision", 0.0)) > 0.5 else 0
            out_of_bounds = 1 if float(m_end.get("out_of_bounds", 0.0)) > 0.5 else 0
            success = 1 if reason == "goal_tolerance" else 0
            sx, sy, gx, gy = (float(v) for v in (*start_pos, *goal_pos))
            straight = float(math.sqrt((gx - sx) ** 2 + (gy - sy) ** 2))
            path_eff = straight / max(path_length, 1e-6)
            smooth = (action_delta_sum / max(action_delta_count, 1)) if action_delta_count > 0 else float("nan")
            sat_rate = float(sat_count) / float(sat_total)
            ttg = (float(step) * float(control_dt)) if success else float("nan")
            margins += [abs(m_end["min_obs_dist"] - thr["collision_threshold"]),
                        abs(m_end["dist_to_goal"] - thr["kill_dist"]),
                        abs(m_end["dist_to_goal"] - thr["position_tolerance"])]
            running = False
            if k_done < K:
                recs[(k_done, e)] = dict(
                    env=e, episode=k_done, success=success, done_reason=R.REASONS.index(reason),
                    episode_len_steps=step, collision=collision, out_of_bounds=out_of_bounds,
                    in_goal_tolerance=int(m_end["in_goal_tolerance"] > 0.5), scene_idx=int(tr["scene_last"][t][e]),
                    env_done_succ=int(tr["done_succ"][t][e]), env_done_coll=int(tr["done_coll"][t][e]),
                    action_delta_count=action_delta_count, action_saturation_count=sat_count,
                    start_x=sx, start_y=sy, goal_x=gx, goal_y=gy, end_x=px, end_y=py,
                    end_yaw=np.float32(tr["yaw"][t][e]), min_obs_dist_end=m_end["min_obs_dist"],
                    min_obs_dist_episode=min_ep, time_to_goal_sec=ttg, return_raw=ep_return_raw,
                    path_length=path_length, straight_line_dist=straight, path_efficiency=path_eff,
                    action_smoothness_mean=smooth, action_smoothness_sum=action_delta_sum,
                    action_saturation_rate=sat_rate, dist_to_goal=m_end["dist_to_goal"])
            else:
                dropped += 1
            k_done += 1
    assert min(margins) >= MARGIN, f"a compared distance is within {MARGIN} of its threshold: {min(margins)}"
    order = sorted(recs)
    out = {}
    for key in keys:
        dt = np.int32 if key in R.INT_KEYS else np.float32 if key in R.F32_KEYS else np.float64
        out[key] = np.array([recs[o][key] for o in order], dt)
    return out, dropped


def oracle_spawns(d, cfg_d):
    """[T][n] float32 spawn x, y of the envs reset at each step: the project's CPU oracle on the fixture's
    recorded reset draws and trigonometry (tests/test_oracle_golden.py _replay, post-physics mode)."""
    from oracle import oracle as O
    from omniisaacgymenvs_loop_amd.tasks.usv_config import build_usv_cfg, thruster_tables
    from tests.test_oracle_golden import scene_rows
    cfg = build_usv_cfg(cfg_d)
    cfg.inj_trig = 1
    T, n = d["px"].shape
    E = O.OracleEnv(cfg, n, O.make_lut(*thruster_tables(cfg_d)))
    E.set_grid_lin(d["grid_lin"])
    if "scene_last" in d:
        sr = cfg_d["env"]["scene_replay"]
        E.set_scenes(scene_rows(), int(sr["start_index"]), bool(sr["cycle"]))
    E.tgt_x[:], E.tgt_y[:] = d["init_tgt"][:, 0], d["init_tgt"][:, 1]
    nu = O.NU_RESET
    ru_all = d["reset_U"]
    if ru_all.shape[1] < nu:
        ru_all = np.concatenate([ru_all, np.zeros((ru_all.shape[0], nu - ru_all.shape[1]), ru_all.dtype)], 1)
    sx, sy, ru = np.zeros((T, n), np.float32), np.zeros((T, n), np.float32), 0
    for t in range(T):
        ids = E.compact()
        np.testing.assert_array_equal(ids, np.nonzero(d["reset_mask"][t])[0])
        if len(ids):
            E.reset(ids, ru_all[ru:ru + len(ids)])
            ru += len(ids)
            sx[t, ids], sy[t, ids] = E.px[ids], E.py[ids]
        E.step_pre(d["actions"][t], float(d["bias"][t]), d["u_step"][t])
        E.step_physics()
        for k in ("px", "py", "yaw", "vx", "vy", "wz", "fl", "fr"):
            getattr(E, k)[:] = d[k][t]
        E.step_post(d["u_step"][t])
        np.testing.assert_array_equal(E.reset_buf, d["reset"][t])
    return sx, sy


def synthetic(thr, seed=11, n=70, T=24):
    """Scripted episodes: env e plays the episode kinds of SCRIPTS[e % len] one after the other (a new one starts
    the step after an ending), then keeps going without ending.  Every kind fixes the END of its episode: the
    distance to the goal and to the nearest obstacle."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    ct, kd, tol = thr["collision_threshold"], thr["kill_dist"], thr["position_tolerance"]
    # kind -> (goal distance at the end, nearest obstacle distance at the end)
    KINDS = {"success": (0.5 * tol, ct + 2.0), "collision": (5.0, 0.6 * ct), "oob": (kd + 1.5, ct + 3.0),
             "other": (4.0, ct + 1.0), "coll_oob": (kd + 2.0, 0.5 * ct), "tol_coll": (0.4 * tol, 0.7 * ct)}
    SCRIPTS = [
        [("success", 6)], [("collision", 5), ("success", 4)], [("oob", 7)], [("other", 10)], [("coll_oob", 4)],
        [("tol_coll", 5)], [("other", 1), ("collision", 1), ("success", 3)], [("still", 6)], [("sat", 8)],
        [("collision", 3), ("other", 3), ("success", 3), ("oob", 3)], [],
        [("success", 2), ("success", 2), ("other", 9)], [("oob", 1), ("tol_coll", 2)],
    ]
    assert n >= 64 + 6 and n >= len(SCRIPTS)   # one full wave plus six lanes; every script played at least once
    sat_vals = [f32(0.95), np.nextafter(f32(0.95), f32(2)), np.nextafter(f32(0.95), f32(0))]
    tr = {"started": np.zeros((T, n), bool), "done": np.zeros((T, n), np.int32)}
    for k in ("start_x", "start_y", "start_gx", "start_gy", "px", "py", "yaw", "tgt_x", "tgt_y", "rew"):
        tr[k] = np.zeros((T, n), f32)
    tr["actions"] = rng.uniform(-1, 1, (T, n, 2)).astype(f32)
    tr["obst"] = np.zeros((T, n, 16, 2), f32)
    tr["rew"] = rng.normal(0, 1, (T, n)).astype(f32)
    tr["yaw"] = rng.uniform(-np.pi, np.pi, (T, n)).astype(f32)
    for k in ("scene_last", "done_succ", "done_coll"):
        tr[k] = np.zeros((T, n), np.int32)
    want = []   # (env, end step, kind) of every scripted ending
    for e in range(n):
        script = list(SCRIPTS[e % len(SCRIPTS)]) + [("free", T)]
        t, scene = 0, e
        for kind, L in script:
            if t >= T:
                break
            L = min(L, T - t)
            ends = kind != "free" and t + L <= T
            base = "other" if kind in ("still", "sat", "free") else kind
            d_goal, d_obs = KINDS[base]
            start = rng.uniform(-6, 6, 2)
            end = start if kind == "still" else start + rng.uniform(-3, 3, 2)
            pts = np.linspace(start, end, L + 1)[1:] + (0 if kind == "still" else rng.normal(0, 0.05, (L, 2)))
            pts = pts.astype(f32)
            ang = rng.uniform(0, 2 * np.pi)
            goal = (pts[-1].astype(np.float64) + d_goal * np.array([math.cos(ang), math.sin(ang)])).astype(f32)
            # obstacles: far from every point of the episode, except the nearest one at the scripted end distance
            obst = np.zeros((16, 2), f32)
            for o in range(16):
                while True:
                    c = rng.uniform(-25, 25, 2).astype(f32)
                    if np.sqrt(((pts.astype(np.float64) - c) ** 2).sum(1)).min() > max(d_obs, ct) + 1.0:
                        obst[o] = c
                        break
            ang = rng.uniform(0, 2 * np.pi)
            obst[int(rng.integers(16))] = (pts[-1].astype(np.float64)
                                           + d_obs * np.array([math.cos(ang), math.sin(ang)])).astype(f32)
            sl = slice(t, t + L)
            tr["started"][t, e] = True
            tr["start_x"][t, e], tr["start_y"][t, e] = f32(start[0]), f32(start[1])
            tr["start_gx"][t, e], tr["start_gy"][t, e] = goal
            tr["px"][sl, e], tr["py"][sl, e] = pts[:, 0], pts[:, 1]
            tr["tgt_x"][sl, e], tr["tgt_y"][sl, e] = goal
            tr["obst"][sl, e] = obst
            tr["scene_last"][sl, e] = scene
            if kind == "still":
                tr["px"][sl, e], tr["py"][sl, e] = f32(start[0]), f32(start[1])
            if kind == "sat":
                for j in range(L):
                    tr["actions"][t + j, e] = [sat_vals[j % 3], -sat_vals[(j + 1) % 3]]
            if ends:
                tr["done"][t + L - 1, e] = 1
                tr["done_succ"][t + L - 1, e] = int(base in ("success", "tol_coll"))
                tr["done_coll"][t + L - 1, e] = int(base in ("collision", "coll_oob", "tol_coll"))
                want.append((e, t + L - 1, kind, L))
            t += L
            scene += n
    return tr, want


def check_synthetic(tr, want, rec, dropped, thr):
    """Every branch occurs, and no scripted ending fell on the wrong side of a threshold."""
    n = tr["px"].shape[1]
    by = {(int(e), int(k)): i for i, (e, k) in enumerate(zip(rec["env"], rec["episode"]))}
    seen, per_env = set(), {}
    for e, t_end, kind, L in want:
        k = per_env.get(e, 0)
        per_env[e] = k + 1
        if k >= K:
            seen.add("dropped")
            continue
        i = by[(e, k)]
        reason = R.REASONS[rec["done_reason"][i]]
        exp = {"success": "goal_tolerance", "collision": "collision", "oob": "out_of_bounds", "other": "other",
               "coll_oob": "collision", "tol_coll": "collision", "still": "other", "sat": "other"}[kind]
        assert reason == exp and rec["episode_len_steps"][i] == L, (e, k, kind, reason)
        assert rec["success"][i] == (kind == "success")
        if kind == "coll_oob":
            assert rec["collision"][i] == 1 and rec["out_of_bounds"][i] == 1
        if kind == "tol_coll":
            assert rec["collision"][i] == 1 and rec["in_goal_tolerance"][i] == 1 and rec["success"][i] == 0
        if kind == "still":
            assert rec["path_length"][i] == 0.0
            assert rec["path_efficiency"][i] == rec["straight_line_dist"][i] / 1e-6
        if kind == "sat":   # per 3 steps: (0.95, -above), (above, -below), (below, -0.95): 2 of 6 saturate
            assert rec["action_saturation_count"][i] == sum(
                int(j % 3 == 1) + int((j + 1) % 3 == 1) for j in range(L))
        if L == 1:
            assert np.isnan(rec["action_smoothness_mean"][i]) and rec["action_delta_count"][i] == 0
            seen.add("one_step")
        if kind == "success":
            assert rec["time_to_goal_sec"][i] > 0
        else:
            assert np.isnan(rec["time_to_goal_sec"][i])
        seen.add(kind)
    assert seen >= {"success", "collision", "oob", "other", "coll_oob", "tol_coll", "still", "sat", "one_step",
                    "dropped"}, seen
    assert dropped == sum(max(v - K, 0) for v in per_env.values()) and dropped > 0
    assert max(per_env.values()) == 4 and len(per_env) < n   # an env with four endings, envs with none


def main():
    P = load_reference()
    import torch
    out = {}
    eg_inputs = {}
    for v in ("A", "S"):
        d = dict(np.load(os.path.join(HERE, f"episode_{v}.npz"), allow_pickle=False))
        cfg_d = json.loads(bytes(d["config_json"]).decode())
        if cfg_d["env"]["scene_replay"].get("enabled"):
            cfg_d["env"]["scene_replay"]["npz_path"] = os.path.join(HERE, "scenes_S.npz")
        sx, sy = oracle_spawns(d, cfg_d)
        if v == "S":   # the spawn is the scene row's start_pos, the goal its goal_pos
            sc = np.load(os.path.join(HERE, "scenes_S.npz"), allow_pickle=False)
            m = d["reset_mask"].astype(bool)
            idx = d["scene_last"][m]
            np.testing.assert_array_equal(np.stack([sx[m], sy[m]], 1), sc["start_pos"][idx].astype(np.float32))
            np.testing.assert_array_equal(d["tgt"][m], sc["goal_pos"][idx].astype(np.float32))
        eg_inputs[f"{v}_start_x"], eg_inputs[f"{v}_start_y"] = sx, sy
        tr, _, _ = R.fixture_traj(v, eg_inputs)
        tp = cfg_d["env"]["task_parameters"]
        thr = dict(collision_threshold=1.2, kill_dist=float(tp["kill_dist"]),
                   position_tolerance=float(tp["position_tolerance"]))
        control_dt = float(cfg_d["sim"]["dt"]) * float(max(int(cfg_d["env"]["controlFrequencyInv"]), 1))
        rec, dropped = episode_records(P, torch, tr, thr, control_dt)
        print(v, "endings", len(rec["env"]), "dropped", dropped,
              {r: int((rec["done_reason"] == i).sum()) for i, r in enumerate(R.REASONS)})
        out.update({f"{v}_rec_{k}": a for k, a in rec.items()})
        out[f"{v}_dropped"], out[f"{v}_control_dt"] = np.int64(dropped), np.float64(control_dt)
        if v == "A":
            thr_c, dt_c = thr, control_dt
    out.update(eg_inputs)
    tr, want = synthetic(thr_c)
    rec, dropped = episode_records(P, torch, tr, thr_c, dt_c)
    check_synthetic(tr, want, rec, dropped, thr_c)
    print("C endings", len(rec["env"]), "dropped", dropped,
          {r: int((rec["done_reason"] == i).sum()) for i, r in enumerate(R.REASONS)})
    out.update({f"C_in_{k}": tr[k] for k in R.TRAJ_KEYS})
    out.update({f"C_rec_{k}": a for k, a in rec.items()})
    out["C_dropped"], out["C_control_dt"] = np.int64(dropped), np.float64(dt_c)
    out["C_thresholds"] = np.array([thr_c["collision_threshold"], thr_c["kill_dist"], thr_c["position_tolerance"]])
    path = os.path.join(HERE, "eval_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
