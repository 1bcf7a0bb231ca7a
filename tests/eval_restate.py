"""Numpy restatement of the per-episode evaluation records (usv_eval_mark / usv_eval_step, include/usv_hip.h),
vectorised over the envs and stepped like the device: what tests/test_eval_cpu.py validates against the
reference-derived fixture (tests/golden/eval_golden.npz) and tests/test_eval_gpu.py then applies to device
read-backs.  Also the trajectory loaders and the record comparison both test files share.

A trajectory is a dict of [T][n] arrays:
  started (bool: the env was reset at the start of step t), start_x / start_y (float32 spawn, read where started),
  start_gx / start_gy (float32 goal after that reset), actions [T][n][2], and after step t: px, py, yaw, tgt_x,
  tgt_y, obst [T][n][16][2], rew (float32), done (the env's reset_buf), scene_last, done_succ, done_coll (int)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REASONS = ("collision", "out_of_bounds", "goal_tolerance", "other")
INT_KEYS = ("env", "episode", "success", "done_reason", "episode_len_steps", "collision", "out_of_bounds",
            "in_goal_tolerance", "scene_idx", "env_done_succ", "env_done_coll", "action_delta_count",
            "action_saturation_count")
F32_KEYS = ("start_x", "start_y", "goal_x", "goal_y", "end_x", "end_y", "end_yaw", "min_obs_dist_end",
            "min_obs_dist_episode")
F64_KEYS = ("time_to_goal_sec", "return_raw", "path_length", "straight_line_dist", "path_efficiency",
            "action_smoothness_mean", "action_smoothness_sum", "action_saturation_rate", "dist_to_goal")
START_KEYS = ("straight_line_dist", "path_length", "path_efficiency", "start_x", "start_y")
TRAJ_KEYS = ("started", "start_x", "start_y", "start_gx", "start_gy", "actions", "px", "py", "yaw", "tgt_x", "tgt_y",
             "obst", "rew", "done", "scene_last", "done_succ", "done_coll")
K_EPISODES = 3   # records kept per env in every fixture trajectory
ENV_FOUR_ENDINGS = 9   # the synthetic set's env with four endings (three kept, one dropped): the n = 1 case


def thresholds(cfg):
    """The three thresholds as the device compares them: the float32 config values, widened."""
    return dict(collision_threshold=float(np.float32(cfg.collision_threshold)),
                kill_dist=float(np.float32(cfg.kill_dist)),
                position_tolerance=float(np.float32(cfg.position_tolerance)))


def restate(tr, thr, K, control_dt, action_scale=1.0):
    """(episodes dict ordered by table column k * n + e, dropped count) of trajectory tr."""
    T, n = tr["px"].shape
    f64, f32 = np.float64, np.float32
    sx, sy, g0x, g0y = (np.zeros(n, f64) for _ in range(4))
    prev_x, prev_y, dsum, ret, path = (np.zeros(n, f64) for _ in range(5))
    prev_a = np.zeros((n, 2), f32)
    has_prev = np.zeros(n, bool)
    dcount, sat, steps, count = (np.zeros(n, np.int64) for _ in range(4))
    min_ep = np.zeros(n, f32)
    tab = {k: np.zeros(K * n, np.int32) for k in INT_KEYS}
    tab.update({k: np.zeros(K * n, f32) for k in F32_KEYS})
    tab.update({k: np.zeros(K * n, f64) for k in F64_KEYS})
    sat_thr = f32(0.95 * float(action_scale))
    for t in range(T):
        st = np.asarray(tr["started"][t], bool)
        sx[st], sy[st] = tr["start_x"][t][st], tr["start_y"][t][st]
        g0x[st], g0y[st] = tr["start_gx"][t][st], tr["start_gy"][t][st]
        prev_x[st], prev_y[st] = sx[st], sy[st]
        has_prev[st] = False
        for arr in (dsum, ret, path, dcount, sat, steps):
            arr[st] = 0
        min_ep[st] = np.inf
        a = np.asarray(tr["actions"][t], f32)
        da = a - prev_a
        nrm = np.sqrt(da[:, 0] * da[:, 0] + da[:, 1] * da[:, 1])
        assert nrm.dtype == f32
        dsum = dsum + np.where(has_prev, nrm.astype(f64), 0.0)
        dcount = dcount + has_prev
        prev_a, has_prev = a.copy(), np.ones(n, bool)
        sat = sat + (np.abs(a) > sat_thr).sum(1)
        ret = ret + np.asarray(tr["rew"][t], f32).astype(f64)
        pxf, pyf = np.asarray(tr["px"][t], f32), np.asarray(tr["py"][t], f32)
        px, py = pxf.astype(f64), pyf.astype(f64)
        ddx, ddy = px - prev_x, py - prev_y
        path = path + np.sqrt(ddx * ddx + ddy * ddy)
        prev_x, prev_y = px, py
        steps = steps + 1
        ob = np.asarray(tr["obst"][t], f32)
        ox, oy = ob[:, :, 0] - pxf[:, None], ob[:, :, 1] - pyf[:, None]
        d_ob = np.sqrt(ox * ox + oy * oy)
        assert d_ob.dtype == f32
        min_obs = d_ob.min(1)
        min_ep = np.minimum(min_ep, min_obs)
        done = np.asarray(tr["done"][t]) != 0
        ids = np.nonzero(done)[0]
        k = count[ids]
        count[ids] += 1
        ids = ids[k < K]
        col = k[k < K] * n + ids
        gdx = np.asarray(tr["tgt_x"][t], f32).astype(f64) - px
        gdy = np.asarray(tr["tgt_y"][t], f32).astype(f64) - py
        dist = np.sqrt(gdx * gdx + gdy * gdy)
        coll = min_obs.astype(f64) < thr["collision_threshold"]
        oob = dist > thr["kill_dist"]
        tol = dist < thr["position_tolerance"]
        reason = np.where(coll, 0, np.where(oob, 1, np.where(tol, 2, 3)))
        ex, ey = g0x - sx, g0y - sy
        straight = np.sqrt(ex * ex + ey * ey)
        with np.errstate(invalid="ignore", divide="ignore"):
            rec = {
                "env": np.arange(n), "episode": count - 1, "success": reason == 2, "done_reason": reason,
                "episode_len_steps": steps, "collision": coll, "out_of_bounds": oob, "in_goal_tolerance": tol,
                "scene_idx": tr["scene_last"][t], "env_done_succ": tr["done_succ"][t],
                "env_done_coll": tr["done_coll"][t], "action_delta_count": dcount, "action_saturation_count": sat,
                "start_x": sx, "start_y": sy, "goal_x": g0x, "goal_y": g0y, "end_x": pxf, "end_y": pyf,
                "end_yaw": tr["yaw"][t], "min_obs_dist_end": min_obs, "min_obs_dist_episode": min_ep,
                "time_to_goal_sec": np.where(reason == 2, steps * control_dt, np.nan), "return_raw": ret,
                "path_length": path, "straight_line_dist": straight,
                "path_efficiency": straight / np.maximum(path, 1e-6),
                "action_smoothness_mean": np.where(dcount > 0, dsum / np.maximum(dcount, 1), np.nan),
                "action_smoothness_sum": dsum, "action_saturation_rate": sat / (2.0 * steps),
                "dist_to_goal": dist,
            }
        for key, v in rec.items():
            tab[key][col] = np.asarray(v)[ids]
    kk, ee = np.divmod(np.arange(K * n), n)
    keep = kk < np.minimum(count, K)[ee]
    return {k: v[keep] for k, v in tab.items()}, int(np.maximum(count - K, 0).sum())


def fixture_traj(variant, eg):
    """Trajectory of episode_<variant>.npz (A or S) with the fixture's reset-time inputs (eval_golden.npz: the
    spawns, which the episode fixtures do not record); also returns the episode fixture and its config."""
    d = dict(np.load(os.path.join(GOLDEN, f"episode_{variant}.npz"), allow_pickle=False))
    cfg_d = json.loads(bytes(d["config_json"]).decode())
    T, n = d["px"].shape
    tr = {"started": d["reset_mask"].astype(bool), "start_x": eg[f"{variant}_start_x"],
          "start_y": eg[f"{variant}_start_y"], "start_gx": d["tgt"][:, :, 0], "start_gy": d["tgt"][:, :, 1],
          "actions": d["actions"], "px": d["px"], "py": d["py"], "yaw": d["yaw"], "tgt_x": d["tgt"][:, :, 0],
          "tgt_y": d["tgt"][:, :, 1], "obst": d["obst"], "rew": d["rew"], "done": d["reset"],
          "scene_last": d["scene_last"] if "scene_last" in d else np.full((T, n), -1, np.int32),
          # the env's own flags are not in the episode fixtures: the GPU test reads them back from the device
          "done_succ": np.zeros((T, n), np.int32), "done_coll": np.zeros((T, n), np.int32)}
    return tr, d, cfg_d


def synthetic_traj(eg):
    return {k: eg[f"C_in_{k}"] for k in TRAJ_KEYS}


def golden_records(eg, name):
    return {k: eg[f"{name}_rec_{k}"] for k in INT_KEYS + F32_KEYS + F64_KEYS}


def select_env(tr, e):
    """The one-env trajectory of env e (n = 1)."""
    return {k: np.ascontiguousarray(v[:, e:e + 1]) for k, v in tr.items()}


def assert_records(got, want, skip=(), msg=""):
    """Integers, flags and float32 fields exactly; doubles at rtol = 1e-12 (NaN where NaN)."""
    for k in INT_KEYS + F32_KEYS + F64_KEYS:
        if k in skip:
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, f"{msg} {k}: {g.shape} records, want {w.shape}"
        if k in F64_KEYS:
            np.testing.assert_allclose(g.astype(np.float64), w.astype(np.float64), rtol=1e-12, atol=0,
                                       equal_nan=True, err_msg=f"{msg} {k}")
        elif k in F32_KEYS:
            np.testing.assert_array_equal(g.astype(np.float32), w.astype(np.float32), err_msg=f"{msg} {k}")
        else:
            np.testing.assert_array_equal(g.astype(np.int64), w.astype(np.int64), err_msg=f"{msg} {k}")
