"""GoToXY / KeepXY / TrackXYVelocity restated in numpy float32, in our own words: the checker of
tests/test_tasks_cpu.py (against the reference's recorded episodes) and tests/test_tasks_gpu.py (against the
device's own states).

Everything is a pure function of what it is handed: the observed state, the target, the previous distance, the
goal counter, the just-reset flag and the step clock.  The comparisons that decide a done or a counter (distance
against the kill distance, distance / speed error against the tolerance) are formed in float32 in the order the
step forms them, so they can be held exactly; the transcendental terms go through float64.

cfg is the UsvCfg of tasks/usv_config.build_usv_cfg (the kernels' constant block).
"""
from __future__ import annotations

import numpy as np

F = np.float32
GO_TO_POSE, GO_TO_XY, KEEP_XY, TRACK_XY = 1, 3, 4, 5
PEN_DEADZONE, PEN_SUM, PEN_SUMSQ, PEN_NORM, PEN_EXPABS = 1, 2, 3, 4, 5
TASK_COLS = slice(3, 23)   # Core's 20-column task_data block of the observation row


def _f(x):
    return np.asarray(x, F)


def _exp(x):
    with np.errstate(over="ignore"):
        return np.exp(np.asarray(x, np.float64)).astype(F)


def _rng(hi, lo):
    return F(float(hi) - float(lo))


def observe(cfg, st, u=None):
    """The state the task is shown: st = dict(px, py, yaw, vx, vy, wz) after the integration, with update_state's
    uniform noise from the step draws u [n][8] (velocity 0..2, heading 3, position 4..5); u = None: no noise."""
    o = {k: _f(st[k]).copy() for k in ("px", "py", "yaw", "vx", "vy", "wz")}
    if u is not None:
        u = _f(u)
        if cfg.pos_noise_on:
            r = _rng(cfg.pos_noise_max, cfg.pos_noise_min)
            o["px"] = o["px"] + (u[:, 4] * r + F(cfg.pos_noise_min))
            o["py"] = o["py"] + (u[:, 5] * r + F(cfg.pos_noise_min))
        if cfg.vel_noise_on:
            r = _rng(cfg.vel_noise_max, cfg.vel_noise_min)
            for k, j in (("vx", 0), ("vy", 1), ("wz", 2)):
                o[k] = o[k] + (u[:, j] * r + F(cfg.vel_noise_min))
        if cfg.head_noise_on:
            o["yaw"] = o["yaw"] + (u[:, 3] * _rng(cfg.head_noise_max, cfg.head_noise_min) + F(cfg.head_noise_min))
    return o


def thrust_units(cfg, actions, bias=0.0, u=None):
    """(clamped command [n][2], command after bias / noise / clamp, unit thrust in [0, 1])."""
    cmd = np.clip(_f(actions), F(-cfg.clip_actions), F(cfg.clip_actions))
    t = cmd.copy()
    if bias != 0.0:
        t = t + F(bias)
    if cfg.act_noise_on and u is not None:
        t = t + (_f(u)[:, 6:8] * _rng(cfg.act_noise_max, cfg.act_noise_min) + F(cfg.act_noise_min))
    t = np.clip(t, F(-1), F(1))
    unit = F(0.5) * (t + F(1)) if cfg.affine_thrust else np.clip(t, F(0), F(1))
    return cmd, t, np.clip(unit, F(0), F(1))


def curriculum(cfg, clock, start, end):
    """Linear from the curriculum value to the task's between warmup and end of the (double) step clock."""
    if clock < cfg.cur_warmup:
        return start
    if clock > cfg.cur_end:
        return end
    r = (clock - cfg.cur_warmup) / (cfg.cur_end - cfg.cur_warmup)
    return r * (end - start) + start


def kill_distance(cfg, clock):
    """The distance kill of GoToXY / KeepXY at the clock after this step's metrics ((t + 1) / horizon)."""
    if cfg.curriculum_on:
        return F(curriculum(cfg, clock, cfg.cur_kill_dist, cfg.kill_dist_d))
    return F(cfg.kill_dist)


def _term(mode, x, coeff):
    x = _f(x)
    if mode == 0:
        return F(1) / (F(1) + x)
    if mode == 1:
        return F(1) / (F(1) + x * x)
    return _exp(-x.astype(np.float64) / float(F(coeff)))


def _pen(kind, k, x0, c, x):
    x = _f(x)
    if kind == PEN_DEADZONE:
        return -np.maximum(np.abs(x) - F(x0), F(0)) * F(k) + F(c)
    if kind == PEN_EXPABS:
        return (_exp(float(F(x0)) * np.abs(x).astype(np.float64)) - F(1)) * F(k) + F(c)
    raise ValueError(f"scalar penalty kind {kind}")


def penalties(cfg, o, cmd, unit, prev_wz, prev_asum, valid):
    """Penalties.compute_penalty: dict of the terms that are on and their sum.  valid = False on the first step
    ever (no previous state / actions: both differences are 0).  The action-variation input is sum(actions) -
    sum(previous actions) with nothing cleared at a reset; with penalties_use_thrust_u the reference compares its
    persistent thrust tensor with itself, so the input is 0."""
    n = len(o["wz"])
    out = {}
    pa = unit if cfg.pen_use_u else cmd
    tot = np.zeros(n, F)
    if cfg.pen_lin_kind == PEN_NORM:
        out["linear_vel_penalty"] = -np.sqrt(o["vx"] * o["vx"] + o["vy"] * o["vy"]) * F(cfg.pen_lin_k) + F(cfg.pen_lin_c)
        tot = tot + out["linear_vel_penalty"]
    if cfg.pen_ang_kind:
        out["angular_vel_penalty"] = _pen(cfg.pen_ang_kind, cfg.pen_ang_k, cfg.pen_ang_x0, cfg.pen_ang_c, o["wz"])
        tot = tot + out["angular_vel_penalty"]
    if cfg.pen_angv_kind:
        d = o["wz"] - (_f(prev_wz) if valid else o["wz"])
        out["angular_vel_variation_penalty"] = _pen(cfg.pen_angv_kind, cfg.pen_angv_k, cfg.pen_angv_x0,
                                                    cfg.pen_angv_c, d)
        tot = tot + out["angular_vel_variation_penalty"]
    if cfg.pen_en_kind == PEN_SUM:
        out["energy_penalty"] = -(pa[:, 0] + pa[:, 1]) * F(cfg.pen_en_k) + F(cfg.pen_en_c)
    elif cfg.pen_en_kind == PEN_SUMSQ:
        out["energy_penalty"] = -(pa[:, 0] * pa[:, 0] + pa[:, 1] * pa[:, 1]) * F(cfg.pen_en_k) + F(cfg.pen_en_c)
    if "energy_penalty" in out:
        tot = tot + out["energy_penalty"]
    asum = cmd[:, 0] + cmd[:, 1]
    if cfg.pen_actv_kind:
        d = np.zeros(n, F) if (cfg.pen_use_u or not valid) else asum - _f(prev_asum)
        out["action_variation_penalty"] = _pen(cfg.pen_actv_kind, cfg.pen_actv_k, cfg.pen_actv_x0, cfg.pen_actv_c, d)
        tot = tot + out["action_variation_penalty"]
    return out, tot, asum


def state_stats(o, t, unit):
    """update_state_statistics: the six per-step state statistics."""
    return {"normed_linear_vel": np.sqrt(o["vx"] * o["vx"] + o["vy"] * o["vy"]), "normed_angular_vel": np.abs(o["wz"]),
            "cmd_neg_rate": ((t[:, 0] < 0).astype(F) + (t[:, 1] < 0).astype(F)) / F(2),
            "u_mean": (unit[:, 0] + unit[:, 1]) / F(2),
            "u_low_rate": ((unit[:, 0] < F(0.05)).astype(F) + (unit[:, 1] < F(0.05)).astype(F)) / F(2),
            "u_sum": unit[:, 0] + unit[:, 1]}


def task_step(kind, cfg, o, tgt, prev_dist, goal_cnt, just_reset, clock, first=False):
    """One step of the task part.  o: observe()'s state; tgt [n][2] target position (velocity for TrackXYVelocity);
    prev_dist [n] the previous step's distance (GoToXY: never cleared); goal_cnt [n] int; just_reset [n] bool;
    clock: the double step clock after this step's metrics; first: the first step ever (no previous distance).
    Returns dict(cols [n][20], reward [n], goal_cnt, die [n] bool, dist [n] (the next prev_dist), sums {key: [n]})."""
    tgt = _f(tgt)
    n = len(o["px"])
    cols = np.zeros((n, 20), F)
    goal_cnt = np.asarray(goal_cnt, np.int32)
    ge = (lambda c: c >= cfg.kill_after_n) if kind in (GO_TO_XY, KEEP_XY) else (lambda c: c > cfg.kill_after_n)
    if kind == TRACK_XY:
        ex, ey = tgt[:, 0] - o["vx"], tgt[:, 1] - o["vy"]
        cols[:, 0], cols[:, 1] = ex, ey
        pos_d = np.sqrt(o["px"] * o["px"] + o["py"] * o["py"])
        vel_d = np.sqrt(ex * ex + ey * ey)
        ok = (vel_d < F(cfg.tk_tol[0])).astype(np.int32)
        cnt = goal_cnt * ok + ok
        rew = _term(cfg.tk_mode[0], vel_d, cfg.tk_coeff[0])
        return dict(cols=cols, reward=rew, goal_cnt=cnt, die=(pos_d > F(cfg.kill_dist)) | ge(cnt), dist=vel_d,
                    sums={"velocity_reward": rew, "velocity_error": vel_d})
    ex, ey = tgt[:, 0] - o["px"], tgt[:, 1] - o["py"]
    yaw = o["yaw"].astype(np.float64)
    theta = np.arctan2(np.sin(yaw).astype(F), np.cos(yaw).astype(F)).astype(F)
    beta = np.arctan2(ey, ex).astype(F)
    alpha = np.fmod((beta - theta) + F(np.pi), F(2 * np.pi)) - F(np.pi)
    dist = np.sqrt(ex * ex + ey * ey)
    cols[:, 0] = np.cos(alpha.astype(np.float64))
    cols[:, 1] = np.sin(alpha.astype(np.float64))
    cols[:, 2] = dist
    bdist = dist - F(cfg.kill_dist)
    bpen = -_exp(-bdist.astype(np.float64) / 0.25) * F(cfg.boundary_cost)
    if kind == KEEP_XY:
        cnt = goal_cnt.copy()                       # never incremented
        rew = _term(cfg.tk_mode[0], dist, cfg.tk_coeff[0])
        sums = {"position_reward": rew, "position_error": dist, "boundary_penalty": bpen, "boundary_dist": bdist}
    else:
        ok = (dist < F(cfg.position_tolerance)).astype(np.int32)
        cnt = goal_cnt * ok + ok
        prev = dist if first else _f(prev_dist)
        if cfg.reward_mode == 0:
            dr = F(cfg.position_scale) * (prev - dist)
        elif cfg.reward_mode == 1:
            dr = F(cfg.position_scale) * (prev * prev - dist * dist)
        else:
            k = float(F(cfg.exp_coeff))
            dr = F(cfg.position_scale) * (_exp(-dist.astype(np.float64) / k) - _exp(-prev.astype(np.float64) / k))
        dr = np.where(np.asarray(just_reset, bool), F(0), dr).astype(F)
        h = np.abs(alpha).astype(np.float64)
        ar = F(cfg.align_la1) * (_exp(float(F(cfg.align_la2)) * h ** 4) + _exp(float(F(cfg.align_la3)) * h ** 2))
        rew = ((dr + ar) + cnt.astype(F) * F(cfg.goal_reward)) + F(cfg.time_reward)
        sums = {"distance_reward": dr, "alignment_reward": ar, "position_error": dist, "boundary_penalty": bpen,
                "boundary_dist": bdist}
    return dict(cols=cols, reward=_f(rew), goal_cnt=cnt, die=(dist > kill_distance(cfg, clock)) | ge(cnt), dist=dist,
                sums=sums)


def dones(cfg, progress_after, die):
    """is_done: the time-out at max_episode_length - 1 overrides; fixed_horizon_eval keeps only the time-out."""
    tout = np.asarray(progress_after) >= cfg.max_episode_length - 1
    return (tout if cfg.fixed_horizon_eval else (tout | np.asarray(die, bool))).astype(np.int64), tout


class Episode:
    """The carried values of a run (previous distance, counter, penalty history, episode sums) around task_step:
    step() takes the post-integration state and returns (cols, reward, dones, goal_cnt, extras or None)."""

    def __init__(self, kind, cfg, n, names, horizon=16):
        self.kind, self.cfg, self.n, self.names = kind, cfg, n, list(names)
        self.prev_dist = np.zeros(n, F)
        self.goal_cnt = np.zeros(n, np.int32)
        self.progress = np.zeros(n, np.int64)
        self.prev_wz = np.zeros(n, F)
        self.prev_asum = np.zeros(n, F)
        self.sums = {k: np.zeros(n, F) for k in self.names}
        self.t = 0
        self.clock = 0.0
        self.inc = 1 / horizon
        self.cause = None

    def step(self, st, tgt, actions, reset_mask, bias=0.0, u=None):
        cfg, first = self.cfg, self.t == 0
        reset_mask = np.asarray(reset_mask, bool)
        extras = None
        if reset_mask.any():   # extras["episode"]: means of the resetting envs' sums, then the sums restart
            extras = np.array([self.sums[k][reset_mask].mean(dtype=F) / (F(1) if k in ("success", "collision")
                                                                          else F(cfg.max_episode_length))
                               for k in self.names], F)
            for k in self.names:
                self.sums[k][reset_mask] = 0
            self.goal_cnt[reset_mask] = 0
            self.progress[reset_mask] = 0
        self.clock += self.inc
        o = observe(cfg, st, u)
        cmd, t, unit = thrust_units(cfg, actions, bias, u)
        r = task_step(self.kind, cfg, o, tgt, self.prev_dist, self.goal_cnt, reset_mask, self.clock, first)
        pens, pen_tot, asum = penalties(cfg, o, cmd, unit, self.prev_wz, self.prev_asum, not first)
        self.progress += 1
        dn, tout = dones(cfg, self.progress, r["die"])
        self.cause = dict(timeout=tout, die=r["die"], counter=(r["goal_cnt"] >= cfg.kill_after_n)
                          if self.kind != TRACK_XY else (r["goal_cnt"] > cfg.kill_after_n))
        for k, v in {**r["sums"], **pens, **state_stats(o, t, unit)}.items():
            if k in self.sums:
                self.sums[k] = self.sums[k] + _f(v)
        self.prev_dist, self.goal_cnt = r["dist"], r["goal_cnt"]
        self.prev_wz, self.prev_asum = o["wz"], asum
        self.t += 1
        return r["cols"], _f(r["reward"] + pen_tot), dn, r["goal_cnt"], extras
