"""Candidate scenarios: two samplers of one law, the geometry metrics, and the geometry-only selections
(the reference's scripts/build_usv_scenario_table.py: sampling :153-209, metrics :215-258, build_candidates
:264-363, preselect_scenarios :366-450, select_scenarios_from_pre :453-515).

The law: target ~ U(+-goal_random_position)^2; spawn = r (cos t, sin t), r ~ U(min_spawn_dist, max_spawn_dist),
t ~ U(0, 2 pi); yaw ~ U(0, pi) as the quaternion (cos(yaw / 2), 0, 0, sin(yaw / 2)); 16 obstacles ~
U(target +- box_half_range)^2, each redrawn while closer than min_dist_safe to the spawn or the target, at most
max_iterations times, then sent to limbo (999, 999); init_vel_mode zero or rand (+-1.5).

  sampler="numpy"   consumes np.random.default_rng(seed) in the reference's call order and shapes (the
                    data-dependent size=(k, 2) redraws included): the reference's tables bit for bit.
  sampler="philox"  the device sampler (usv_scn_generate, csrc/usv_scenario.hip) with its metrics
                    (usv_scn_metrics); philox_host() restates it on the host from the same Philox words.  A draw is
                    keyed by (seed, candidate, iteration, site), so a redraw of one obstacle does not depend on
                    the other obstacles, and any range of candidates can be generated on its own.
Both map uniforms to values in double and round to float32 once."""
from __future__ import annotations

import math
import os
import sys
from dataclasses import asdict, dataclass
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np

from .._abi import DEFINES
from .table import BIG, LIMBO, hashes_of, make_table, obstacles_hash

F = np.float32
METRIC_KEYS = ("d_spawn", "d_goal", "d_corr", "d_oo", "density_score")
SITE_POSE, SITE_YAW, SITE_OBST = (DEFINES["USV_SCN_SITE_POSE"], DEFINES["USV_SCN_SITE_YAW"],
                                  DEFINES["USV_SCN_SITE_OBST"])
SC_OBST, SC_START, SC_YAW = DEFINES["USV_SC_OBST"], DEFINES["USV_SC_START"], DEFINES["USV_SC_YAW"]
SC_VEL, SC_GOAL, STRIDE = DEFINES["USV_SC_VEL"], DEFINES["USV_SC_GOAL"], DEFINES["USV_SCENE_STRIDE"]
DEVICE_CHUNK = 1 << 20   # candidates per usv_scn_generate call


@dataclass
class SamplingParams:
    """The reference's command-line defaults (:578-590)."""
    big: int = BIG
    goal_random_position: float = 5.0
    min_spawn_dist: float = 0.5
    max_spawn_dist: float = 5.0
    box_half_range: float = 15.0
    min_dist_safe: float = 2.0
    max_iterations: int = 20
    obstacle_radius: float = 0.5
    quant_m: float = 0.05
    init_vel_mode: str = "zero"

    def check(self) -> None:
        if int(self.big) != BIG:
            raise ValueError(f"big = {self.big}: the scene rows and the kernels hold {BIG} obstacles")
        if self.init_vel_mode not in ("zero", "rand"):
            raise ValueError(f"Unknown init_vel_mode: {self.init_vel_mode}")

    def meta(self) -> Dict[str, Any]:
        return asdict(self)


# ------------------------------------------------------------------------------------------------ metrics
def _norm(dx, dy):
    """np.linalg.norm of float32 2-vectors: float32 products, two-term sum and sqrt."""
    return np.sqrt(dx * dx + dy * dy)


def metrics_host(obstacles_xy, spawn_xy, goal_xy, obstacle_radius: float,
                 limbo_threshold: float = 100.0) -> Dict[str, np.ndarray]:
    """_compute_metrics (:215-258) of S scenarios at once, as float64 arrays holding what the reference's Python
    floats hold: float32 arithmetic in its order; the corridor and pair minima are Python floats (doubles) when
    the radius is subtracted, the spawn and goal minima numpy float32.  usv_scn_metrics gives their float32."""
    obs = np.asarray(obstacles_xy, F).reshape(-1, BIG, 2)
    s = np.asarray(spawn_xy, F).reshape(-1, 1, 2)
    g = np.asarray(goal_xy, F).reshape(-1, 1, 2)
    ox, oy = obs[..., 0], obs[..., 1]
    lim, inf = F(limbo_threshold), F(np.inf)
    valid = (np.abs(ox) < lim) & (np.abs(oy) < lim)
    with np.errstate(all="ignore"):
        apx, apy = ox - s[..., 0], oy - s[..., 1]
        d_s = np.where(valid, _norm(apx, apy), inf).min(1)
        d_g = np.where(valid, _norm(ox - g[..., 0], oy - g[..., 1]), inf).min(1)
        abx, aby = g[..., 0] - s[..., 0], g[..., 1] - s[..., 1]
        ab2 = abx * abx + aby * aby
        t = (apx * abx + apy * aby) / ab2
        t = np.where(t < F(0), F(0), np.where(t > F(1), F(1), t)).astype(F)
        prx, pry = s[..., 0] + t * abx, s[..., 1] + t * aby
        seg = np.where(ab2.astype(np.float64) <= 1e-12, _norm(apx, apy), _norm(ox - prx, oy - pry))
        d_c = np.where(valid, seg, inf).min(1)
        pair = _norm(ox[:, :, None] - ox[:, None, :], oy[:, :, None] - oy[:, None, :])
        both = valid[:, :, None] & valid[:, None, :] & np.triu(np.ones((BIG, BIG), bool), 1)[None]
        d_o = np.where(both, pair, inf).reshape(-1, BIG * BIG).min(1)
        out = {"d_spawn": (d_s - F(obstacle_radius)).astype(np.float64),
               "d_goal": (d_g - F(obstacle_radius)).astype(np.float64),
               "d_corr": d_c.astype(np.float64) - float(obstacle_radius),
               "d_oo": d_o.astype(np.float64) - 2.0 * float(obstacle_radius)}
    out["density_score"] = np.minimum(np.minimum(out["d_spawn"], out["d_goal"]), out["d_corr"])
    return out


def metrics_device(rows, obstacle_radius: float, limbo_threshold: float = 100.0):
    """usv_scn_metrics of [S][USV_SCENE_STRIDE] device rows: a [5][S] float32 device tensor (METRIC_KEYS order)."""
    import torch

    from .. import _capi
    s = int(rows.shape[0])
    out = torch.empty((DEFINES["USV_SCM_ROWS"], s), device=rows.device, dtype=torch.float32)
    _capi.call("usv_scn_metrics", _capi.ptr(rows), s, float(obstacle_radius), float(limbo_threshold), _capi.ptr(out),
               _capi.stream_ptr())
    return out


# ----------------------------------------------------------------------------------------------- samplers
def _cand(obs, spawn_xy, quat, target_xy, vel, params: SamplingParams, metrics=None, hashes=None) -> Dict[str, Any]:
    n = int(np.asarray(obs).shape[0])
    z = np.zeros((n, 1), F)
    c = {"obstacles_xy": np.asarray(obs, F).reshape(n, BIG, 2),
         "spawn_root_pos": np.concatenate([np.asarray(spawn_xy, F).reshape(n, 2), z], 1),
         "spawn_root_rot": np.asarray(quat, F).reshape(n, 4),
         "target_pos": np.concatenate([np.asarray(target_xy, F).reshape(n, 2), z], 1),
         "target_rot": np.tile(np.array([1.0, 0.0, 0.0, 0.0], F), (n, 1)),   # the task keeps the target orientation
         "init_root_vel_xy": np.asarray(vel, F).reshape(n, 2)}
    c["obstacles_hash"] = hashes if hashes is not None else hashes_of(c["obstacles_xy"], params.quant_m)
    c["metrics"] = metrics if metrics is not None else metrics_host(
        c["obstacles_xy"], c["spawn_root_pos"][:, :2], c["target_pos"][:, :2], params.obstacle_radius)
    return c


def _take_rows(c: Dict[str, Any], idx) -> Dict[str, Any]:
    idx = np.asarray(idx, np.int64)
    out = {k: v[idx] for k, v in c.items() if k != "metrics"}
    out["metrics"] = {k: v[idx] for k, v in c["metrics"].items()}
    return out


def sample_numpy(n_candidates: int, seed: int, params: SamplingParams) -> Dict[str, Any]:
    """build_candidates (:264-363): unique candidates (dedup by obstacles_hash) from np.random.default_rng(seed)."""
    params.check()
    p = params
    rng = np.random.default_rng(int(seed))
    seen, rows = set(), []
    attempts, max_attempts = 0, max(int(n_candidates) * 50, 1000)
    while len(rows) < int(n_candidates) and attempts < max_attempts:
        attempts += 1
        target = rng.uniform(low=-float(p.goal_random_position), high=float(p.goal_random_position), size=(2,)).astype(F)
        r = float(rng.uniform(low=float(p.min_spawn_dist), high=float(p.max_spawn_dist)))
        theta = float(rng.uniform(low=0.0, high=2.0 * math.pi))
        spawn = np.array([r * math.cos(theta), r * math.sin(theta)], dtype=F)
        yaw = float(rng.uniform(low=0.0, high=math.pi))
        quat = np.array([math.cos(yaw * 0.5), 0.0, 0.0, math.sin(yaw * 0.5)], dtype=F)
        lo, hi = target - float(p.box_half_range), target + float(p.box_half_range)
        obs = rng.uniform(low=lo, high=hi, size=(BIG, 2)).astype(F)

        def invalid():
            d_start = np.linalg.norm(obs - spawn[None, :], axis=1)
            d_target = np.linalg.norm(obs - target[None, :], axis=1)
            return (d_start < float(p.min_dist_safe)) | (d_target < float(p.min_dist_safe))

        for _ in range(int(p.max_iterations)):
            bad = invalid()
            if not bool(bad.any()):
                break
            obs[bad] = rng.uniform(low=lo, high=hi, size=(int(bad.sum()), 2)).astype(F)
        bad = invalid()
        if bool(bad.any()):
            obs[bad] = np.array([LIMBO, LIMBO], dtype=F)
        vel = (np.zeros(2, F) if p.init_vel_mode == "zero"
               else rng.uniform(low=-1.5, high=1.5, size=(2,)).astype(F))
        h = obstacles_hash(obs, p.quant_m)
        if h in seen:
            continue
        seen.add(h)
        rows.append((obs, spawn, quat, target, vel, h))
    if len(rows) < int(n_candidates):
        raise RuntimeError(f"Could only generate {len(rows)}/{n_candidates} unique scenarios after {attempts} attempts. "
                           "Try increasing max_attempts or loosening dedup/constraints.")
    cols = [np.stack([r[i] for r in rows]) for i in range(5)]
    return _cand(*cols, params, hashes=np.array([r[5] for r in rows], dtype="U40"))


def _philox():
    try:
        from oracle.ppo_oracle import philox4x32_10
    except ImportError:   # run from another directory: the oracle sits beside the package
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
        from oracle.ppo_oracle import philox4x32_10
    return philox4x32_10


def _uniform(words) -> np.ndarray:
    return np.asarray(words, np.uint32).astype(np.float64) * (1.0 / 4294967296.0)


def _value(lo, hi, u) -> np.ndarray:
    return (lo + (hi - lo) * u).astype(F)


def philox_host(first: int, count: int, seed: int, params: SamplingParams) -> Tuple[np.ndarray, np.ndarray]:
    """usv_scn_generate restated on the host: (rows [count][USV_SCENE_STRIDE], spawn_quat [count][4])."""
    params.check()
    p, philox = params, _philox()
    cand = np.uint64(first) + np.arange(count, dtype=np.uint64)
    c0, c1 = cand & np.uint64(0xFFFFFFFF), cand >> np.uint64(32)
    key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    w = philox((c0, c1, 0, SITE_POSE), key)
    g = float(p.goal_random_position)
    tx, ty = _value(-g, g, _uniform(w[0])), _value(-g, g, _uniform(w[1]))
    r = float(p.min_spawn_dist) + (float(p.max_spawn_dist) - float(p.min_spawn_dist)) * _uniform(w[2])
    th = (2.0 * math.pi) * _uniform(w[3])
    sx, sy = (r * np.cos(th)).astype(F), (r * np.sin(th)).astype(F)
    y = philox((c0, c1, 0, SITE_YAW), key)
    yaw = math.pi * _uniform(y[0])
    box, safe = F(p.box_half_range), F(p.min_dist_safe)
    mn = np.stack([tx - box, ty - box], 1).astype(np.float64)[:, None, :]   # [count][1][2]
    mx = np.stack([tx + box, ty + box], 1).astype(np.float64)[:, None, :]
    lanes = np.arange(BIG, dtype=np.uint64)[None, :]

    def draw(k: int) -> np.ndarray:
        ww = philox((c0[:, None], c1[:, None], k, np.uint64(SITE_OBST) + lanes), key)
        return _value(mn, mx, np.stack([_uniform(ww[0]), _uniform(ww[1])], 2))

    def invalid(o) -> np.ndarray:
        d_s = _norm(o[..., 0] - sx[:, None], o[..., 1] - sy[:, None])
        d_t = _norm(o[..., 0] - tx[:, None], o[..., 1] - ty[:, None])
        return (d_s < safe) | (d_t < safe)

    obs = draw(0)
    for k in range(1, int(p.max_iterations) + 1):
        bad = invalid(obs)
        if not bad.any():
            break
        obs = np.where(bad[..., None], draw(k), obs)
    obs = np.where(invalid(obs)[..., None], F(LIMBO), obs).astype(F)
    rows = np.zeros((count, STRIDE), F)
    rows[:, SC_OBST:SC_OBST + 2 * BIG] = obs.reshape(count, 2 * BIG)
    rows[:, SC_START], rows[:, SC_START + 1] = sx, sy
    rows[:, SC_YAW] = yaw.astype(F)
    if p.init_vel_mode == "rand":
        rows[:, SC_VEL], rows[:, SC_VEL + 1] = _value(-1.5, 1.5, _uniform(y[1])), _value(-1.5, 1.5, _uniform(y[2]))
    rows[:, SC_GOAL], rows[:, SC_GOAL + 1] = tx, ty
    quat = np.zeros((count, 4), F)
    quat[:, 0], quat[:, 3] = np.cos(yaw * 0.5).astype(F), np.sin(yaw * 0.5).astype(F)
    return rows, quat


def generate_device(first: int, count: int, seed: int, params: SamplingParams, device="cuda:0"):
    """usv_scn_generate: (rows [count][USV_SCENE_STRIDE], spawn_quat [count][4]) float32 device tensors."""
    import torch

    from .. import _capi
    params.check()
    p = params
    rows = torch.empty((count, STRIDE), device=device, dtype=torch.float32)
    quat = torch.empty((count, 4), device=device, dtype=torch.float32)
    with torch.cuda.device(rows.device):
        _capi.call("usv_scn_generate", int(seed), int(first), int(count), float(p.goal_random_position),
                   float(p.min_spawn_dist), float(p.max_spawn_dist), float(p.box_half_range), float(p.min_dist_safe),
                   int(p.max_iterations), 1 if p.init_vel_mode == "rand" else 0, _capi.ptr(rows), _capi.ptr(quat),
                   _capi.stream_ptr())
    return rows, quat


def rows_to_candidates(rows: np.ndarray, quat: np.ndarray, params: SamplingParams, metrics=None) -> Dict[str, Any]:
    rows = np.asarray(rows, F)
    n = rows.shape[0]
    return _cand(rows[:, SC_OBST:SC_OBST + 2 * BIG].reshape(n, BIG, 2), rows[:, SC_START:SC_START + 2], quat,
                 rows[:, SC_GOAL:SC_GOAL + 2], rows[:, SC_VEL:SC_VEL + 2], params, metrics=metrics)


def sample_philox(n_candidates: int, seed: int, params: SamplingParams, device="cuda:0") -> Dict[str, Any]:
    """Unique candidates from the device sampler with the device metrics; the rows kept are deduplicated on
    the host by their sha1, and further candidate indices are generated until n_candidates are unique."""
    n = int(n_candidates)
    parts, seen, have, first = [], set(), 0, 0
    max_attempts = max(n * 50, 1000)
    while have < n and first < max_attempts:
        count = min(max(n - have, 1), DEVICE_CHUNK)
        rows, quat = generate_device(first, count, seed, params, device)
        met = metrics_device(rows, params.obstacle_radius).cpu().numpy().astype(np.float64)
        c = rows_to_candidates(rows.cpu().numpy(), quat.cpu().numpy(), params,
                               metrics={k: met[i] for i, k in enumerate(METRIC_KEYS)})
        keep = []
        for i, h in enumerate(c["obstacles_hash"]):
            if h not in seen:
                seen.add(h)
                keep.append(i)
        parts.append(_take_rows(c, keep))
        have += len(keep)
        first += count
    if have < n:
        raise RuntimeError(f"Could only generate {have}/{n} unique scenarios after {first} candidates.")
    out = {k: np.concatenate([q[k] for q in parts]) for k in parts[0] if k != "metrics"}
    out["metrics"] = {k: np.concatenate([q["metrics"][k] for q in parts]) for k in METRIC_KEYS}
    return out


def build_candidates(n_candidates: int, seed: int, params: Optional[SamplingParams] = None, sampler: str = "numpy",
                     device="cuda:0") -> Dict[str, Any]:
    params = params or SamplingParams()
    if sampler == "numpy":
        return sample_numpy(n_candidates, seed, params)
    if sampler == "philox":
        return sample_philox(n_candidates, seed, params, device)
    raise ValueError(f"Unknown sampler: {sampler} (numpy | philox)")


# --------------------------------------------------------------------------------------------- selections
def _take(rng, pool: Sequence[int], k: int) -> list:
    if k <= 0:
        return []
    if len(pool) <= k:
        return list(pool)
    return [pool[int(i)] for i in rng.choice(len(pool), size=k, replace=False)]


def preselect(density_score, n_preselect: int, ratio_sparse_mid_dense=(1, 3, 1), seed: int = 1):
    """preselect_scenarios (:366-450) on the candidates' density scores (the Python floats of the metrics):
    (candidate indices in table order = source_candidate_id, summary).  seed is the reference's seed + 1."""
    rng = np.random.default_rng(int(seed))
    dens = [float(v) for v in np.asarray(density_score, np.float64)]
    scores = np.array(dens, dtype=F)
    q20, q80 = float(np.quantile(scores, 0.2)), float(np.quantile(scores, 0.8))
    ids = range(len(dens))
    sparse = [i for i in ids if dens[i] >= q80]
    dense = [i for i in ids if dens[i] <= q20]
    mid = [i for i in ids if q20 < dens[i] < q80]
    r0, r1, r2 = ratio_sparse_mid_dense
    rsum = max(r0 + r1 + r2, 1)
    k_sparse = int(round(n_preselect * (r0 / rsum)))
    k_mid = int(round(n_preselect * (r1 / rsum)))
    k_dense = int(round(n_preselect * (r2 / rsum)))
    pre = _take(rng, sparse, k_sparse) + _take(rng, mid, k_mid) + _take(rng, dense, k_dense)
    if len(pre) < n_preselect:   # rounding left it short: fill from the rest
        chosen = set(pre)
        pre += _take(rng, [i for i in ids if i not in chosen], n_preselect - len(pre))
    summary = {"n_candidates": len(dens), "n_preselect": len(pre), "density_score_quantiles": {"q20": q20, "q80": q80},
               "bin_counts": {"sparse": len(sparse), "mid": len(mid), "dense": len(dense)},
               "ratio_sparse_mid_dense": list(ratio_sparse_mid_dense)}
    return np.array(pre, dtype=np.int64), summary


def select_from_pre(density_score, n_selected: int, seed: int = 2):
    """select_scenarios_from_pre (:453-515) on the preselected scenarios' density scores: (indices into the
    preselected table, summary).  seed is the reference's seed + 2."""
    dens = [float(v) for v in np.asarray(density_score, np.float64)]
    if n_selected <= 0:
        raise ValueError("n_selected must be > 0")
    if n_selected > len(dens):
        raise ValueError(f"n_selected ({n_selected}) must be <= preselected ({len(dens)})")
    rng = np.random.default_rng(int(seed))
    scores = np.array(dens, dtype=F)
    q25, q75 = float(np.quantile(scores, 0.25)), float(np.quantile(scores, 0.75))
    preferred = [i for i in range(len(dens)) if q25 <= dens[i] <= q75]
    inpref = set(preferred)
    nonpreferred = [i for i in range(len(dens)) if i not in inpref]
    sel = _take(rng, preferred, min(n_selected, len(preferred)))
    if len(sel) < n_selected:
        sel += _take(rng, nonpreferred, n_selected - len(sel))
    summary = {"n_preselected": len(dens), "n_selected": len(sel), "pre_density_score_quantiles": {"q25": q25, "q75": q75}}
    return np.array(sel, dtype=np.int64), summary


def table_of(cands: Dict[str, Any], idx, meta: Dict[str, Any], extra=None) -> Dict[str, Any]:
    """The table of candidates idx, scenario_id re-assigned 0 .. len(idx) - 1."""
    c = _take_rows(cands, idx)
    return make_table(np.arange(len(c["obstacles_hash"]), dtype=np.int64), c["obstacles_xy"], c["spawn_root_pos"],
                      c["spawn_root_rot"], c["target_pos"], c["target_rot"], c["init_root_vel_xy"], c["metrics"], meta,
                      hashes=c["obstacles_hash"], extra=extra)
