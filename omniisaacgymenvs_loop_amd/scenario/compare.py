"""Teacher-vs-student comparison on a scenario table: the privileged-tail overrides of the reference's compare tool
(scripts/rlgames_play_loopz_compare.py, eval.priv_tail_mode = base_const_all / wrong_random) applied on the device
(usv_priv_tail), and the paired per-scenario fold of two arms' evaluator tables (usv_cmp_fold, csrc/usv_compare.hip).

Host restatements (pure numpy, no device): base_const_tail_host / wrong_random_tail_host compute the tails from a
parameter dict (tail_params) and given uniforms, in the reference's precisions: the fake mass, the coupling ratio
and the coupled scalars are Python floats (doubles) rounded once to float32; the CoM and the encoders are float32.

Pairing: every arm plays a fresh task with the same seed, n, table and R, so episode 0 of every env has the same
scene and the same reset draws in every arm (scenario.runner).  With K > 1 episodes per env the later episodes share
the scene only: compare() reports paired_draws = (K == 1) instead of refusing."""
from __future__ import annotations

import math
import time
from typing import Any, Callable, Dict, Mapping, Optional, Sequence

import numpy as np

from .._abi import DEFINES

F = np.float32
PT_CONST, PT_WRONG_RANDOM, PT_SITE = DEFINES["USV_PT_CONST"], DEFINES["USV_PT_WRONG_RANDOM"], DEFINES["USV_PT_SITE"]
CMP_ROWS = DEFINES["USV_CMP_ROWS"]
CMP_KEYS = {"pairs": "USV_CMP_PAIRS", "both_success": "USV_CMP_BOTH_SUCC", "only_a": "USV_CMP_ONLY_A",
            "only_b": "USV_CMP_ONLY_B", "neither": "USV_CMP_NEITHER", "collision_a": "USV_CMP_COLL_A",
            "collision_b": "USV_CMP_COLL_B", "out_of_bounds_a": "USV_CMP_OOB_A", "out_of_bounds_b": "USV_CMP_OOB_B",
            "d_steps": "USV_CMP_D_STEPS", "d_return": "USV_CMP_D_RETURN", "d_final_dist": "USV_CMP_D_FINAL_DIST",
            "d_min_margin": "USV_CMP_D_MIN_MARGIN"}
CMP_INT_KEYS = ("pairs", "both_success", "only_a", "only_b", "neither", "collision_a", "collision_b",
                "out_of_bounds_a", "out_of_bounds_b")
PRIV_MODES = ("raw", "centered", "minmax")
TAIL_MODES = {"base_const_all": PT_CONST, "wrong_random": PT_WRONG_RANDOM}


# ------------------------------------------------------------------ host restatements of the tails
def tail_params(cfg) -> Dict[str, Any]:
    """The parameter dict of the host restatements from a usv_cfg_t (tasks.usv_config): the float32 values the
    kernel reads, so the restatement fed usv_priv_tail's Philox words gives usv_priv_tail's bits."""
    return {"priv_dim": int(cfg.priv_dim), "priv_mode": PRIV_MODES[int(cfg.priv_mode)],
            "nominal": float(cfg.priv_nominal), "mass_relative": bool(cfg.mass_relative),
            "com_scaled": bool(cfg.com_scaled), "com_scale": [float(v) for v in cfg.com_scale],
            "com_mode": int(cfg.com_mode), "com_legacy_r": float(cfg.com_legacy_r),
            "base_com": [float(v) for v in cfg.base_com], "com_disp": [float(v) for v in cfg.com_disp],
            "min_mass": float(cfg.mass_min), "max_mass": float(cfg.mass_max), "base_mass": float(cfg.base_mass),
            "couple_drag": bool(cfg.couple_drag), "couple_thr": bool(cfg.couple_thr), "couple_kiz": bool(cfg.couple_kiz),
            "k_drag_min": float(cfg.kdrag_min), "k_drag_max": float(cfg.kdrag_max), "thr_rand": float(cfg.thr_rand),
            "thr_min": float(cfg.thr_min), "thr_max": float(cfg.thr_max),
            "k_iz_min": float(cfg.kiz_min), "k_iz_max": float(cfg.kiz_max)}


def _enc_centered(x, x_min: float, x_max: float, nominal: float):
    """USV_Virtual._encode_centered_priv_param on a float32 value: the scale is a double, the arithmetic float32."""
    scale = float(max(abs(float(x_min) - nominal), abs(float(x_max) - nominal), 1e-6))
    return np.clip((F(x) - F(nominal)) / F(scale), F(-1.0), F(1.0)).astype(F)


def _enc_minmax(x, x_min: float, x_max: float):
    """USV_Virtual._encode_minmax_priv_param: 0 for a degenerate range."""
    if (float(x_max) - float(x_min)) <= 1e-6:
        return np.zeros_like(np.asarray(x, F))
    z = (F(x) - F(x_min)) / F(float(x_max) - float(x_min))
    return np.clip(F(2.0) * z - F(1.0), F(-1.0), F(1.0)).astype(F)


def _thr_bounds(p: Mapping[str, Any]):
    a = float(p["thr_rand"])
    return (float(p.get("thr_min", 1.0 - a)), float(p.get("thr_max", 1.0 if p["couple_thr"] else 1.0 + a)))


def _encode_extras(p: Mapping[str, Any], k_drag, thr, k_iz) -> list:
    """The four extra columns (k_drag, thr_l, thr_r, k_iz) through the task's raw / centered / minmax encoder."""
    mode, (thr_min, thr_max) = str(p["priv_mode"]), _thr_bounds(p)
    if mode == "centered":
        nom = float(p["nominal"])
        kd = _enc_centered(k_drag, p["k_drag_min"], p["k_drag_max"], nom)
        th = _enc_centered(thr, thr_min, thr_max, nom)
        kz = _enc_centered(k_iz, p["k_iz_min"], p["k_iz_max"], nom)
    elif mode == "minmax":
        kd = _enc_minmax(k_drag, p["k_drag_min"], p["k_drag_max"])
        th = _enc_minmax(thr, thr_min, thr_max)
        kz = _enc_minmax(k_iz, p["k_iz_min"], p["k_iz_max"])
    else:
        kd, th, kz = F(k_drag), F(thr), F(k_iz)
    return [kd, th, th, kz]


def base_const_tail_host(p: Mapping[str, Any]) -> np.ndarray:
    """_compute_base_const_all_tail (:184-293): mass and CoM through get_base_masses' encodings (relative mass 0,
    CoM / (scale + 1e-6) in float32), the four extras the nominal 1.0 through the task's encoder."""
    mass = F(0.0) if p["mass_relative"] else F(p["base_mass"])
    com = np.asarray(p["base_com"], F)
    if p["com_scaled"]:
        com = (com / (np.asarray(p["com_scale"], F) + F(1e-6))).astype(F)
    tail = [mass, com[0], com[1], com[2]]
    if int(p["priv_dim"]) == 8:
        tail += _encode_extras(p, 1.0, 1.0, 1.0)
    return np.asarray(tail, F)


def wrong_random_tail_host(p: Mapping[str, Any], u_mass, u_com) -> np.ndarray:
    """_compute_wrong_random_tail (:296-507) from given uniforms in [0, 1): u_mass [...] draws the mass, u_com
    [...][3] the CoM (unused without com_displacement_xyz).  Returns [...][priv_dim] float32."""
    if int(p["com_mode"]) == 2 and float(p["com_legacy_r"]) > 0.0:
        raise NotImplementedError("wrong_random: the legacy disk CoM mode is not supported")
    u_mass = np.asarray(u_mass, np.float64)
    u_com = np.asarray(u_com, np.float64)
    lo, hi, base = float(p["min_mass"]), float(p["max_mass"]), float(p["base_mass"])
    if hi < lo:
        lo, hi = hi, lo
    m = lo + (hi - lo) * u_mass
    mass = ((m - base) / max(abs(base), 1e-6)).astype(F) if p["mass_relative"] else m.astype(F)
    com = np.broadcast_to(np.asarray(p["base_com"], F), u_mass.shape + (3,))
    if int(p["com_mode"]) == 1:
        com = com + (-1.0 + 2.0 * u_com).astype(F) * np.asarray(p["com_disp"], F)
    if p["com_scaled"]:   # the compare tool's divisor (the env step divides by scale + 1e-6)
        com = com / np.maximum(np.asarray(p["com_scale"], F), F(1e-6))
    cols = [mass, com[..., 0].astype(F), com[..., 1].astype(F), com[..., 2].astype(F)]
    if int(p["priv_dim"]) == 8:
        r = np.clip((m - base) / max(hi - base, 1e-6), 0.0, 1.0)
        one = np.ones_like(m)
        a = float(p["thr_rand"])
        kd = float(p["k_drag_min"]) + r * (float(p["k_drag_max"]) - float(p["k_drag_min"])) if p["couple_drag"] else one
        th = np.clip(1.0 - r * a, 1.0 - a, 1.0) if p["couple_thr"] else one
        kz = float(p["k_iz_min"]) + r * (float(p["k_iz_max"]) - float(p["k_iz_min"])) if p["couple_kiz"] else one
        cols += _encode_extras(p, kd.astype(F), th.astype(F), kz.astype(F))
    return np.stack([np.asarray(c, F) for c in cols], axis=-1)


def wrong_random_words(seed: int, n: int, episode) -> np.ndarray:
    """usv_priv_tail's Philox words as uniforms: [n][4] doubles (column 0 the mass, 1..3 the CoM)."""
    from .sampling import _philox, _uniform
    env = np.arange(n, dtype=np.uint64)
    ep = np.asarray(episode, np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    key = (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    w = _philox()((env, ep, 0, PT_SITE), key)
    return np.stack([_uniform(w[i]) for i in range(4)], 1)


def base_const_tail(task) -> np.ndarray:
    return base_const_tail_host(tail_params(task.cfg))


# ------------------------------------------------------------------ the override as a policy wrapper
class TailOverride:
    """policy(obs with the privileged tail replaced): mode "base_const_all" or "wrong_random".  evaluator: the
    EpisodeEvaluator of the run (its ep_count keys the wrong tail per episode); the sim never sees the override."""

    def __init__(self, policy: Callable, task, evaluator, mode: str, seed: int = 0):
        import torch
        if mode not in TAIL_MODES:
            raise ValueError(f"mode must be one of {sorted(TAIL_MODES)}, got {mode!r}")
        self.policy, self.task, self.evaluator = policy, task, evaluator
        self.mode, self.seed = TAIL_MODES[mode], int(seed) & 0xFFFFFFFFFFFFFFFF
        self.n, self.obs_dim = int(task.num_envs), int(task.num_observations)
        self.obs = torch.zeros((self.n, self.obs_dim), device=task.device, dtype=torch.float32)
        self.const_tail = torch.from_numpy(base_const_tail(task)).to(task.device) if self.mode == PT_CONST else None

    def reset(self) -> None:
        if hasattr(self.policy, "reset"):
            self.policy.reset()

    def override(self, obs):
        import torch
        from .. import _capi
        if obs.dtype != torch.float32 or not obs.is_contiguous():
            obs = obs.float().contiguous()
        _capi.call("usv_priv_tail", _capi.byref(self.task.cfg), self.mode, _capi.ptr(obs), _capi.ptr(self.obs), self.n,
                   self.obs_dim, _capi.ptr(self.const_tail), _capi.ptr(self.evaluator.ep_count), self.seed,
                   _capi.stream_ptr())
        return self.obs

    def __call__(self, obs):
        return self.policy(self.override(obs))


# ------------------------------------------------------------------ the paired fold
def pairing_info(n: int, S: int, R: int) -> Dict[str, Any]:
    """Episodes per env of the playlist and whether every pair shares its reset draws (K == 1)."""
    K = (int(S) * int(R) + int(n) - 1) // int(n)
    return {"episodes_per_env": K, "paired_draws": K == 1}


def cmp_to_dict(out: np.ndarray) -> Dict[str, np.ndarray]:
    """usv_cmp_fold's [USV_CMP_ROWS][S] doubles by name (counts as int64)."""
    d = {k: np.array(out[DEFINES[row]]) for k, row in CMP_KEYS.items()}
    for k in CMP_INT_KEYS:
        d[k] = d[k].astype(np.int64)
    return d


def cmp_totals(cmp: Mapping[str, np.ndarray]) -> Dict[str, Any]:
    """Totals over scenarios, summed in table order: the counts, the paired success difference (only_b - only_a)
    / pairs with its normal-approximation 95 % interval (per-pair differences are -1 / 0 / +1; population std, as
    eval.report), and the means of the differences (d_steps weighted by both_success, the others by pairs; a
    scenario whose value is NaN is left out)."""
    t: Dict[str, Any] = {k: int(sum(int(v) for v in cmp[k])) for k in CMP_INT_KEYS}
    N, a, b = t["pairs"], t["only_a"], t["only_b"]
    if N > 0:
        mean = (b - a) / N
        std = math.sqrt(max((a + b) / N - mean * mean, 0.0))
        half = 1.96 * std / math.sqrt(N)
    else:
        mean = std = half = float("nan")
    t["success_diff"] = {"count": N, "mean": mean, "std": std, "ci95_lo": mean - half, "ci95_hi": mean + half}
    for k, wk in (("d_steps", "both_success"), ("d_return", "pairs"), ("d_final_dist", "pairs"),
                  ("d_min_margin", "pairs")):
        num = den = 0.0
        for v, w in zip(cmp[k], cmp[wk]):
            if np.isfinite(v) and w > 0:
                num += float(v) * float(w)
                den += float(w)
        t[k] = num / den if den > 0 else float("nan")
    return t


def cmp_fold_device(ev_a, ev_b, n: int, S: int, R: int, K: int, collision_threshold: float, device) -> np.ndarray:
    """usv_cmp_fold of two UsvEval structs: [USV_CMP_ROWS][S] doubles on the host."""
    import torch
    from .. import _capi
    out = torch.zeros((CMP_ROWS, int(S)), device=device, dtype=torch.float64)
    _capi.call("usv_cmp_fold", _capi.byref(ev_a), _capi.byref(ev_b), int(n), int(S), int(R), int(K),
               float(collision_threshold), _capi.ptr(out), _capi.stream_ptr())
    return out.cpu().numpy()


class ArmTable:
    """An arm's evaluator table kept after its task is gone: clones of the table and the counts, and the usv_eval_t
    that points at them."""

    def __init__(self, evaluator):
        from .. import _capi
        from .._abi import UsvEval
        self.table, self.ep_count = evaluator.table.clone(), evaluator.ep_count.clone()
        ev = UsvEval()
        ev.acc, ev.episodes, ev.ep_count = None, _capi.ptr(self.table), _capi.ptr(self.ep_count)
        ev.max_episodes, ev.action_scale, ev.control_dt = (evaluator.max_episodes, evaluator.action_scale,
                                                           evaluator.control_dt)
        self.ev = ev


def compare(runner_factory: Callable[[], Any], arms: Mapping[str, Callable[[Any], Callable]],
            max_steps: Optional[int] = None, allow_incomplete: bool = False) -> Dict[str, Any]:
    """runner_factory() -> a ScenarioRunner on a fresh task (the same seed, n, table and R every time);
    arms: name -> make_policy(runner) -> policy callable, in order; the first arm is the baseline "a" of every
    pair.  Returns {"arms": {name: {"fold", "table", "steps", "wall_s"}}, "pairs": {name: {"scenarios", "totals"}}
    for every arm after the first, "baseline", "paired_draws", "episodes_per_env", "n", "S", "R"}."""
    import torch
    names = list(arms)
    if not names:
        raise ValueError("compare needs at least one arm")
    out: Dict[str, Any] = {"arms": {}, "pairs": {}, "baseline": names[0]}
    geo = None
    for name in names:
        runner = runner_factory()
        g = (runner.n, runner.S, runner.R, runner.K)
        if geo is None:
            geo = g
            out.update(pairing_info(runner.n, runner.S, runner.R), n=runner.n, S=runner.S, R=runner.R)
        elif g != geo:
            raise ValueError(f"arm {name}: runner geometry {g} differs from the first arm's {geo}")
        policy = arms[name](runner)
        if hasattr(policy, "reset"):
            policy.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fold = runner.run(policy, max_steps=max_steps, allow_incomplete=allow_incomplete)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        out["arms"][name] = {"fold": fold, "table": ArmTable(runner.evaluator), "steps": int(runner.steps_taken),
                             "wall_s": wall, "ms_per_step": 1e3 * wall / max(int(runner.steps_taken), 1)}
        thr, dev = runner.collision_threshold, runner.task.device
        del policy, runner
        if name != names[0]:
            n, S, R, K = geo
            cmp = cmp_to_dict(cmp_fold_device(out["arms"][names[0]]["table"].ev, out["arms"][name]["table"].ev, n, S, R,
                                              K, thr, dev))
            out["pairs"][name] = {"scenarios": cmp, "totals": cmp_totals(cmp)}
    return out


def arm_factories(names: Sequence[str], make_teacher: Callable[[Any], Callable],
                  make_student: Optional[Callable[[Any, bool], Callable]], seed: int = 0) -> Dict[str, Callable]:
    """The named arms of scripts/compare_policies.py: teacher, teacher_base_tail, teacher_wrong_tail, student,
    student_zero_latent.  make_teacher(runner) and make_student(runner, zero_latent) build the policies."""
    known = {
        "teacher": lambda r: make_teacher(r),
        "teacher_base_tail": lambda r: TailOverride(make_teacher(r), r.task, r.evaluator, "base_const_all", seed),
        "teacher_wrong_tail": lambda r: TailOverride(make_teacher(r), r.task, r.evaluator, "wrong_random", seed),
        "student": lambda r: make_student(r, False),
        "student_zero_latent": lambda r: make_student(r, True),
    }
    out = {}
    for nm in names:
        if nm not in known:
            raise ValueError(f"unknown arm {nm!r}; known: {sorted(known)}")
        if nm.startswith("student") and make_student is None:
            raise ValueError(f"arm {nm!r} needs id_encoder=<id_encoder_*.pth>")
        out[nm] = known[nm]
    return out
