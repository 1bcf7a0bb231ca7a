"""What the PPO optimiser-step tests share (test infrastructure only): a float64 restatement of one step of
trancate_gradients_and_step + torch.optim.Adam + AdaptiveScheduler (a2c_common.py:308-330, schedulers.py:26-32), the
fp32 numpy oracle's step on the same inputs (the model whose error sets the kernel's tolerance), the seeded gradient
and state families, the one-step cases and the scheduler sequence of the GPU suite, and source mutants of the
float64 step that the tolerance must reject.

One step.  The kernel (csrc/ppo.hip k_apply and its chained forms) maps (p, m, v, opt[slot], grad, kl) to
(p', m', v', opt[1 - slot]).  Every check feeds ref_step64 exactly the fp32 inputs the device held before the launch,
so nothing accumulates across steps.  The constants are the fp32-rounded ppo_cfg_t fields (OptCfg rounds on
construction): both sides then agree on what kl == 2 * kl_threshold means.

Measure and tolerance.  Per tensor max |x - x64| / max |x64| (p', m', v'), relative error for the scalars (next
learning rate, step count, kept KL, gradient norm).  The kernel may miss float64 by FACTOR (ppo_ref64's 8) times what
the fp32 oracle step (PO.clip_grad, PO.Adam.apply, PO.adaptive_lr) misses it by on the same inputs, and never by less
than 2 ulp of fp32 at the compared scale: the oracle can be exact on a case, and the kernel forms lr / bc1 in double
and rounds it once.  No tolerance comes from the kernel's output.
"""
from __future__ import annotations

import dataclasses
import functools
import inspect
import math

import numpy as np

from oracle import ppo_oracle as PO
from tests import ppo_ref64 as R

F = np.float32
NPARAM = PO.NPARAM
ULP2 = 2.0 * 2.0 ** -23          # 2 ulp of fp32, relative
G_CAP = 1e15                     # |g * grad_scale| <= G_CAP: g^2 stays finite in fp32
KEYS = ("p", "m", "v", "lr", "step", "kl", "norm")
YAML = dict(adam_b1=0.9, adam_b2=0.999, adam_eps=1e-8)
_FLOATS = ("grad_norm", "adam_b1", "adam_b2", "adam_eps", "weight_decay", "kl_threshold", "lr_min", "lr_max")


@dataclasses.dataclass(frozen=True)
class OptCfg:
    """The optimiser's fields of ppo_cfg_t, floats as the fp32 values the kernel reads."""
    truncate_grads: int = 1
    grad_norm: float = 1.0
    adam_b1: float = 0.9
    adam_b2: float = 0.999
    adam_eps: float = 1e-8
    weight_decay: float = 0.0
    lr_adaptive: int = 1
    kl_threshold: float = 0.016
    lr_min: float = 1e-6
    lr_max: float = 1e-2

    def __post_init__(self):
        for k in _FLOATS:
            object.__setattr__(self, k, float(F(getattr(self, k))))

    def fields(self) -> dict:
        return dataclasses.asdict(self)

    def apply_to(self, kcfg):
        """Write the fields into a ppo_cfg_t (ctypes) and check that it holds the same fp32 values."""
        for k, val in self.fields().items():
            setattr(kcfg, k, val)
            assert float(getattr(kcfg, k)) == val, k
        return kcfg

    def oracle(self) -> PO.PPOConfig:
        return PO.PPOConfig(grad_norm=self.grad_norm, truncate_grads=bool(self.truncate_grads),
                            kl_threshold=self.kl_threshold, b1=self.adam_b1, b2=self.adam_b2, eps=self.adam_eps)


# ------------------------------------------------------------------ the float64 reference
def ref_step64(cfg, p, m, v, g, kl, opt_in, grad_scale):
    """One optimiser step in float64: (p', m', v', opt_out = [next lr, step, kept kl, gradient norm]).
    g, kl: the (all-reduced) gradient sum and KL sum before the 1 / world scale; opt_in = [lr, steps taken, kl]."""
    p, m, v, g = (np.asarray(a, np.float64) for a in (p, m, v, g))
    lr, step0, kl_prev = float(opt_in[0]), float(opt_in[1]), float(opt_in[2])
    b1, b2, eps, wd = cfg.adam_b1, cfg.adam_b2, cfg.adam_eps, cfg.weight_decay
    # clip_grad_norm_ on the scaled gradient (a2c_common.py:309-326)
    gs = g * float(grad_scale)
    norm = math.sqrt(float(np.sum(gs * gs)))
    coef = min(cfg.grad_norm / (norm + 1e-6), 1.0) if cfg.truncate_grads else 1.0
    gc = gs * coef
    # AdaptiveScheduler.update: the rate it returns is the next step's
    kl = float(kl) * float(grad_scale)
    new_lr, kl_keep = lr, kl_prev
    if cfg.lr_adaptive:
        if kl > 2.0 * cfg.kl_threshold:
            new_lr = max(lr / 1.5, cfg.lr_min)
        if kl < 0.5 * cfg.kl_threshold:
            new_lr = min(lr * 1.5, cfg.lr_max)
        kl_keep = kl
    step_lr = lr
    # torch.optim.Adam, amsgrad off: L2 weight decay, lerp, denom = sqrt(v) / sqrt(bc2) + eps, step_size = lr / bc1
    step = step0 + 1.0
    gd = gc + wd * p
    m1 = m + (1.0 - b1) * (gd - m)
    v1 = v * b2 + (1.0 - b2) * gd * gd
    bc1 = np.float64(1.0) - np.float64(b1) ** step
    bc2 = np.float64(1.0) - np.float64(b2) ** step
    denom = np.sqrt(v1) / np.sqrt(bc2) + eps
    p1 = p - (step_lr / bc1) * (m1 / denom)
    return p1, m1, v1, np.array([new_lr, step, kl_keep, norm], np.float64)


def model_step32(cfg: OptCfg, p, m, v, g, kl, opt_in, grad_scale):
    """The same step by the fp32 numpy oracle (PO.clip_grad, PO.Adam.apply, PO.adaptive_lr), in k_apply's order:
    scale, clip, weight decay, Adam.  Returns fp32 (p', m', v', opt_out[4])."""
    p, m, v, g = (np.asarray(a, F) for a in (p, m, v, g))
    gs = (g * F(grad_scale)).astype(F)
    gc, total = PO.clip_grad(gs, cfg.grad_norm)
    if not cfg.truncate_grads:
        gc = gs
    if cfg.weight_decay != 0.0:
        gc = (gc + F(cfg.weight_decay) * p).astype(F)
    adam = PO.Adam(m.copy(), v.copy(), int(opt_in[1]))
    lr = float(opt_in[0])
    p1 = adam.apply(p, gc, lr, cfg.oracle())
    klv = float(F(kl) * F(grad_scale))
    new_lr, keep = lr, float(opt_in[2])
    if cfg.lr_adaptive:
        new_lr, keep = PO.adaptive_lr(lr, klv, cfg.kl_threshold, cfg.lr_min, cfg.lr_max), klv
    return p1, adam.m, adam.v, np.array([new_lr, adam.step, keep, total], np.float64).astype(F)


# ------------------------------------------------------------------ measure and tolerance
def errors(out, ref) -> dict:
    """KEYS -> error of out = (p', m', v', opt_out) against ref (float64): max |x - x64| / max |x64| per tensor,
    relative error per scalar (absolute where the reference is 0); a non-finite value counts as infinitely wrong."""
    e = {}
    for k, x, y in zip(KEYS[:3], out[:3], ref[:3]):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        assert np.isfinite(y).all(), k
        scale = float(np.abs(y).max())
        e[k] = float(np.abs(x - y).max() / (scale if scale > 0 else 1.0)) if np.isfinite(x).all() else math.inf
    for j, k in enumerate(KEYS[3:]):
        x, y = float(out[3][j]), float(ref[3][j])
        e[k] = abs(x - y) / (abs(y) if y != 0 else 1.0) if math.isfinite(x) else math.inf
    return e


def tolerances(model_err: dict) -> dict:
    return {k: max(R.FACTOR * model_err[k], ULP2) for k in KEYS}


def worst_ratio(err: dict, tol: dict) -> tuple:
    k = max(KEYS, key=lambda q: err[q] / tol[q])
    return k, err[k] / tol[k]


# ------------------------------------------------------------------ gradient and state families
# |g| per parameter block (x 10^U(-0.5, 0.5) per parameter): 1e-12 .. 1e3, one block all zeros
BLOCK_MAG = {"sigma": 1e-12, "W1": 1e-3, "b1": 1e-8, "W2": 1.0, "b2": 0.0, "Wv": 1e3, "bv": 1e-5, "Wmu": 1e-1,
             "bmu": 1e2}


def graded_gradient(seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    parts = {}
    for k, s in PO.SHAPES:
        mag = BLOCK_MAG[k] * 10.0 ** rng.uniform(-0.5, 0.5, s)
        parts[k] = (mag * rng.choice([-1.0, 1.0], s)).astype(F)
    return PO.flatten(parts)


def scaled_to_norm(g: np.ndarray, norm: float) -> np.ndarray:
    """g times one factor, so that its float64 norm is `norm` (up to the fp32 rounding of its elements)."""
    n0 = math.sqrt(float(np.sum(np.asarray(g, np.float64) ** 2)))
    return (np.asarray(g, np.float64) * (norm / n0)).astype(F)


def fresh_moments():
    return np.zeros(NPARAM, F), np.zeros(NPARAM, F)


def resumed_moments(seed: int, g: np.ndarray):
    """Moments of a run under way: v a millionth of g^2, about g^2 and a million times g^2 in equal shares (0.1 ..
    10 x 1e-6 where g is 0), m of the size of g with either sign."""
    rng = np.random.default_rng(seed)
    g2 = np.asarray(g, np.float64) ** 2
    v = g2 * 10.0 ** rng.choice([-6.0, 0.0, 6.0], NPARAM) * rng.uniform(0.5, 2.0, NPARAM)
    v = np.where(g2 == 0, 1e-6 * 10.0 ** rng.uniform(-1, 1, NPARAM), v)
    m = np.where(g2 == 0, 1e-3, np.abs(g)) * rng.uniform(-1.0, 1.0, NPARAM)
    return m.astype(F), v.astype(F)


def params(seed: int = 5) -> np.ndarray:
    return PO.flatten(R.stress_params(seed))


@dataclasses.dataclass
class StepCase:
    name: str
    cfg: OptCfg
    p: np.ndarray
    m: np.ndarray
    v: np.ndarray
    g: np.ndarray
    kl: float            # the fp32 value in grad[NPARAM]
    opt_in: np.ndarray   # [lr, steps taken, kl, norm] of the slot the step reads
    grad_scale: float = 1.0
    want_norm: float | None = None   # the regime: norm of g * grad_scale (asserted at rel 1e-6)
    want_clipped: bool | None = None

    def inputs(self):
        return self.p, self.m, self.v, self.g, self.kl, self.opt_in, self.grad_scale


def assert_step_case(c: StepCase):
    """The family conditions of a one-step case, on its inputs alone."""
    gs = np.asarray(c.g, np.float64) * c.grad_scale
    assert np.abs(gs).max() <= G_CAP, (c.name, np.abs(gs).max())
    assert np.isfinite((c.g * F(c.grad_scale)) ** 2).all(), c.name
    blocks = PO.unflatten(c.g)
    assert sum(1 for k, _ in PO.SHAPES if not blocks[k].any()) == 1, "one block of the gradient is all zeros"
    nz = np.abs(c.g[c.g != 0]).astype(np.float64)
    assert nz.max() / nz.min() > 1e12, "the gradient spans the blocks' magnitudes"
    norm = math.sqrt(float(np.sum(gs * gs)))
    if c.want_norm is not None:
        assert abs(norm / c.want_norm - 1.0) < 1e-6, (c.name, norm, c.want_norm)
    if c.want_clipped is not None:
        assert bool(c.cfg.truncate_grads and c.cfg.grad_norm / (norm + 1e-6) < 1.0) == c.want_clipped, c.name
    assert c.p.dtype == c.m.dtype == c.v.dtype == c.g.dtype == F and (c.v >= 0).all()


CONSTANTS = dict(adam_b1=0.8, adam_b2=0.99, adam_eps=1e-5, weight_decay=1e-2, kl_threshold=0.01, lr_min=2e-5,
                 lr_max=5e-3)
RESUME_STEPS = (9, 999, 99999)


@functools.lru_cache(maxsize=None)
def step_cases() -> tuple:
    """The one-step cases of the GPU suite (tests/test_ppo_opt_edges_gpu.py), built on the CPU."""
    p, g0 = params(), graded_gradient(21)
    zm, zv = fresh_moments()
    rm, rv = resumed_moments(22, g0)
    base = OptCfg()
    thr = base.kl_threshold
    opt = lambda lr, step: np.array([lr, step, 0.0, 0.0], F)
    out = []

    def add(name, cfg, g, resumed, opt_in, kl, scale=1.0, norm=None, clipped=None):
        m, v = (rm, rv) if resumed else (zm, zv)
        if resumed:   # the moments follow the gradient's scale, so that v << g^2, ~ g^2 and >> g^2 all stay present
            f = math.sqrt(float(np.sum(np.asarray(g, np.float64) ** 2)) / float(np.sum(np.asarray(g0, np.float64) ** 2)))
            m, v = (rm * F(f)).astype(F), (rv.astype(np.float64) * f * f).astype(F)
        out.append(StepCase(name, cfg, p, m, v, g, float(F(kl)), opt_in, scale, norm, clipped))

    # clip regimes, grad_norm = 1 (the yaml's): far below, either side of the threshold, far above
    for tag, norm, clipped in (("far_below", 1e-3, False), ("just_below", 1.0 - 1e-3, False),
                               ("just_above", 1.0 + 1e-3, True), ("far_above", 1e3, True)):
        for resumed in (False, True):
            add(f"clip_{tag}_{'resumed' if resumed else 'first'}", base, scaled_to_norm(g0, norm), resumed,
                opt(3e-4, 37 if resumed else 0), 3 * thr, norm=norm, clipped=clipped)
    # grad_norm = 1e-4 with a norm near 2e-4: the 1e-6 of the denominator is 5e-3 of it
    small = dataclasses.replace(base, grad_norm=1e-4)
    add("clip_gn1e-4_first", small, scaled_to_norm(g0, 2e-4), False, opt(3e-4, 0), thr, norm=2e-4, clipped=True)
    add("clip_gn1e-4_resumed", small, scaled_to_norm(g0, 2e-4), True, opt(3e-4, 37), thr, norm=2e-4, clipped=True)
    # truncate_grads = 0: no clipping, the norm still reported
    add("noclip_resumed", dataclasses.replace(base, truncate_grads=0), scaled_to_norm(g0, 1e3), True, opt(3e-4, 37),
        0.2 * thr, norm=1e3, clipped=False)
    # grad_scale on the all-reduced gradient: the norm is that of the scaled gradient (2 = clipped; unscaled 8)
    for scale in (1.0, 0.25):
        add(f"scale_{scale:g}", base, scaled_to_norm(g0, 2.0 / scale), True, opt(3e-4, 37), 3 * thr / scale, scale,
            norm=2.0, clipped=True)
    # step counts the host wrote (restore): bias corrections from step + 1
    for n in RESUME_STEPS:
        add(f"resume_{n}", base, scaled_to_norm(g0, 0.5), True, opt(1e-3, n), 3 * thr, norm=0.5, clipped=False)
    # non-yaml constants, first and resumed step, clipped
    const = dataclasses.replace(base, **CONSTANTS)
    add("constants_first", const, scaled_to_norm(g0, 3.0), False, opt(3e-4, 0), 3 * const.kl_threshold, norm=3.0,
        clipped=True)
    add("constants_resumed", const, scaled_to_norm(g0, 3.0), True, opt(3e-4, 37), 0.2 * const.kl_threshold, norm=3.0,
        clipped=True)
    for c in out:
        assert_step_case(c)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


# ------------------------------------------------------------------ the scheduler sequence
SCHED = dict(kl_threshold=0.01, lr_min=1e-5, lr_max=2e-3)   # non-yaml, so that floor and cap are 14 steps apart
SCHED_LR0 = 3e-4


def scheduler_plan(cfg: OptCfg):
    """[(kl as the fp32 the test writes into grad[NPARAM], what the rate must do)]: down to lr_min and held, up to
    lr_max and held, in band, exactly on either threshold (no change: the comparisons are strict), one float
    outside either threshold (a change) and one float inside (none)."""
    thr = F(cfg.kl_threshold)
    hi, lo = F(2) * thr, F(0.5) * thr
    # the thresholds as the kernel forms them, 2.0f * thr and 0.5f * thr, are exact in fp32 and equal the float64
    # products of the rounded field
    assert float(hi) == 2.0 * cfg.kl_threshold and float(lo) == 0.5 * cfg.kl_threshold
    up, dn = lambda x: np.nextafter(F(x), F(np.inf)), lambda x: np.nextafter(F(x), F(-np.inf))
    plan = [(F(10) * thr, "down")] * 12                     # 3e-4 / 1.5^9 < 1e-5: at the floor from step 9 on
    plan += [(F(0.1) * thr, "up")] * 17                     # 1e-5 x 1.5^14 > 2e-3: at the cap from step 14 on
    plan += [(F(10) * thr, "down")] * 3                     # off the cap: 2e-3 / 1.5^3
    plan += [(thr, "same"), (F(1.5) * thr, "same")]         # in band
    plan += [(hi, "same"), (lo, "same")]                    # exactly on a threshold
    plan += [(up(hi), "down"), (dn(hi), "same"), (dn(lo), "up"), (up(lo), "same")]
    for kl, _ in plan:
        assert kl.dtype == F and np.isfinite(kl)
    assert len(plan) >= 40
    return plan


def assert_rate_move(what: str, lr_in: float, lr_out: float, cfg: OptCfg):
    """The rate's move of one step, as the plan states it (lr_in, lr_out: either side's)."""
    if what == "same":
        assert lr_out == lr_in, (what, lr_in, lr_out)
    elif what == "down":
        assert lr_out < lr_in or lr_in == lr_out == cfg.lr_min, (what, lr_in, lr_out)
    else:
        assert lr_out > lr_in or lr_in == lr_out == cfg.lr_max, (what, lr_in, lr_out)


def scheduler_cases():
    """The scheduler sequence on the CPU: the state advances by the fp32 oracle step, each step is a StepCase
    (its opt_in the previous step's opt_out), as the GPU test sees them from the device's own state."""
    cfg = OptCfg(**SCHED)
    p, g = params(), scaled_to_norm(graded_gradient(21), 2.0)
    m, v = fresh_moments()
    opt = np.array([SCHED_LR0, 0.0, 0.0, 0.0], F)
    out = []
    for i, (kl, what) in enumerate(scheduler_plan(cfg)):
        c = StepCase(f"sched_{i:02d}_{what}", cfg, p, m, v, g, float(kl), opt.copy(), 1.0, 2.0, True)
        out.append((c, what))
        p, m, v, opt = model_step32(cfg, *c.inputs())
    return out


def assert_scheduler_coverage(lrs, cfg: OptCfg):
    """lrs: the rate before every step and after the last.  The floor and the cap are each reached and held."""
    lrs = [float(F(x)) for x in lrs]
    for bound in (cfg.lr_min, cfg.lr_max):
        held = max((sum(1 for _ in grp) for val, grp in _runs(lrs) if val == bound), default=0)
        assert held >= 3, (bound, lrs)


def _runs(xs):
    import itertools
    return ((val, list(grp)) for val, grp in itertools.groupby(xs))


# ------------------------------------------------------------------ mutants of the float64 step
_Y = {k: repr(float(F(val))) for k, val in YAML.items()}
_CONSTS = "b1, b2, eps, wd = cfg.adam_b1, cfg.adam_b2, cfg.adam_eps, cfg.weight_decay"
# name -> [(text, replacement)]: edits of ref_step64's source, each matching exactly once
MUTANTS = {
    "bias_correction_omitted": [("bc1 = np.float64(1.0) - np.float64(b1) ** step", "bc1 = np.float64(1.0)"),
                                ("bc2 = np.float64(1.0) - np.float64(b2) ** step", "bc2 = np.float64(1.0)")],
    "bias_correction_step_minus_1": [("np.float64(b1) ** step", "np.float64(b1) ** (step - 1.0)"),
                                     ("np.float64(b2) ** step", "np.float64(b2) ** (step - 1.0)")],
    "bc2_without_sqrt": [("/ np.sqrt(bc2) + eps", "/ bc2 + eps")],
    "eps_inside_sqrt": [("denom = np.sqrt(v1) / np.sqrt(bc2) + eps", "denom = np.sqrt(v1 / bc2 + eps)")],
    "decoupled_weight_decay": [("gd = gc + wd * p", "gd = gc"),
                               ("p1 = p - (step_lr", "p1 = p * (1.0 - step_lr * wd) - (step_lr")],
    "clip_eps_missing": [("(norm + 1e-6)", "(norm)")],
    "scale_after_norm": [("norm = math.sqrt(float(np.sum(gs * gs)))", "norm = math.sqrt(float(np.sum(g * g)))")],
    "new_rate_this_step": [("step_lr = lr", "step_lr = new_lr")],
    "ge_upper_threshold": [("if kl > 2.0 * cfg.kl_threshold", "if kl >= 2.0 * cfg.kl_threshold")],
    "le_lower_threshold": [("if kl < 0.5 * cfg.kl_threshold", "if kl <= 0.5 * cfg.kl_threshold")],
    "floor_missing": [("new_lr = max(lr / 1.5, cfg.lr_min)", "new_lr = lr / 1.5")],
    "cap_missing": [("new_lr = min(lr * 1.5, cfg.lr_max)", "new_lr = lr * 1.5")],
    "b1_hard_coded": [(_CONSTS, f"b1, b2, eps, wd = {_Y['adam_b1']}, cfg.adam_b2, cfg.adam_eps, cfg.weight_decay")],
    "b2_hard_coded": [(_CONSTS, f"b1, b2, eps, wd = cfg.adam_b1, {_Y['adam_b2']}, cfg.adam_eps, cfg.weight_decay")],
    "eps_hard_coded": [(_CONSTS, f"b1, b2, eps, wd = cfg.adam_b1, cfg.adam_b2, {_Y['adam_eps']}, cfg.weight_decay")],
}
# the cases a mutant is judged on where the issue names them (a prefix of the case name); the rest: every case
MUTANT_CASES = {"clip_eps_missing": "clip_gn1e-4"}


@functools.lru_cache(maxsize=None)
def mutant_step(name: str):
    src = inspect.getsource(ref_step64)
    for old, new in MUTANTS[name]:
        assert src.count(old) == 1, f"mutant {name}: ref_step64 no longer has {old!r}"
        src = src.replace(old, new)
    ns = {"np": np, "math": math}
    exec(compile(src, f"<ref_step64 mutant {name}>", "exec"), ns)
    fn = ns["ref_step64"]

    def run(*a):
        with np.errstate(all="ignore"):
            return fn(*a)
    return run
