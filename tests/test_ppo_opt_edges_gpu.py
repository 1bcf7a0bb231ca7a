"""The PPO optimiser step on the device (csrc/ppo.hip: k_apply, the speculative Adam step of k_reduce_partials, redo_step,
clip_coef, adam_consts_tagged, opt_next, opt_store) against one float64 step (tests/ppo_opt_ref64.py) where it can go
wrong unseen: gradients from 1e-12 to 1e3 with a zero block, fresh and resumed moments, every clip regime, grad_scale
on the all-reduced path, the norm from the reduction's chunk squares, step counts and rates the host wrote under
stale cached constants, the KL thresholds to the float, the rate's floor and cap, non-yaml constants, weight decay,
both optimiser slots -- and the chained update (ppo_minibatch_fused / ppo_minibatch_finish) bit for bit against the
split path under the same configurations, which carries the float64 coverage over to the chain.

Every float64 check is one step from the device's own state: p, m, v, the optimiser slot, the gradient and the KL are
read back before the launch and the reference steps exactly those fp32 values.  Tolerance per figure: FACTOR (8) x the
error of the fp32 numpy oracle step on the same inputs, at least 2 ulp -- computed on the CPU, none taken from the
kernel.  tests/test_ppo_opt_ref64_cpu.py shows that fifteen wrong steps exceed four times this tolerance on these cases.
The params, m, v, grad and kl_out buffers are followed by 1,024 sentinel floats each, compared bit for bit after every
launch; PPO_NPARAM = 21253 leaves 5 parameters to the last workgroup and one float behind the norm's float4 loop."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import ppo_oracle as PO
from tests import errtab as ET
from tests import ppo_opt_ref64 as O
from tests import ppo_ref64 as R
from tests import test_ppo_gpu as TG
from tests.test_ppo_w2_image_gpu import HS, IMAGE, NH, OFF_W2, _fill

pytestmark = pytest.mark.gpu
F = np.float32
NP = PO.NPARAM
SENT = -7.25
PAD = 1024
SENT_BITS = int(F(SENT).view(np.int32))
ONE_STEP = {c.name: c for c in O.step_cases()}


def _dev():
    return TG.DEV


def _sync():
    if torch.device(_dev()).type == "cuda":
        torch.cuda.synchronize()


def _guarded(n, fill=0.0):
    t = torch.full((n + PAD,), SENT, device=_dev())
    t[:n] = fill
    return t


def _pad_ok(t, n):
    return bool((t[n:].view(torch.int32) == SENT_BITS).all())


def _np(t):
    return t.detach().cpu().numpy().copy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


class OptRig:
    """params, m, v, grad (ppo_grad_floats()) and kl_out, each with sentinel padding, the two optimiser slots, and a
    ppo_cfg_t whose optimiser fields are an OptCfg's; step() is one ppo_minibatch_apply checked against float64."""

    def __init__(self, cfg: O.OptCfg, kcfg=None, grad=None):
        from omniisaacgymenvs_loop_amd import _capi as c
        self.c = c
        if kcfg is None:
            self._ag = TG._agent(2, 32, mini_epochs=1)   # (a ppo_cfg_t with every other field set; kept alive)
            kcfg = self._ag.cfg
        self.cfg, self.kcfg = cfg, cfg.apply_to(kcfg)
        self.gf = c.lib().ppo_grad_floats()
        assert self.gf >= NP + 8 + IMAGE
        self.grad = _guarded(self.gf) if grad is None else grad
        assert self.grad.numel() == self.gf + PAD and self.grad.data_ptr() % 16 == 0
        self.p, self.m, self.v = _guarded(NP), _guarded(NP), _guarded(NP)
        self.opt = torch.zeros(16, device=_dev())
        self.kl_out = _guarded(1, SENT)
        self.lrs = []

    def set_cfg(self, cfg: O.OptCfg):
        self.cfg, self.kcfg = cfg, cfg.apply_to(self.kcfg)

    def put(self, t, a):
        t[:len(a)].copy_(torch.tensor(np.ascontiguousarray(a, F), device=_dev()))

    def load(self, case: O.StepCase, slot: int):
        self.set_cfg(case.cfg)
        for t, a in ((self.p, case.p), (self.m, case.m), (self.v, case.v), (self.grad, case.g)):
            self.put(t, a)
        self.grad[NP] = float(case.kl)
        self.opt.zero_()
        self.opt[8 * slot:8 * slot + 4].copy_(torch.tensor(case.opt_in, device=_dev()))

    def step(self, tn, slot, grad_scale=1.0, norm_from_partials=0, move=None, table=None):
        """One launch from the device's own state; returns (opt_out[8] as the device wrote it, errors, tolerances)."""
        c, cfg, o = self.c, self.cfg, 8 * slot
        pre = {k: _np(getattr(self, k)[:NP]) for k in ("p", "m", "v")}
        g, kl = _np(self.grad[:NP]), float(self.grad[NP])
        opt_in, grad_before = _np(self.opt[o:o + 8]), self.grad.clone()
        # the family's cap, on the values the device holds: g^2 stays finite in fp32
        assert np.abs(g.astype(np.float64) * grad_scale).max() <= O.G_CAP
        c.call("ppo_minibatch_apply", c.byref(self.kcfg), c.ptr(self.p), c.ptr(self.grad), c.ptr(self.m), c.ptr(self.v),
               c.ptr(self.opt), slot, float(grad_scale), c.ptr(self.kl_out), int(norm_from_partials), c.stream_ptr())
        _sync()
        out = tuple(_np(getattr(self, k)[:NP]) for k in ("p", "m", "v"))
        opt_out = _np(self.opt[8 - o:16 - o])
        # bounds and bystanders: the sentinels, the slot the launch read, the whole gradient buffer
        for k in ("p", "m", "v"):
            assert _pad_ok(getattr(self, k), NP), f"{tn}: floats behind {k} written"
        assert _pad_ok(self.grad, self.gf) and _pad_ok(self.kl_out, 1), f"{tn}: floats behind grad / kl_out written"
        assert _same_bits(_np(self.opt[o:o + 8]), opt_in), f"{tn}: the slot the step reads was written"
        assert torch.equal(self.grad.view(torch.int32), grad_before.view(torch.int32)), f"{tn}: grad written"
        klv = F(kl) * F(grad_scale)
        if cfg.lr_adaptive:
            assert _same_bits(_np(self.kl_out[:1]), [klv]), f"{tn}: kl_out"
        else:   # the fixed rate: lr and the kept KL pass through, kl_out is not touched
            assert _same_bits(_np(self.kl_out[:1]), [SENT]), f"{tn}: kl_out written without the adaptive schedule"
            assert _same_bits(opt_out[[0, 2]], opt_in[[0, 2]]), f"{tn}: lr / kl changed without the adaptive schedule"
        self.kl_out[0] = SENT
        args = (cfg, pre["p"], pre["m"], pre["v"], g, kl, opt_in, grad_scale)
        ref = O.ref_step64(*args)
        model_err = O.errors(O.model_step32(*args), ref)
        tol = O.tolerances(model_err)
        err = O.errors(out + (opt_out[:4],), ref)
        # the next step's cached constants (opt[4..7] = step_size, sqrt(bc2), their step, their rate): tags exact,
        # values within 2 ulp of float64
        n2 = float(opt_out[1]) + 1.0
        ss = float(opt_out[0]) / (1.0 - cfg.adam_b1 ** n2)
        bc = math.sqrt(1.0 - cfg.adam_b2 ** n2)
        tag_err = max(abs(float(opt_out[4]) / ss - 1.0), abs(float(opt_out[5]) / bc - 1.0))
        k, ratio = O.worst_ratio(err, tol)
        print(f"{tn}: worst {k}: err {err[k]:.3g}, model {model_err[k]:.3g}, tol {tol[k]:.3g} ({ratio:.2f} x tol); "
              f"all {({q: float(f'{err[q]:.2g}') for q in O.KEYS})}; norm {opt_out[3]:.6g} lr {opt_in[0]:.6g} -> "
              f"{opt_out[0]:.6g} step {opt_out[1]:g}; cached constants {tag_err:.2g}")
        tb = table or tn
        for q in O.KEYS:
            ET.record(tb, f"model {q}", model_err[q], 0.0)
            ET.record(tb, f"err/tol {q}", err[q] / tol[q], 0.0, tol=("<=1", 0))
            if model_err[q] > 0:
                ET.record(tb, f"err/model {q}", err[q] / model_err[q], 0.0, tol=(f"<={R.FACTOR}, or 2 ulp", 0))
        for q in O.KEYS:
            assert err[q] <= tol[q], f"{tn}: {q} misses float64 by {err[q]:.3g} > {tol[q]:.3g} (model {model_err[q]:.3g})"
        assert opt_out[6] == opt_out[1] + 1 and _same_bits(opt_out[7:8], opt_out[0:1]), f"{tn}: tags {opt_out}"
        assert tag_err <= O.ULP2, f"{tn}: cached constants off by {tag_err:.3g}"
        if move is not None:
            O.assert_rate_move(move, float(opt_in[0]), float(opt_out[0]), cfg)
            O.assert_rate_move(move, float(opt_in[0]), float(ref[3][0]), cfg)
        self.lrs.append(float(opt_in[0]))
        return opt_out, err, tol


# ---------------------------------------------------------------- one step: clip regimes, scale, constants, slots
@pytest.mark.parametrize("name", list(ONE_STEP))
def test_one_step_vs_float64(name):
    """Clip regimes (norm at 1e-3, 1 -+ 1e-3 and 1e3 x grad_norm; grad_norm = 1e-4 under a norm of 2e-4;
    truncate_grads = 0, the norm still reported), grad_scale 1 and 0.25 with the norm of the scaled gradient
    (norm_from_partials = 0, the collective chain's path), step counts 10, 1000 and 100000, non-yaml betas, eps,
    weight decay, KL threshold and rate bounds -- each from fresh (m = v = 0, step 0) or resumed moments."""
    case = ONE_STEP[name]
    O.assert_step_case(case)
    slot = list(ONE_STEP).index(name) % 2
    rig = OptRig(case.cfg)
    rig.load(case, slot)
    opt_out, _, _ = rig.step(f"ppo_opt_{name}", slot, case.grad_scale)
    if case.want_clipped is not None and case.cfg.truncate_grads:
        assert (case.cfg.grad_norm / (float(opt_out[3]) + 1e-6) < 1.0) == case.want_clipped


@pytest.mark.parametrize("name", ["clip_just_above_resumed", "constants_first"])
def test_both_slot_parities(name):
    """The same step through slot 0 -> 1 and slot 1 -> 0: the same bits, each within tolerance of float64."""
    case, outs = ONE_STEP[name], []
    for slot in (0, 1):
        rig = OptRig(case.cfg)
        rig.load(case, slot)
        opt_out, _, _ = rig.step(f"ppo_opt_slot{slot}_{name}", slot, case.grad_scale)
        outs.append([_np(rig.p), _np(rig.m), _np(rig.v), opt_out])
    for a, b in zip(*outs):
        assert _same_bits(a, b)


def test_norm_from_partials_after_real_gradient():
    """norm_from_partials = 1 behind a real ppo_minibatch_grad (stress family, 96 rows): the clip norm comes from the
    reduction's chunk squares, the reference's from the device gradient it read back; clipped (grad_norm at half the
    norm) and not; then the same inputs with the norm from the gradient itself (norm_from_partials = 0)."""
    from tests.test_ppo_grad_edges_gpu import Rig
    case = R.make_case("stress", 96)
    grig = Rig(96)
    grig.load(case)
    out = grig.run()
    norm = math.sqrt(float(np.sum(out["grad"].astype(np.float64) ** 2)))
    assert norm > 0 and out["kl"] > 0
    for tag, gn in (("clipped", 0.5 * norm), ("unclipped", 2.0 * norm)):
        cfg = O.OptCfg(grad_norm=gn, kl_threshold=float(out["kl"]))   # kl between the thresholds: the rate stays
        rig = OptRig(cfg, kcfg=grig.ag.cfg, grad=grig.grad)
        m, v = O.resumed_moments(3, out["grad"])
        for nfp in (1, 0):
            for t, a in ((rig.p, PO.flatten(case.P)), (rig.m, m), (rig.v, v)):
                rig.put(t, a)
            rig.opt.zero_()
            rig.opt[0], rig.opt[1] = 3e-4, 37.0
            opt_out, _, _ = rig.step(f"ppo_opt_partials{nfp}_{tag}", 0, 1.0, nfp, move="same")
            assert (gn / (float(opt_out[3]) + 1e-6) < 1.0) == (tag == "clipped")


def test_host_written_step_and_rate_under_stale_constants():
    """What restore does (a2c_continuous.py set_full_state_weights): the host writes opt[0] (rate) and opt[1] (step
    count) of a slot and leaves the cached constants opt[4..7] of an earlier chain behind.  First step from zeroed
    scalars; then, per step count 9, 999, 99999: the host's rate and count over the constants the previous launch left
    (both tags stale), and the slot that launch wrote, untouched (tags match: the constants may be reused); last, a
    slot with only the rate changed and one with only the count changed.  Every step must meet float64."""
    case = ONE_STEP["resume_9"]
    rig = OptRig(case.cfg)
    rig.load(case, 0)
    rig.opt.zero_()
    rig.opt[0] = 3e-4
    out, _, _ = rig.step("ppo_opt_tags_first", 0)                       # slot 0 (zeroed) -> slot 1
    assert out[1] == 1 and out[6] == 2
    slot = 1
    for n in O.RESUME_STEPS:
        tags = _np(rig.opt[8 * slot + 4:8 * slot + 8])
        rig.opt[8 * slot + 0], rig.opt[8 * slot + 1] = 1e-3 * (1 + slot), float(n)
        assert tags[2] != n + 1 and tags[3] != float(rig.opt[8 * slot]) and tags[2] > 0   # stale, from a real launch
        out, _, _ = rig.step(f"ppo_opt_tags_host_{n}", slot)
        assert out[1] == n + 1
        slot ^= 1
        out, _, _ = rig.step(f"ppo_opt_tags_kept_{n}", slot)            # the slot the kernel just wrote
        assert out[1] == n + 2
        slot ^= 1
    rig.opt[8 * slot + 0] = float(rig.opt[8 * slot]) * 0.5              # the rate alone
    assert float(rig.opt[8 * slot + 6]) == float(rig.opt[8 * slot + 1]) + 1
    rig.step("ppo_opt_tags_rate_only", slot)
    slot ^= 1
    rig.opt[8 * slot + 1] = 19.0                                        # the count alone
    assert float(rig.opt[8 * slot + 7]) == float(rig.opt[8 * slot])
    out, _, _ = rig.step("ppo_opt_tags_count_only", slot)
    assert out[1] == 20


def test_scheduler_sequence():
    """One sequence of 40 steps with the KL slot grad[PPO_NPARAM] written by the test (non-yaml kl_threshold 0.01,
    lr_min 1e-5, lr_max 2e-3): the rate falls to the floor and stays, climbs to the cap and stays, holds in band and
    exactly on 2 thr and 0.5 thr (fp32 products of the cfg field), moves one float outside either threshold and holds
    one float inside.  The slots alternate as in an epoch.  Then lr_adaptive = 0: the rate and the kept KL pass
    through and kl_out is not written."""
    seq = O.scheduler_cases()
    c0, cfg = seq[0][0], seq[0][0].cfg
    rig = OptRig(cfg)
    rig.load(c0, 0)
    for i, (case, move) in enumerate(seq):
        rig.grad[NP] = float(case.kl)
        assert float(rig.grad[NP]) == case.kl
        out, _, _ = rig.step(f"ppo_opt_sched_{i:02d}_{move}", i % 2, move=move, table="ppo_opt_sched")
        assert out[1] == i + 1
    O.assert_scheduler_coverage(rig.lrs + [float(out[0])], cfg)
    assert F(cfg.lr_min) in [F(x) for x in rig.lrs] and F(cfg.lr_max) in [F(x) for x in rig.lrs]
    import dataclasses
    rig.set_cfg(dataclasses.replace(cfg, lr_adaptive=0))
    n = len(seq)
    for i, kl in enumerate((F(10) * F(cfg.kl_threshold), F(0.1) * F(cfg.kl_threshold))):
        rig.grad[NP] = float(kl)
        rig.step(f"ppo_opt_sched_fixed_{i}", (n + i) % 2, table="ppo_opt_sched_fixed")


# ---------------------------------------------------------------- the chained update under the new configurations
OUT = ("model_params", "adam_m", "adam_v", "opt", "kls", "loss_log", "exp_mu", "exp_sigma")
ROWS = 64                                    # two gradient workgroups: the smallest real reduction
CHAINS = {1: (1, 1), 2: (2, 1), 5: (5, 1)}   # chain length: (minibatches, mini-epochs); _fill: odd minibatches 100 x
LR_FLOOR = 1e-4
CHAIN_CFGS = {
    "weight_decay": dict(weight_decay=1e-2),
    "betas_eps": dict(adam_b1=0.8, adam_b2=0.99, adam_eps=1e-5),
    "host_resumed": {},
    "lr_floor": dict(lr_min=LR_FLOOR, kl_threshold=1e-9),   # every KL is above 2 thr: the rate stays on its floor
}


def _chain(monkeypatch, fused, name, length, grad_norm, norms=None, last_unclipped=False):
    """update_epoch_minibatches over a chain of `length` steps, split (USV_PPO_FUSED=0) or fused; the fused run's grad
    has its image region and the floats behind it full of sentinels.  norms: the split path's clip norm of every step.
    last_unclipped: the split path's last step with truncate_grads = 0 (what the last speculative step computes)."""
    from omniisaacgymenvs_loop_amd import _capi as c
    nmb, me = CHAINS[length]
    monkeypatch.setenv("USV_PPO_FUSED", "1" if fused else "0")
    ag = TG._agent(ROWS * nmb // 16, ROWS, me)
    assert ag.cfg.minibatch == ROWS and ag.num_minibatches == nmb and ag.mini_epochs_num == me
    for k, val in CHAIN_CFGS[name].items():
        setattr(ag.cfg, k, val)
    ag.cfg.truncate_grads, ag.cfg.grad_norm = 1, grad_norm
    gf = ag.grad.numel()
    big = torch.full((gf + PAD,), SENT, device=_dev())
    big[:gf - IMAGE] = 0
    if fused:
        ag.grad = big
    if name == "lr_floor":
        ag.opt[0] = LR_FLOOR
    if name == "host_resumed":
        # an earlier chain leaves its cached constants in the slots; the host then writes step count and rate over
        # them (restore) and the dataset is put back
        _fill(ag, ROWS)
        ag.update_epoch_minibatches()
        _sync()
        assert float(ag.opt[6]) == length + 1 and float(ag.opt[1]) == length
        ag.opt[0], ag.opt[1] = 2e-4, 999.0
    _fill(ag, ROWS)
    call, applies = c.call, [0]

    def wrapped(fn, *a):
        last = fn == "ppo_minibatch_apply" and applies[0] == length - 1
        if last and last_unclipped:
            ag.cfg.truncate_grads = 0
        call(fn, *a)
        if fn == "ppo_minibatch_apply":
            applies[0] += 1
            if norms is not None:   # the launch read slot a[6] and wrote the other: its [3] is the norm
                norms.append(float(ag.opt[8 * (1 - a[6]) + 3]))
            if last:
                ag.cfg.truncate_grads = 1
    monkeypatch.setattr(c, "call", wrapped)
    try:
        ag.update_epoch_minibatches()
        _sync()
    finally:
        monkeypatch.setattr(c, "call", call)
    assert applies[0] == (0 if fused else length)
    out = {k: getattr(ag, k).clone() for k in OUT}
    if fused:
        assert _pad_ok(big, gf), "floats behind grad written"
        out["image"] = big[gf - IMAGE:gf].clone()
    if name == "lr_floor":
        assert _same_bits(_np(ag.opt[:1]), [LR_FLOOR]) and bool((ag.kls > 2e-9).all())
    if name == "host_resumed":
        assert float(ag.opt[1]) == 999 + length
    return out


@pytest.mark.parametrize("length", list(CHAINS))
@pytest.mark.parametrize("name", list(CHAIN_CFGS))
def test_chain_matches_split_path_under_new_configurations(name, length, monkeypatch):
    """ppo_minibatch_fused + ppo_minibatch_finish against ppo_minibatch_grad + ppo_minibatch_apply, bit for bit --
    parameters, moments, optimiser scalars (cached constants included), KLs, losses, mu / sigma write-back -- with
    weight decay, non-yaml betas and eps, a step count and rate the host wrote over an earlier chain's constants, and
    a rate pinned on its floor; chains of 1, 2 and 5 steps (the state ends in bank 1, 0, 1: both parities and the
    copy-back); clipping never due, due at every step (each speculative step redone) and, from two steps on, at some.
    The W2 image behind grad holds, in the image's layout, the W2 of the last speculative step bit for bit: the final
    W2 when that step was not clipped, else the W2 of the same step taken unclipped (the finish redoes a clipped
    step into the bank, not into the image, which no later launch reads); its pad words and the floats behind grad
    keep their sentinels.  With the one-step checks above on the split path this extends float64 to the chain."""
    free = []
    ref = _chain(monkeypatch, False, name, length, 1e6, free)
    assert len(free) == length and min(free) > 0
    modes = [("never", 1e6), ("always", 1e-6)]
    if length > 1:
        modes.append(("some", float(np.sqrt(min(free) * max(free)))))
    for mode, gn in modes:
        seen = []
        a = ref if mode == "never" else _chain(monkeypatch, False, name, length, gn, seen)
        seen = seen or free
        clipped = [n + 1e-6 > gn for n in seen]   # clip_grad_norm_: coef = gn / (norm + 1e-6) < 1
        print(f"chain {name} x {length}, {mode}: norms {[float(f'{n:.4g}') for n in seen]} clipped {clipped}")
        assert {"never": not any(clipped), "always": all(clipped),
                "some": any(clipped) and not all(clipped)}[mode], (mode, gn, seen)
        if mode != "never":
            assert not torch.equal(a["model_params"], ref["model_params"])
        b = _chain(monkeypatch, True, name, length, gn)
        for k in OUT:
            assert bool(torch.isfinite(b[k]).all()), f"{k} not finite ({mode})"
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{k} differs from the split path ({mode})"
        spec = _chain(monkeypatch, False, name, length, gn, last_unclipped=True) if clipped[-1] else a
        img = b["image"].view(NH, HS)
        w2 = spec["model_params"][OFF_W2:OFF_W2 + NH * NH].view(NH, NH)
        assert torch.equal(img[:, :NH].contiguous().view(torch.int32), w2.contiguous().view(torch.int32)), \
            f"W2 image after the finish ({mode})"
        assert bool((img[:, NH].contiguous().view(torch.int32) == SENT_BITS).all()), f"image pad words written ({mode})"
        if clipped[-1]:
            assert not torch.equal(w2.reshape(-1), a["model_params"][OFF_W2:OFF_W2 + NH * NH])
