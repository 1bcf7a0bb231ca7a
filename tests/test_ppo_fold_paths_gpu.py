"""The gradient kernel's cross-lane folds (csrc/ppo.hip mb_grad8w): the clip norm's chunk-square sums in front of the
first barrier, the heads' 16-lane sums, and the loss sums, which their waves keep in registers over the dz2 phase
and fold / store behind its barrier.

Shapes: minibatches of 32, 64 and 96 rows (one, two and three gradient workgroups -- the smallest of each; 96 rows
is no power of two of workgroups) and one of 8,192 rows (the headline minibatch)."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import ppo_oracle as PO
from tests.test_ppo_gpu import DEV, _agent
from tests.test_ppo_w2_image_gpu import _bits, _fill

pytestmark = pytest.mark.gpu
F = np.float32
ROWS = (32, 64, 96, 8192)
RB, RD_P = 32, 128                       # rows per gradient workgroup, slots per reduction chunk (csrc/ppo.hip)
P_LOSS = PO.NPARAM                       # partial-row slots of the a, c, entropy, bound and KL sums
OUT = ("model_params", "adam_m", "adam_v", "opt", "kls", "loss_log", "exp_mu", "exp_sigma")


def _chain(monkeypatch, fused, rows, grad_norm):
    """1 minibatch x 3 mini-epochs: ppo_minibatch_fused x 3 + ppo_minibatch_finish, or the split path's three
    ppo_minibatch_grad + ppo_minibatch_apply."""
    from omniisaacgymenvs_loop_amd import _capi as c
    monkeypatch.setenv("USV_PPO_FUSED", "1" if fused else "0")
    ag = _agent(rows // 16, rows, 3)
    assert ag.cfg.minibatch == rows and ag.num_minibatches == 1 and ag._fused_update() == fused
    ag.cfg.truncate_grads, ag.cfg.grad_norm = 1, grad_norm
    _fill(ag, rows)
    seen = []
    call = c.call

    def recording(name, *a):
        call(name, *a)
        seen.append(name)
    monkeypatch.setattr(c, "call", recording)
    ag.update_epoch_minibatches()
    torch.cuda.synchronize()
    monkeypatch.setattr(c, "call", call)
    want = ["ppo_minibatch_fused"] * 3 + ["ppo_minibatch_finish"] if fused else ["ppo_minibatch_grad",
                                                                                 "ppo_minibatch_apply"] * 3
    assert [n for n in seen if n.startswith("ppo_minibatch")] == want
    out = {k: getattr(ag, k).clone() for k in OUT}
    out["grad"] = ag.grad[:PO.NPARAM + 1].clone()   # the last minibatch's gradient and KL mean
    return out


@pytest.mark.parametrize("grad_norm", (1e6, 1e-6), ids=("never_clipped", "always_clipped"))
@pytest.mark.parametrize("rows", ROWS)
def test_chained_update_matches_split_path(rows, grad_norm, monkeypatch):
    """Parameters, Adam moments, optimiser scalars, loss_log, kls, the last gradient and the mu / sigma write-back of
    the chained update are the split path's bit for bit, with the chain's speculative step kept (norm 1e6) and redone
    in every launch (1e-6)."""
    ref = _chain(monkeypatch, False, rows, grad_norm)
    got = _chain(monkeypatch, True, rows, grad_norm)
    for k in ref:
        assert bool(torch.isfinite(ref[k]).all()), f"{k} not finite"
        assert torch.equal(_bits(ref[k]), _bits(got[k])), f"{k} differs between the chained and the split path"
    assert float(ref["loss_log"].abs().sum()) > 0 and float(ref["grad"].abs().sum()) > 0


def _fold64(v):
    """wave_sum's order in float32: partners 32, 16, 8, 4, 2, 1; lane 0's result."""
    v = np.asarray(v, F).copy()
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = (v + v[lane ^ m]).astype(F)
    return v[0]


@pytest.mark.parametrize("rows", ROWS)
def test_loss_slots_of_the_partial_rows(rows):
    """After one split-path ppo_minibatch_grad the five loss slots of every workgroup's partial row (chunk-major:
    [slot // 128][workgroup][slot % 128]) hold that workgroup's sums.

    Bit for bit where the per-row terms can be restated in float32 on the host: the bound loss from the mu the
    kernel wrote back (lanes 0-31 the rows, 32-63 zero, folded in wave_sum's order; the mu bias is set so that most
    rows are out of bounds) and the entropy (every row the same term E, 32 E exact).  The actor, critic and KL
    sums go through expf / logf and the device's forward, which the host cannot restate bit for bit: they are held
    to the float32 oracle's sums of the same 32 rows within 1e-3 of the sum of magnitudes (+ 1e-6) -- the oracle's
    forward differs from the matrix cores' by accumulation order only (~1e-6 relative in mu and v, amplified by at
    most ~|z| <= 10 through the ratio), and a sum stored to another slot or from a stale register is off by
    the size of the sum itself."""
    from omniisaacgymenvs_loop_amd import _capi as c
    ag = _agent(rows // 16, rows, 1)
    P = PO.unflatten(ag.model_params.cpu().numpy())
    P["bmu"] = np.array([1.6, -1.4], F)
    P["sigma"] = np.array([-0.25, 0.125], F)
    ag.model_params.copy_(torch.tensor(PO.flatten(P), device=DEV))
    _fill(ag, rows, seed=3)
    ag.partials.fill_(float("nan"))
    inputs = {k: getattr(ag, k).cpu().numpy().copy() for k in ("exp_obs", "exp_act", "exp_nlp", "exp_val", "exp_ret",
                                                               "exp_adv", "exp_mu", "exp_sigma")}
    c.call("ppo_minibatch_grad", c.byref(ag.cfg), c.ptr(ag.model_params), c.ptr(ag.obs_rms), c.ptr(ag.val_rms), 0,
           0, c.ptr(ag.exp_obs), c.ptr(ag.exp_act), c.ptr(ag.exp_nlp), c.ptr(ag.exp_val), c.ptr(ag.exp_ret),
           c.ptr(ag.exp_adv), c.ptr(ag.exp_mu), c.ptr(ag.exp_sigma), c.ptr(ag.grad), c.ptr(ag.losses),
           c.ptr(ag.partials), c.ptr(ag.work), c.stream_ptr())
    torch.cuda.synchronize()
    nblk = rows // RB
    part = ag.partials.cpu().numpy()

    def slot(b, idx):
        return part[(idx // RD_P) * nblk * RD_P + b * RD_P + idx % RD_P]

    mu = ag.exp_mu.cpu().numpy().astype(F)          # the kernel's mu, written back
    assert np.isfinite(mu).all() and (np.abs(mu) > 1.1).mean() > 0.5
    ls = P["sigma"].astype(F)
    half_log_2pi = F(0.5) * F(math.log(float(F(6.28318530717958647692))))   # 0.5f * logf(USV_2PI_F)
    E = F(F(F(0.5) + half_log_2pi) + ls[0]) + F(F(F(0.5) + half_log_2pi) + ls[1])
    xn = PO.RMS.zeros(33).norm(inputs["exp_obs"]) if ag.cfg.normalize_input else inputs["exp_obs"]
    cfg = PO.PPOConfig(e_clip=ag.cfg.e_clip, critic_coef=ag.cfg.critic_coef, entropy_coef=ag.cfg.entropy_coef,
                       bounds_loss_coef=ag.cfg.bounds_loss_coef, clip_value=bool(ag.cfg.clip_value), minibatch=RB)
    for b in range(nblk):
        r = slice(b * RB, (b + 1) * RB)
        # bound loss: (bl0^2 + bh0^2) + (bl1^2 + bh1^2) per row, plain float32 operations
        m = mu[r]
        bh, bl = np.maximum(m - F(1.1), F(0)).astype(F), np.minimum(m + F(1.1), F(0)).astype(F)
        t = ((bl * bl).astype(F) + (bh * bh).astype(F)).astype(F)
        rows_b = (t[:, 0] + t[:, 1]).astype(F)
        want_b = _fold64(np.concatenate([rows_b, np.zeros(32, F)]))
        got = [slot(b, P_LOSS + q) for q in range(5)]
        print(f"rows {rows} workgroup {b}: loss slots {got}, bound restated {want_b}, entropy restated {F(32) * E}")
        assert want_b > 0
        assert F(got[3]).view(np.int32) == want_b.view(np.int32), (b, got[3], want_b)
        assert F(got[2]).view(np.int32) == F(F(32) * E).view(np.int32), (b, got[2], F(32) * E)
        # actor, critic, KL: the oracle's float32 terms of the same 32 rows
        _, losses, kl, _, _ = PO.minibatch_grad(P, xn[r], inputs["exp_act"][r], inputs["exp_nlp"][r],
                                                inputs["exp_val"][r], inputs["exp_ret"][r], inputs["exp_adv"][r],
                                                inputs["exp_mu"][r], inputs["exp_sigma"][r], cfg)
        mag_a = float(np.abs(inputs["exp_adv"][r]).sum()) * 1.2    # |a_loss| <= |A| max(ratio, 1 + e_clip)
        for q, want, mag in ((0, losses[0] * RB, max(mag_a, abs(losses[0]) * RB)), (1, losses[1] * RB, losses[1] * RB),
                             (4, kl * RB, abs(kl) * RB)):
            assert abs(float(got[q]) - want) <= 1e-3 * mag + 1e-6, (b, q, got[q], want)
        assert abs(float(got[3]) - losses[3] * RB) <= 1e-3 * losses[3] * RB + 1e-6
    # the mean losses the reduction forms from the slots (sum over workgroups / rows) agree with the slots
    tot = np.array([sum(float(slot(b, P_LOSS + q)) for b in range(nblk)) for q in range(4)]) / rows
    np.testing.assert_allclose(ag.losses.cpu().numpy()[:4], tot, rtol=1e-5, atol=1e-7)
