"""The W2 image of the chained PPO update (csrc/ppo.hip): the speculative Adam step of k_reduce_partials writes W2 in
the gradient kernel's LDS layout (image[j * 129 + k] = W2[j][k]) into the last 16,512 floats of `grad`, and the next
minibatch's chained k_mb_grad copies it flat into LDS instead of staging W2 through registers.

Shapes: a minibatch of 32 rows (one gradient workgroup, a single reduction row), 64 rows (two workgroups, the
smallest real reduction) and 8,192 rows (the headline minibatch)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import ppo_oracle as PO
from tests.test_ppo_gpu import DEV, _agent

pytestmark = pytest.mark.gpu
NH, HS = 128, 129
IMAGE = NH * HS
OFF_W2 = 2 + NH * 33 + NH                # sigma, W1, b1 come first (include/usv_hip.h PPO_OFF_W2)
SENT = -7.25                             # sentinel (pad words, floats behind the buffer), compared bit for bit
PAD = 1024
ROWS = (32, 64, 8192)
OUT = ("model_params", "adam_m", "adam_v", "opt", "kls", "loss_log", "exp_mu", "exp_sigma")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sent_bits():
    return int(np.float32(SENT).view(np.int32))


def _fill(ag, rows, seed=0):
    """Random experience for every minibatch of the agent's dataset; the advantages and value errors of odd
    minibatches are 100 x those of even ones, so a chain over both has small and large gradient norms in turn."""
    rng = np.random.default_rng(seed)
    B = ag.exp_obs.shape[0]
    obs = rng.normal(0, 2, (B, 33)).astype(np.float32)
    act = rng.normal(0, 1, (B, 2)).astype(np.float32)
    P = PO.unflatten(ag.model_params.cpu().numpy())
    _, _, mu0, _ = PO.forward(P, np.clip(obs, -5, 5))
    sig0 = np.ones_like(mu0)
    nlp0 = PO.neglogp(act, mu0, sig0, np.zeros_like(mu0)) + rng.normal(0, 0.05, B).astype(np.float32)
    scale = np.where((np.arange(B) // rows) % 2 == 1, 5.0, 0.05).astype(np.float32)
    val = rng.normal(0, 1, B).astype(np.float32)
    ret = (val + rng.normal(0, 0.1, B) * scale).astype(np.float32)
    adv = rng.normal(0, 1, B).astype(np.float32) * scale
    T = lambda a: torch.tensor(np.ascontiguousarray(a), device=DEV)
    for name, arr in (("exp_obs", obs), ("exp_act", act), ("exp_nlp", nlp0), ("exp_val", val), ("exp_ret", ret),
                      ("exp_adv", adv), ("exp_mu", mu0 + 0.01), ("exp_sigma", sig0)):
        getattr(ag, name).copy_(T(arr))


def _guarded_grad(ag, image_fill):
    """grad at the size the library states, its image region filled with image_fill, followed by PAD sentinels."""
    gf = ag.grad.numel()
    big = torch.full((gf + PAD,), SENT, device=DEV)
    big[:gf - IMAGE] = 0
    big[gf - IMAGE:gf] = image_fill
    return big, gf


def _update(monkeypatch, fused, rows, nmb, mini_epochs, grad_norm, norms=None):
    """One update_epoch_minibatches over nmb minibatches x mini_epochs (a chain of nmb * mini_epochs steps).  The
    fused run starts from an image region (pad words included) full of NaN, with sentinels behind the buffer.
    norms: the split path's gradient norm of every step is appended (read after each ppo_minibatch_apply)."""
    from omniisaacgymenvs_loop_amd import _capi as c
    monkeypatch.setenv("USV_PPO_FUSED", "1" if fused else "0")
    ag = _agent(rows * nmb // 16, rows, mini_epochs)
    assert ag.cfg.minibatch == rows and ag.num_minibatches == nmb
    ag.cfg.truncate_grads, ag.cfg.grad_norm = 1, grad_norm
    _fill(ag, rows)
    big, gf = _guarded_grad(ag, float("nan"))
    if fused:
        ag.grad = big
    if norms is not None:
        call = c.call

        def recording(name, *a):
            call(name, *a)
            if name == "ppo_minibatch_apply":   # reads optimiser slot a[6], writes the other: its [3] is the norm
                norms.append(float(ag.opt[8 * (1 - a[6]) + 3]))
        monkeypatch.setattr(c, "call", recording)
    ag.update_epoch_minibatches()
    torch.cuda.synchronize()
    if norms is not None:
        monkeypatch.setattr(c, "call", call)
    if fused:   # bounds: nothing behind ppo_grad_floats() is written
        assert bool((_bits(big[gf:]) == _sent_bits()).all()), "floats behind grad written"
    return {k: getattr(ag, k).clone() for k in OUT}


def _same(a, b, what):
    for k in OUT:
        assert bool(torch.isfinite(b[k]).all()), f"{k} not finite ({what})"
        assert torch.equal(a[k], b[k]), f"{k} differs from the split path ({what})"


@pytest.mark.parametrize("rows", ROWS)
def test_poisoned_image_chain_matches_split_path(rows, monkeypatch):
    """Parameters, moments, optimiser scalars, KLs, losses and the mu / sigma write-back of the fused chain, started
    with the whole image region NaN, are the split path's (USV_PPO_FUSED=0) bit for bit -- never clipped (1e6),
    always clipped (1e-6: every step redone in the next launch, over a copy that may still be landing) and
    sometimes clipped (a norm between the chain's own) over 2 minibatches x 2 mini-epochs, and over a chain of odd
    length (1 minibatch x 3 mini-epochs, state copied back from bank 1).  So minibatch 0 never reads the image, the
    later ones read only words the reduction wrote, and the clip path wins over a late copy.  The sentinels behind
    ppo_grad_floats() floats of grad stay intact (checked in every fused run)."""
    free = []
    ref = _update(monkeypatch, False, rows, 2, 2, 1e6, free)
    assert len(free) == 4 and min(free) > 0
    lo, hi = max(free[0], free[2]), min(free[1], free[3])   # small-advantage / large-advantage minibatches
    assert lo < hi, free
    mid = float(np.sqrt(lo * hi))   # step 0 (norm free[0] < mid) is not clipped, so step 1 (free[1] > mid) is
    _same(ref, _update(monkeypatch, True, rows, 2, 2, 1e6), "never clipped")
    for gn, what in ((1e-6, "always clipped"), (mid, "sometimes clipped")):
        seen = []
        a = _update(monkeypatch, False, rows, 2, 2, gn, seen)
        clipped = [n + 1e-6 > gn for n in seen]               # clip_grad_norm_: coef = gn / (norm + 1e-6) < 1
        print(f"rows {rows} grad_norm {gn:.3g}: norms {seen} clipped {clipped}")
        assert all(clipped) if gn == 1e-6 else (any(clipped) and not all(clipped)), (gn, seen)
        assert not torch.equal(a["model_params"], ref["model_params"])
        _same(a, _update(monkeypatch, True, rows, 2, 2, gn), what)
    for gn in (1e6, 1e-6):
        _same(_update(monkeypatch, False, rows, 1, 3, gn), _update(monkeypatch, True, rows, 1, 3, gn),
              f"odd chain, grad_norm {gn}")


def _fused_call(ag, grad, k, update_obs_rms=0):
    from omniisaacgymenvs_loop_amd import _capi as c
    return c.call_rc("ppo_minibatch_fused", c.byref(ag.cfg), c.byref(ag._adam_banks()), k, c.ptr(ag.obs_rms),
                     update_obs_rms, k % ag.num_minibatches, c.ptr(ag.exp_obs), c.ptr(ag.exp_act), c.ptr(ag.exp_nlp),
                     c.ptr(ag.exp_val), c.ptr(ag.exp_ret), c.ptr(ag.exp_adv), c.ptr(ag.exp_mu), c.ptr(ag.exp_sigma),
                     c.ptr(grad), c.ptr(ag.loss_log[k]), c.ptr(ag.partials), c.ptr(ag.work),
                     c.ptr(ag.kls[k - 1:k]) if k else None, c.stream_ptr())


@pytest.mark.parametrize("rows", ROWS)
def test_image_holds_w2_of_the_bank_each_call_wrote(rows):
    """A fused chain k = 0, 1, 2: after each call the image words [j * 129 + k] are W2 of the bank that call's
    reduction stepped into (bank 1, 0, 1), bit for bit; the pad words [j * 129 + 128] keep what the test put there,
    and so do the floats behind the buffer."""
    ag = _agent(rows * 2 // 16, rows, mini_epochs=2)
    _fill(ag, rows)
    big, gf = _guarded_grad(ag, SENT)
    banks = (ag.model_params, ag._bank1[0])
    w2_before = banks[0][OFF_W2:OFF_W2 + NH * NH].clone()
    for k in range(3):
        assert _fused_call(ag, big, k) == 0
        torch.cuda.synchronize()
        img = big[gf - IMAGE:gf].view(NH, HS)
        w2 = banks[(k & 1) ^ 1][OFF_W2:OFF_W2 + NH * NH].view(NH, NH)
        assert bool(torch.isfinite(w2).all()) and not torch.equal(w2.reshape(-1), w2_before)   # a step was taken
        assert torch.equal(_bits(img[:, :NH]), _bits(w2)), f"image after call {k}"
        assert bool((_bits(img[:, NH]) == _sent_bits()).all()), f"pad words written by call {k}"
        assert bool((_bits(big[gf:]) == _sent_bits()).all()), f"floats behind grad written by call {k}"
        w2_before = w2.reshape(-1).clone()


@pytest.mark.parametrize("rows", ROWS)
def test_misaligned_grad_is_refused_before_any_launch(rows):
    """A grad pointer 4 bytes off a 16-byte boundary: the fused entry point returns non-zero (the code of its other
    alignment checks) for the first call of a chain and for a chained one, and nothing is launched -- the
    observation statistics it was asked to update, the banks, grad, partials, the loss row and the mu write-back
    are untouched."""
    ag = _agent(rows * 2 // 16, rows, mini_epochs=2)
    _fill(ag, rows)
    big, gf = _guarded_grad(ag, SENT)
    assert big.data_ptr() % 16 == 0
    watched = {"obs_rms": ag.obs_rms, "params": ag.model_params, "bank1": ag._bank1, "m": ag.adam_m, "v": ag.adam_v,
               "opt": ag.opt, "grad": big, "partials": ag.partials, "loss_log": ag.loss_log, "exp_mu": ag.exp_mu}
    before = {k: t.clone() for k, t in watched.items()}
    for k in (0, 1):
        assert _fused_call(ag, big[1:], k, update_obs_rms=1) == 3
    torch.cuda.synchronize()
    for k, t in watched.items():   # (no NaN in any of them: equal values are equal bits up to the sign of zero)
        assert torch.equal(t, before[k]), f"{k} changed"
