"""The PPO gradient's reference pair on the CPU: the numpy oracle's hand-written backprop (oracle/ppo_oracle.py,
fp32) against float64 autograd of the same loss (tests/ppo_ref64.py) on the stress and boundary families, the
model of the kernel's tanh that sets the GPU tolerance, and the mutants that tolerance has to reject.

Measured (K = max |g - g64| / A, see ppo_ref64): oracle 1.9e-7 .. 4.1e-6, tanh model 2.1e-7 .. 4.6e-6, the
largest at 32 rows; the weakest rejected mutant (bound term dropped, bounds_loss_coef 1e-4) is 16x the rejection
threshold of 32 K_model at its weakest row count (96), the next (a dropped row, 8224 rows) 180x."""
import numpy as np
import pytest

from oracle import ppo_oracle as PO
from tests import errtab as ET
from tests import ppo_ref64 as R

CONFIGS = {"base": {}, "ent": {"entropy_coef": 0.01}, "noclip": {"clip_value": False},
           "ent_noclip": {"entropy_coef": 0.01, "clip_value": False},
           "coefs": {"e_clip": 0.1, "critic_coef": 2.0, "bounds_loss_coef": 1.0}}
# sanity cap on the reference pair (about 4x the largest measured K), not a kernel tolerance
K_CAP = 2e-5


def _case(family, rows, cfg_name):
    cfg = PO.PPOConfig(minibatch=rows, **CONFIGS[cfg_name])
    case = R.make_case(family, rows, cfg.e_clip)
    return case, cfg, R.case_ref64(case, cfg)   # (asserts the family conditions)


@pytest.mark.parametrize("cfg_name", list(CONFIGS))
@pytest.mark.parametrize("rows", R.ROWS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_oracle_backprop_vs_float64_autograd(family, rows, cfg_name):
    case, cfg, ref = _case(family, rows, cfg_name)
    g, losses, kl, mu, sigma = R.oracle_grad(case, cfg)
    tn = f"ppo_oracle64_{family}_{rows}_{cfg_name}"
    R.check_grad(tn, g, ref, K_CAP)
    np.testing.assert_allclose(losses, ref.losses, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(kl, ref.kl, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(mu, ref.mu, rtol=0, atol=1e-5)
    np.testing.assert_allclose(sigma, ref.sigma, rtol=0, atol=1e-5)


def test_tanh_model_pointwise():
    """The model of ppo.hip fast_tanh stays within the 2e-7 the kernel's comment states, saturates to +-1 exactly
    where exp2 overflows / underflows, and is what the formula says at a few hand-checked points."""
    x = np.concatenate([np.linspace(-12, 12, 200001), [-200.0, -90.0, 90.0, 200.0, 0.0]]).astype(np.float32)
    y = R.tanh_model(x)
    assert y.dtype == np.float32
    assert np.abs(y.astype(np.float64) - np.tanh(x.astype(np.float64))).max() < 2e-7
    np.testing.assert_array_equal(y[-5:], np.array([-1, -1, 1, 1, 0], np.float32))


@pytest.mark.parametrize("rows", R.ROWS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_tanh_model_gradient_vs_float64(family, rows):
    """K_model: the oracle with the kernel's tanh.  Within the same sanity cap, and close to the plain oracle's K:
    the 2e-7 of the tanh is not what limits the pair."""
    case, cfg, ref = _case(family, rows, "base")
    km = R.K_model(case, cfg, ref)
    R.check_grad(f"ppo_tanh_model_{family}_{rows}", R.oracle_grad(case, cfg, tanh=True)[0], ref, K_CAP)
    assert km == R.K_of(R.oracle_grad(case, cfg, tanh=True)[0], ref)   # (deterministic: the GPU test recomputes it)
    klow = R.K_model(case, cfg, ref, lowp=True)
    ET.record(f"ppo_tanh_model_{family}_{rows}", "K bf16", klow, 0.0)
    assert km < klow   # bf16 operands (2^-9 relative) in the 128 x 128 products sit far above fp32


def _mutant_cfg(mutant):
    return "ent" if mutant == "entropy_dropped" else "base"


@pytest.mark.parametrize("rows", R.ROWS)
@pytest.mark.parametrize("mutant", [m for m in R.MUTANTS if m != "tie_g1"])
def test_mutant_is_rejected(mutant, rows):
    """Each wrong oracle fails the GPU tests' own assertion (check_grad) at four times the GPU tolerance
    FACTOR * K_model, on at least one family, at every row count; the unmutated oracle passes it at the tolerance
    itself on both.  e_clip + 0.005 is judged on the boundary family alone (rows at 1 + e_clip + 0.002)."""
    rejected = []
    for family in (("boundary",) if mutant == "e_clip_0205" else R.FAMILIES):
        case, cfg, ref = _case(family, rows, _mutant_cfg(mutant))
        tol = R.FACTOR * R.K_model(case, cfg, ref)
        R.check_grad("", R.oracle_grad(case, cfg)[0], ref, tol, record=False)
        g = R.oracle_grad(case, cfg, mutant=mutant)[0]
        if R.K_of(g, ref) > 4 * tol:   # (K_of itself asserts a finite gradient: only a K above the bound counts)
            with pytest.raises(AssertionError, match="K = "):
                R.check_grad("", g, ref, 4 * tol, record=False)
            rejected.append(family)
    assert rejected, f"{mutant} at {rows} rows passes 4 x tolerance on every family"


@pytest.mark.parametrize("rows", R.ROWS)
def test_tie_arm_mutant_is_equivalent(rows):
    """The tie arm 0.5 (g1 + g2) of the surrogate is taken when s1 == s2: inside the clip range, where g1 == g2,
    or at adv == 0 (forced on three boundary rows), where both are 0.  Returning g1 there is therefore the same
    function -- no data can reject it through the gradient -- and the mutant is pinned as equivalent instead:
    bit-identical gradients, with the tie rows present."""
    for family in R.FAMILIES:
        case, cfg, ref = _case(family, rows, "base")
        if family == "boundary":
            assert (case.adv == 0).sum() >= 2
        np.testing.assert_array_equal(R.oracle_grad(case, cfg, mutant="tie_g1")[0], R.oracle_grad(case, cfg)[0])


def test_family_conditions_reject_the_benign_regime():
    """The data of the existing gradient tests (fresh parameters, N(0, 1) actions around zero-bias means, 0.05 noise
    on the old neglogp) meets none of the five branch conditions: each of the helper's assertions is live."""
    from omniisaacgymenvs_loop_amd.rl_games.a2c_continuous import default_linear_init
    rng = np.random.default_rng(0)
    B = 96
    P = PO.unflatten(default_linear_init(42).numpy())
    obs = rng.normal(0, 2, (B, 33)).astype(np.float32)
    xn = R.norm64(obs, *R.rms64(obs)[:2])
    _, _, mu, v = PO.forward(P, xn.astype(np.float32))
    act = rng.normal(0, 1, (B, 2)).astype(np.float32)
    nlp = PO.neglogp(act, mu, np.ones_like(mu), np.zeros_like(mu)) + rng.normal(0, 0.05, B).astype(np.float32)
    val = rng.normal(0, 1, B).astype(np.float32)
    case = R.Case("stress", B, 0.2, P, obs, act, nlp, val, (val + rng.normal(0, 0.5, B)).astype(np.float32),
                  rng.normal(0, 1, B).astype(np.float32), mu + 0.01, np.ones_like(mu))
    cfg = PO.PPOConfig(minibatch=B)
    held = R.conditions(case, R.ref64(P, xn, *case.data(), cfg))
    for name in ("ratio clip share", "value clip share", "bound share", "saturated layer-1 unit", "obs clip share"):
        assert not held[name][0], (name, held[name][1])
    with pytest.raises(AssertionError):
        R.case_ref64(case, cfg)


def test_float64_statistics_vs_oracle_rms():
    """rms64 (two-pass batch variance, Chan merge) and the oracle's RMS.update agree over two merges."""
    rng = np.random.default_rng(7)
    a, b = rng.normal(1, 2, (96, 33)).astype(np.float32), rng.normal(-1, 3, (32, 33)).astype(np.float32)
    o = PO.RMS.zeros(33)
    o.update(a)
    o.update(b)
    m, v, n = R.rms64(b, *R.rms64(a))
    np.testing.assert_allclose(m, o.mean, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(v, o.var, rtol=1e-13)
    assert n == o.count == 129


def test_float64_reference_matches_finite_differences():
    """The autograd gradient against central differences of the float64 loss on one element per block, away from
    the kinks (every row is 1e-3 from a threshold): the forward expression and the returned blocks belong together."""
    case, cfg, ref = _case("stress", 32, "ent")
    xn = R.case_xn64(case)

    def loss(P):
        r = R.ref64(P, xn, *case.data(), cfg)
        return r.losses[0] + 0.5 * cfg.critic_coef * r.losses[1] - cfg.entropy_coef * r.losses[2] \
            + cfg.bounds_loss_coef * r.losses[3]

    for k, shape in PO.SHAPES:
        idx = tuple(s // 2 for s in shape)
        h = 1e-6
        Pp = {q: np.asarray(w, np.float64).copy() for q, w in case.P.items()}
        Pm = {q: w.copy() for q, w in Pp.items()}
        Pp[k][idx] += h
        Pm[k][idx] -= h
        fd = (loss(Pp) - loss(Pm)) / (2 * h)
        assert abs(fd - ref.grad[k][idx]) <= 1e-6 * max(1.0, ref.A[k][idx]), (k, fd, ref.grad[k][idx])
