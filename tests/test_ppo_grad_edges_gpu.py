"""ppo_minibatch_grad (k_obs_stats, k_mb_grad, k_reduce_partials of csrc/ppo.hip) against float64 autograd of the
same loss (tests/ppo_ref64.py) where the gradient path can go wrong unseen: parameters and data that take every
branch (saturated tanh, clipped ratio and value, bound loss, observations on the +-5 clip, sigma != 1), 1, 3, 17,
255 and 257 gradient workgroups, the config switches, a row offset, and the observation statistics on columns with
a large mean and a small spread.

The gradient is judged by K = max |g - g64| / A (A: the sum over rows of the absolute per-row contributions).  Its
tolerance is FACTOR x K_model, K_model being the K of the fp32 numpy oracle with a model of the kernel's tanh on the
same case, computed here on the CPU: no tolerance comes from the kernel's output.  tests/test_ppo_ref64_cpu.py
shows that eight kinds of wrong gradient exceed four times this tolerance at every row count."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import ppo_oracle as PO
from tests import errtab as ET
from tests import ppo_ref64 as R
from tests.test_ppo_gpu import DEV, _agent

pytestmark = pytest.mark.gpu
SENT = -7.25            # sentinel padding / untouched rows (compared bit for bit)
PAD = 1024              # sentinel floats behind grad and partials
BUFS = ("exp_obs", "exp_act", "exp_nlp", "exp_val", "exp_ret", "exp_adv", "exp_mu", "exp_sigma")


class Rig:
    """An agent's cfg, parameters and experience buffers around ppo_minibatch_grad, with grad and partials of the
    sizes the library states (ppo_grad_floats, ppo_partials_floats) followed by sentinel padding."""

    def __init__(self, rows, nmb=1, **cfg):
        from omniisaacgymenvs_loop_amd import _capi as c
        assert (rows * nmb) % 16 == 0
        self.c, self.rows = c, rows
        self.ag = ag = _agent(rows * nmb // 16, rows, mini_epochs=1)
        assert ag.cfg.minibatch == rows and ag.exp_obs.shape[0] == rows * nmb
        # the yaml's values are the ones the float64 side states
        base = PO.PPOConfig()
        for k in ("e_clip", "critic_coef", "entropy_coef", "bounds_loss_coef"):
            assert abs(getattr(ag.cfg, k) - getattr(base, k)) < 1e-7, k
        assert ag.cfg.clip_value == 1 and ag.cfg.normalize_input == 1 and ag.cfg.bf16_gemm == 0
        for k, v in cfg.items():
            setattr(ag.cfg, k, v)
        self.gf, self.pf = c.lib().ppo_grad_floats(), c.lib().ppo_partials_floats(rows)
        assert self.gf == ag.grad.numel() and self.pf == ag.partials.numel()
        # floats the nblk partial rows take: the size's slope in the row-block count (the chunk-major rows are the
        # whole buffer)
        lib = c.lib()
        row = (lib.ppo_partials_floats(32 * 8192) - lib.ppo_partials_floats(32 * 4096)) // 4096
        self.used = rows // 32 * row
        assert PO.NPARAM + 8 <= row < PO.NPARAM + 8 + 128 and self.used == self.pf
        self.grad = torch.full((self.gf + PAD,), SENT, device=DEV)
        self.partials = torch.full((self.pf + PAD,), SENT, device=DEV)
        self.grad[:self.gf] = 0
        self.partials[:self.pf] = 0
        for name in BUFS:
            getattr(ag, name).fill_(SENT)
        self.rms0 = ag.obs_rms.clone()

    def load(self, case, mb_index=0):
        ag, a = self.ag, slice(mb_index * self.rows, (mb_index + 1) * self.rows)
        assert case.rows == self.rows
        ag.model_params.copy_(torch.tensor(PO.flatten(case.P), device=DEV))
        for name, arr in zip(BUFS, (case.obs,) + case.data()):
            getattr(ag, name)[a].copy_(torch.tensor(np.ascontiguousarray(arr), device=DEV))
        self.saved = {name: getattr(ag, name).clone() for name in BUFS}

    def restore(self):
        for name, t in self.saved.items():
            getattr(self.ag, name).copy_(t)
        self.ag.obs_rms.copy_(self.rms0)

    def run(self, update_obs_rms=1, mb_index=0):
        ag, c = self.ag, self.c
        c.call("ppo_minibatch_grad", c.byref(ag.cfg), c.ptr(ag.model_params), c.ptr(ag.obs_rms), c.ptr(ag.val_rms),
               update_obs_rms, mb_index, c.ptr(ag.exp_obs), c.ptr(ag.exp_act), c.ptr(ag.exp_nlp), c.ptr(ag.exp_val),
               c.ptr(ag.exp_ret), c.ptr(ag.exp_adv), c.ptr(ag.exp_mu), c.ptr(ag.exp_sigma), c.ptr(self.grad),
               c.ptr(ag.losses), c.ptr(self.partials), c.ptr(ag.work), c.stream_ptr())
        torch.cuda.synchronize()
        n = lambda t: t.cpu().numpy().copy()
        out = {"grad": n(self.grad[:PO.NPARAM]), "kl": float(self.grad[PO.NPARAM]), "losses": n(ag.losses)[:5],
               "mu": n(ag.exp_mu), "sigma": n(ag.exp_sigma), "obs_rms": n(ag.obs_rms)}
        # nothing is written behind the sizes the library states
        assert bool((self.grad[self.gf:].view(torch.int32) == _bits(SENT)).all()), "grad tail written"
        assert bool((self.partials[self.pf:].view(torch.int32) == _bits(SENT)).all()), "partials tail written"
        # ... nor behind the nblk rows (used == pf: the rows end where the buffer does)
        assert bool((self.partials[self.used:self.pf].view(torch.int32) == 0).all()), "partials past nblk rows written"
        return out


def _bits(x):
    return int(np.float32(x).view(np.int32))


def _bitwise_equal(a, b, keys=("grad", "kl", "losses", "mu", "sigma", "obs_rms")):
    for k in keys:
        x, y = (np.ascontiguousarray(np.atleast_1d(v)).view(np.uint8) for v in (a[k], b[k]))
        np.testing.assert_array_equal(x, y, err_msg=k)


def _check(tn, out, case, cfg, normalize=True, lowp=False, rows_slice=slice(None)):
    """The per-case assertions: gradient by K against FACTOR x K_model, loss means and KL at the project's 1e-5, the
    mu / sigma write-back within 1e-5 of the float64 forward.  bf16 GEMM mode (lowp): the gradient is still judged
    against float64, but loss means, KL and write-back cannot be -- bf16 operands move them by 1e-4 .. 1e-2 -- and
    are held, at the same bounds, to the oracle with the same operand rounding (as test_ppo_gpu.py does)."""
    ref = R.case_ref64(case, cfg, normalize)                    # (asserts the family conditions)
    km = R.K_model(case, cfg, ref, normalize, lowp=lowp)        # CPU only: fp32 oracle with the kernel's tanh
    fwd = ref
    if lowp:
        _, losses, kl, mu, sigma = R.oracle_grad(case, cfg, normalize, tanh=True, lowp=True)
        fwd = R.Ref64(None, None, losses, kl, mu, sigma, None)
    tol = R.FACTOR * km
    ET.record(tn, "K_model", km, 0.0)
    K = R.K_of(out["grad"], ref)
    print(f"{tn}: K_kernel = {K:.3g}, K_model = {km:.3g}, ratio {K / km:.2f}, tol {tol:.3g}; "
          f"blocks {({k: float(f'{v:.2g}') for k, v in R.K_blocks(out['grad'], ref).items()})}")
    print(f"{tn}: losses {out['losses'][:4]} vs {fwd.losses}, kl {out['kl']} vs {fwd.kl}, "
          f"max |mu - ref| {np.abs(out['mu'][rows_slice] - fwd.mu).max():.3g}, "
          f"max |sigma - ref| {np.abs(out['sigma'][rows_slice] - fwd.sigma).max():.3g}")
    R.check_grad(tn, out["grad"], ref, tol, k_model=km, blocks=True)
    ET.check(tn, "losses", out["losses"][:4], np.array(fwd.losses), 1e-5, 1e-5, ["a", "c", "ent", "b"])
    ET.check(tn, "kl", out["kl"], fwd.kl, 1e-5, 1e-5)
    ET.check(tn, "mu", out["mu"][rows_slice], fwd.mu, 0, 1e-5, ["mu0", "mu1"])
    ET.check(tn, "sigma", out["sigma"][rows_slice], fwd.sigma, 0, 1e-5, ["s0", "s1"])
    return ref


@pytest.mark.parametrize("rows", R.ROWS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_gradient_vs_float64_at_edge_row_counts(family, rows):
    """nblk = 1, 3, 17, 255, 257: one workgroup, odd counts, one more than the reduction's 16 row groups, one less
    and one more than its 256-row step.  update_obs_rms = 1 from zero statistics: the kernel's own normalisation
    (one-pass fp64 sums) feeds the gradient, the float64 side normalises with two-pass statistics."""
    case, cfg = R.make_case(family, rows), PO.PPOConfig(minibatch=rows)
    rig = Rig(rows)
    rig.load(case)
    out = rig.run()
    _check(f"ppo_edges_{family}_{rows}", out, case, cfg)
    mean, var, count = R.rms64(case.obs)
    # fp64 sums of at most 8224 values of mean magnitude ~2 in another order: n eps mean|x| = 2e-12 at the worst
    np.testing.assert_allclose(out["obs_rms"][:33], mean, rtol=0, atol=1e-11)
    np.testing.assert_allclose(out["obs_rms"][33:66], var, rtol=1e-9)   # (means near 0: one pass loses nothing)
    assert out["obs_rms"][66] == count


COEFS = dict(e_clip=0.1, critic_coef=2.0, bounds_loss_coef=1.0)
# name: (fields of the kernel's ppo_cfg_t, the same statement for the float64 side)
CONFIG_PATHS = {
    "noclip": (dict(clip_value=0), dict(clip_value=False)),
    "nonorm": (dict(normalize_input=0), {}),
    "ent": (dict(entropy_coef=0.01), dict(entropy_coef=0.01)),
    "coefs": (COEFS, COEFS),
    "bf16": (dict(bf16_gemm=1), {}),
}


@pytest.mark.parametrize("path", list(CONFIG_PATHS))
def test_config_paths_vs_float64(path):
    """clip_value = 0, normalize_input = 0 (observations pre-scaled, statistics untouched), the entropy bonus,
    non-yaml e_clip / critic_coef / bounds_loss_coef (a constant hard-coded at its yaml value fails here), and the
    bf16 GEMM mode, whose K_model is the oracle's bf16 operand rounding against float64."""
    kcfg, ocfg = CONFIG_PATHS[path]
    cfg = PO.PPOConfig(minibatch=96, **ocfg)
    normalize = path != "nonorm"
    case = R.make_case("stress", 96, cfg.e_clip, normalize)
    rig = Rig(96, **kcfg)
    rig.load(case)
    out = rig.run(update_obs_rms=int(normalize))
    tn = f"ppo_edges_cfg_{path}"
    ref = _check(tn, out, case, cfg, normalize, lowp=path == "bf16")
    if not normalize:
        np.testing.assert_array_equal(out["obs_rms"], rig.rms0.cpu().numpy())
    if path == "bf16":
        # 8 x 0.03 against float64 sees little.  Against the oracle with the same bf16 operand rounding the kernel
        # differs by fp32 order and tanh only, so the distance between the two, in the same measure, is held to the
        # fp32 tolerance of the case (an operand that rounds to the other bf16 neighbour would show as 2^-9)
        g_lowp = R.oracle_grad(case, cfg, tanh=True, lowp=True)[0]
        A = ref.flat_A()
        k_lowp = float(np.max(np.abs(out["grad"] - g_lowp)[A > 0] / A[A > 0]))
        tol32 = R.FACTOR * R.K_model(case, cfg, ref)
        print(f"{tn}: K vs bf16 oracle = {k_lowp:.3g}, tol {tol32:.3g}")
        ET.record(tn, "K vs bf16 oracle", k_lowp, 0.0, tol=(f"K<={tol32:.3g}", 0))
        assert k_lowp <= tol32, (k_lowp, tol32)


def test_row_offset_takes_the_second_minibatch():
    """mb_index = 1 of a 2 x 96-row dataset: the gradient, losses, KL and statistics are those of the second half alone
    (bit for bit the same as that half run as a dataset of its own, and within tolerance of float64), its mu /
    sigma rows are written, and the first half's keep their sentinel bit for bit."""
    case, other, cfg = R.make_case("stress", 96), R.make_case("boundary", 96), PO.PPOConfig(minibatch=96)
    rig = Rig(96, nmb=2)
    rig.load(other, 0)
    rig.load(case, 1)
    rig.ag.exp_mu[:96].fill_(SENT)
    rig.ag.exp_sigma[:96].fill_(SENT)
    out = rig.run(mb_index=1)
    _check("ppo_edges_offset", out, case, cfg, rows_slice=slice(96, 192))
    for k in ("mu", "sigma"):
        assert (out[k][:96].view(np.int32) == _bits(SENT)).all(), f"{k} of the first minibatch written"
    alone = Rig(96)
    alone.load(case)
    out0 = alone.run()
    _bitwise_equal(out, out0, ("grad", "kl", "losses", "obs_rms"))
    np.testing.assert_array_equal(out["mu"][96:], out0["mu"])
    np.testing.assert_array_equal(out["sigma"][96:], out0["sigma"])


@pytest.mark.parametrize("rows", [96, 544, 8224])
def test_repeat_is_bit_identical(rows):
    case = R.make_case("stress", rows)
    rig = Rig(rows)
    rig.load(case)
    a = rig.run()
    rig.restore()
    b = rig.run()
    _bitwise_equal(a, b)


# ---------------------------------------------------------------- observation statistics under the gradient
def _stat_columns(rng, rows):
    """33 columns shaped like the task's: N(0, 2), constant 0.1, constant 0, mean 100 with std 1e-3, mean 1e3 with
    std 1e-2 (kind = column % 5), as the fp32 values the kernel reads."""
    kinds = np.arange(33) % 5
    x = np.empty((rows, 33))
    x[:, kinds == 0] = rng.normal(0, 2, (rows, int((kinds == 0).sum())))
    x[:, kinds == 1] = 0.1
    x[:, kinds == 2] = 0.0
    x[:, kinds == 3] = 100 + rng.normal(0, 1e-3, (rows, int((kinds == 3).sum())))
    x[:, kinds == 4] = 1e3 + rng.normal(0, 1e-2, (rows, int((kinds == 4).sum())))
    return x.astype(np.float32), kinds


@pytest.mark.parametrize("start", ["zero", "matched"])
@pytest.mark.parametrize("rows", [32, 96, 8224])
def test_obs_statistics_vs_two_pass_float64(rows, start):
    """k_obs_stats (fp64 sums over 64 workgroups; 32 rows: half of them have no row) against two-pass float64 over two
    updates in sequence -- the second merges into count > 1: count and mean, the variance never negative, and what
    the network sees, (x - mean) / sqrt(var + 1e-5) clipped at +-5, within 1e-5 when formed in float64 from either
    side's statistics.  start = zero: the fresh (0, 1, count 1), where the jump of the mean carries the merged
    variance of the large-mean columns.  start = matched: the statistics of an earlier batch of the same columns
    (mean 100 / var 1e-6, constant / var 0, ...), where the batch variance itself carries it -- a one-pass
    (sum x^2 - n mean^2) loses 1e-4 of it at mean 100 and can go negative on a constant column."""
    rng = np.random.default_rng(11)
    a, kinds = _stat_columns(rng, rows)
    b, _ = _stat_columns(rng, rows)
    case = R.make_case("stress", rows)
    rig = Rig(rows, nmb=2)
    rig.load(case, 0)
    rig.load(case, 1)
    rig.ag.exp_obs[:rows].copy_(torch.tensor(a, device=DEV))
    rig.ag.exp_obs[rows:].copy_(torch.tensor(b, device=DEV))
    want = (None, None, 1.0)
    if start == "matched":
        e = _stat_columns(rng, rows)[0].astype(np.float64)
        want = (e.mean(0), ((e - e.mean(0)) ** 2).sum(0) / (rows - 1.0), float(rows))
        assert (want[1][(kinds == 1) | (kinds == 2)] == 0).all()
        rig.ag.obs_rms.copy_(torch.tensor(np.concatenate([want[0], want[1], [want[2]]]), device=DEV))
    for i, x in enumerate((a, b)):
        got = rig.run(update_obs_rms=1, mb_index=i)["obs_rms"]
        want = R.rms64(x, *want)
        tn = f"ppo_edges_obs_stats_{rows}_{start}_call{i}"
        dn = max(np.abs(R.norm64(y, got[:33], got[33:66]) - R.norm64(y, want[0], want[1])).max() for y in (a, b))
        print(f"{tn}: min var {got[33:66].min():.3g}, max |var - var64| per kind "
              f"{[float(f'{np.abs(got[33:66] - want[1])[kinds == q].max():.2g}') for q in range(5)]}, "
              f"max |normalised - normalised64| {dn:.3g}")
        ET.record(tn, "var", got[33:66], want[1])
        assert got[66] == want[2]
        # fp64 sums in another order: n eps mean|x| at the worst, 9e-10 of 1e3 and 2e-12 of the N(0, 2) columns
        ET.check(tn, "mean", got[:33], want[0], 1e-12, 1e-11)
        assert (got[33:66] >= 0).all(), got[33:66].min()
        for y in (a, b):
            ET.check(tn, "normalised", R.norm64(y, got[:33], got[33:66]), R.norm64(y, want[0], want[1]), 0, 1e-5)
        assert np.isfinite(rig.grad[:PO.NPARAM].cpu().numpy()).all()
