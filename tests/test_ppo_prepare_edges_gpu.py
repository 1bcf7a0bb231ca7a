"""ppo_prepare (k_value, k_gae<16> / k_gae<0>, k_prepare_finalize, k_prepare_apply of csrc/ppo.hip) and the rollout
forward (ppo_policy_step, ppo_value) against float64 where they can go wrong unseen.

Dataset preparation, through the C ABI with the test's own buffers (work sized as a2c_continuous.py sizes it): 1, 255,
257 and 1,000 envs x 16 slots in the vector form and in the runtime-horizon loop, horizons 8 and 24 that only the loop
takes, 262,145 envs x 1 slot (1,025 partial rows: the second round of the finalize fold); no env done, every slot
done, an env done at every slot beside one done only at slot 0 and one only at slot H - 1, mixed last_dones, a random
30 %; the yaml's gamma / tau and (0.9, 0.5); N(0.5, 1) values, and values of 1e3 + N(0, 1e-2) with rewards N(0, 1e-3)
-- denormalised returns late in training -- on fresh value statistics and on statistics matched to an earlier batch;
normalize_value and normalize_advantage each on and off.

* Raw returns and advantages against the float64 recursion of a2c_common.py:525-540 (bootstrap: the float64 forward
  of the same parameters), at FACTOR x the error of the fp32 oracle (PO.discount_values behind PO.forward with the
  kernel's tanh model) on the same case, relative to the batch maximum.
* The value statistics against two-pass float64 (Chan merge, values then returns): count exact, mean within
  n eps mean|x|, variance never negative, and what the update sees -- formed in float64 from either side's
  statistics -- within 1e-5.
* The normalised values, returns and advantages the kernel stores, within 1e-5 of the float64 normalisation (two-pass
  statistics) of the fp32 returns and advantages the device itself holds before it normalises (the bits of a run
  with that normalisation off: one step from the device's own state, as in the optimiser tests; the raw arrays are
  judged above).  The one-pass fp64 variance of k_prepare_finalize holds: on the matched large-mean cases it is within
  4e-7 of the two-pass one, the normalised values formed from it within 9e-7.  What did not hold was
  k_prepare_apply's fp32 difference: x - (float)mean loses the mean's rounding, up to 3e-5 of a spread of 1e-2, and
  stored values 2.1e-3 and 2.3e-3 off at 257 x 16 and 257 x 24 (1.3e-5 at 1,000 x 16), advantages 8.5e-5 off at
  262,145 x 1 (normalize_value off: mean -1e3, spread 0.29).  Since this test the kernel takes the difference in
  double wherever |mean| exceeds 64 sd (1.05e-6 and 4.8e-7 at the worst on those cases) and keeps the reference's
  fp32 difference, bit for bit, below that, where its share is under 2^-24 x 64 = 4e-6; two cases sit either
  side of the switch, at 48 sd (fp32 difference: 1.3e-6) and at 76 sd (2.1e-7).

Rollout forward: stress and boundary parameters (saturated tanh, Wv x 8 so that the value passes its +-5 clamp),
observation statistics that put columns on the +-5 clip, val_rms = (0.3, 2.5); 1 and 33 envs, and 100 envs on 3
workgroups (a looped workgroup, a ragged last tile, the double-buffered draw); both USV_POLICY_RW forms."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import ppo_oracle as PO
from tests import errtab as ET
from tests import ppo_ref64 as R
from tests import test_ppo_gpu as TG

pytestmark = pytest.mark.gpu
F = np.float32
SENT = -7.25
PAD = 1024
SENT_BITS = int(F(SENT).view(np.int32))
GAE_TB = 256                  # envs per k_gae workgroup = partial rows of the finalize fold
CONSTS = {"yaml": (0.99, 0.95), "alt": (0.9, 0.5)}
# centre of the values with a spread of 1e-2: the large-mean family, and one on either side of |mean| = 64 sd (sd =
# sqrt(var + 1e-5) = 0.0105), where k_prepare_apply goes from the reference's fp32 difference to the double one
CENTRE = {"large": 1e3, "below64": 0.5, "above64": 0.8}
WIDE_RATIO = 64.0


def _dev():
    return TG.DEV


def _sync():
    if torch.device(_dev()).type == "cuda":
        torch.cuda.synchronize()


def _guarded(n, fill=SENT, dtype=torch.float32):
    t = torch.full((n + PAD,), SENT, device=_dev(), dtype=dtype)
    t[:n] = fill
    return t


def _pad_ok(t, n):
    if t.dtype == torch.float64:
        return bool((t[n:] == SENT).all())
    return bool((t[n:].view(torch.int32) == SENT_BITS).all())


def _np(t):
    return t.detach().cpu().numpy().copy()


_AGENT = []


def _cfg(n_envs, horizon, **fields):
    """A ppo_cfg_t of the yaml's (from a small agent, kept alive) with the shape and the given fields replaced."""
    from omniisaacgymenvs_loop_amd._abi import PpoCfg
    if not _AGENT:
        _AGENT.append(TG._agent(2, 32, mini_epochs=1))
    kc = PpoCfg.from_buffer_copy(_AGENT[0].cfg)
    kc.n_envs, kc.horizon, kc.nan_probe, kc.nan_flag = n_envs, horizon, 0, None
    assert kc.normalize_input == 1 and abs(kc.rms_eps - 1e-5) < 1e-12
    for k, v in fields.items():
        setattr(kc, k, v)
    return kc


# ---------------------------------------------------------------- the cases, built on the CPU
def _dones(kind, rng, N, H):
    d, last = np.zeros((N, H), np.uint8), np.zeros(N, np.int64)
    if kind == "all1":
        d[:], last[:] = 1, 1
    elif kind == "mixed":     # env 0: every slot; env 1: slot 0 only; env 2: slot H - 1 only; last_dones: every third
        d[0, :] = 1
        if N > 1:
            d[1, 0] = 1
        if N > 2:
            d[2, H - 1] = 1
        last[::3] = 1
        if N > 4:
            last[4] = 7       # any non-zero int64 is a done
    elif kind == "rand30":
        d[:] = rng.random((N, H)) < 0.3
        last[:] = rng.random(N) < 0.3
    else:
        assert kind == "all0"
    return d, last


class PrepCase:
    """Inputs of one ppo_prepare call and its float64 / fp32-oracle references (env-major [N, H])."""

    def __init__(self, N, H, dones, consts, family, start, seed=17):
        rng = np.random.default_rng(seed)
        self.N, self.H, self.family, self.start = N, H, family, start
        self.gamma, self.tau = (float(F(x)) for x in CONSTS[consts])
        self.P = R.stress_params(5)
        self.last_obs = rng.normal(0, 2, (N, PO.NIN)).astype(F)
        if family == "benign":
            self.val = rng.normal(0.5, 1.0, (N, H)).astype(F)
            self.rew = rng.normal(0.0, 0.2, (N, H)).astype(F)
        else:                 # a mean far from 0 over a small spread
            self.val = (CENTRE[family] + rng.normal(0, 1e-2, (N, H))).astype(F)
            self.rew = rng.normal(0, 1e-3, (N, H)).astype(F)
            v64 = self.val.astype(np.float64)
            assert family != "large" or abs(v64.mean()) / v64.std() > 3e4 or N * H < 32
        self.done, self.last_done = _dones(dones, rng, N, H)
        self.rms0 = (np.zeros(1), np.ones(1), 1.0)
        if start == "matched":   # the statistics of an earlier batch of the same family
            e = (CENTRE[family] + rng.normal(0, 1e-2, N * H)).astype(F).astype(np.float64)
            self.rms0 = (np.array([e.mean()]), np.array([((e - e.mean()) ** 2).sum() / (e.size - 1.0)]), float(e.size))
        self.obs_rms = (np.zeros(PO.NIN), np.ones(PO.NIN))

    # bootstrap value of the last observation: float64 forward / fp32 oracle forward with the kernel's tanh
    def last_val64(self, normalize_value):
        xn = R.norm64(self.last_obs, *self.obs_rms)
        v = R._forward64(self.P, xn)[1]
        if normalize_value:
            v = np.clip(v, -5.0, 5.0) * math.sqrt(self.rms0[1][0] + 1e-5) + self.rms0[0][0]
        return v

    def last_val32(self, normalize_value):
        o = PO.RMS(*self.obs_rms, 1.0)
        v = R._oracle_namespace(True, None)["forward"](self.P, o.norm(self.last_obs))[3]
        if normalize_value:
            v = PO.RMS(self.rms0[0], self.rms0[1], self.rms0[2]).denorm(v)
        return np.asarray(v, F)[:, 0]

    def gae64(self, normalize_value):
        """(returns, advantages) [N, H] by the recursion of a2c_common.py:525-540 in float64."""
        v, r = self.val.astype(np.float64), self.rew.astype(np.float64)
        nd, nl = 1.0 - self.done.astype(np.float64), 1.0 - (self.last_done != 0).astype(np.float64)
        adv, lam, lv = np.zeros_like(v), np.zeros(self.N), self.last_val64(normalize_value)
        for t in reversed(range(self.H)):
            nnt, nv = (nl, lv) if t == self.H - 1 else (nd[:, t + 1], v[:, t + 1])
            delta = r[:, t] + self.gamma * nv * nnt - v[:, t]
            adv[:, t] = lam = delta + self.gamma * self.tau * nnt * lam
        return adv + v, adv

    def gae32(self, normalize_value):
        """The fp32 oracle: PO.discount_values, returns = advs + values, advantages = returns - values."""
        hn = lambda a: np.ascontiguousarray(a.T)[:, :, None]
        advs = PO.discount_values(self.gamma, self.tau, (self.last_done != 0).astype(F),
                                  self.last_val32(normalize_value)[:, None], np.ascontiguousarray(self.done.T).astype(F),
                                  hn(self.val), hn(self.rew))
        ret = (advs + hn(self.val)).astype(F)
        adv = (ret - hn(self.val)).astype(F)
        return ret[:, :, 0].T, adv[:, :, 0].T


def _two_pass(x):
    x = np.asarray(x, np.float64).reshape(-1)
    m = x.mean()
    return m, ((x - m) ** 2).sum() / (x.size - 1.0) if x.size > 1 else float("nan")


class PrepRig:
    def __init__(self, case: PrepCase):
        from omniisaacgymenvs_loop_amd import _capi as c
        self.c, self.case = c, case
        N, B = case.N, case.N * case.H
        self.B = B
        T = lambda a, **k: torch.tensor(np.ascontiguousarray(a), device=_dev(), **k)
        self.params = T(PO.flatten(case.P))
        self.obs_rms = T(np.concatenate([case.obs_rms[0], case.obs_rms[1], [1.0]]))
        self.last_obs, self.last_done = T(case.last_obs), T(case.last_done)
        self.done, self.rew = T(case.done.reshape(-1)), T(case.rew.reshape(-1))
        self.nwork = 8 + 8 * 4096 + N // 2 + 64          # as a2c_continuous.py allocates it
        assert (N + GAE_TB - 1) // GAE_TB <= 4096

    def run(self, nv, na, vec=None, monkeypatch=None):
        c, case, B = self.c, self.case, self.B
        if vec is not None:
            monkeypatch.setenv("USV_GAE_VEC", str(vec))
        kc = _cfg(case.N, case.H, normalize_value=nv, normalize_advantage=na, gamma=case.gamma, tau=case.tau)
        assert float(kc.gamma) == case.gamma and float(kc.tau) == case.tau
        val, ret, adv = _guarded(B), _guarded(B), _guarded(B)
        val[:B].copy_(torch.tensor(case.val.reshape(-1), device=_dev()))
        work = _guarded(self.nwork, 0.0, torch.float64)
        rms = _guarded(3, 0.0, torch.float64)
        rms[:3].copy_(torch.tensor([case.rms0[0][0], case.rms0[1][0], case.rms0[2]], device=_dev(), dtype=torch.float64))
        for t in (val, ret, adv, work):
            assert t.data_ptr() % 16 == 0
        c.call("ppo_prepare", c.byref(kc), c.ptr(self.params), c.ptr(self.obs_rms), c.ptr(rms), c.ptr(self.last_obs),
               c.ptr(self.last_done), c.ptr(self.done), c.ptr(val), c.ptr(self.rew), c.ptr(ret), c.ptr(adv),
               c.ptr(work), c.stream_ptr())
        _sync()
        for name, t, n in (("val", val, B), ("ret", ret, B), ("adv", adv, B), ("work", work, self.nwork),
                           ("val_rms", rms, 3)):
            assert _pad_ok(t, n), f"floats behind {name} written"
        return {"val": _np(val[:B]), "ret": _np(ret[:B]), "adv": _np(adv[:B]), "rms": _np(rms[:3]),
                "stats": _np(work[:6])}


def _rel_max(x, x64):
    return float(np.abs(np.asarray(x, np.float64) - x64).max() / np.abs(x64).max())


def _norm64(x, mean, var):
    return np.clip((np.asarray(x, np.float64) - mean) / np.sqrt(var + 1e-5), -5.0, 5.0)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _check_raw(tn, case, out, normalize_value, ret=True):
    """Raw advantages (and returns) of a run against the float64 recursion at FACTOR x the fp32 oracle's error."""
    x64s, x32s = case.gae64(normalize_value), case.gae32(normalize_value)
    for q, got, x32, x64 in (("returns", out["ret"], x32s[0], x64s[0]), ("advantages", out["adv"], x32s[1], x64s[1])):
        if q == "returns" and not ret:
            continue
        model, err = _rel_max(x32.reshape(-1), x64.reshape(-1)), _rel_max(got, x64.reshape(-1))
        tol = R.FACTOR * model
        print(f"{tn}: raw {q}: kernel {err:.3g}, oracle {model:.3g}, tol {tol:.3g}, max |x| {np.abs(x64).max():.4g}")
        ET.record(tn, f"model {q}", model, 0.0)
        ET.record(tn, f"err/model {q}", err / model if model > 0 else float(err > 0), 0.0, tol=(f"<={R.FACTOR}", 0))
        assert np.isfinite(got).all() and err <= tol, f"{tn}: raw {q} {err:.3g} > {tol:.3g} ({R.FACTOR} x {model:.3g})"


def _check_adv_norm(tn, out, raw_adv):
    a = raw_adv.astype(np.float64)
    ma, va = _two_pass(a)
    want, st = (a - ma) / (math.sqrt(va) + 1e-8), out["stats"]
    print(f"{tn}: adv mean {st[4]:.9g} vs {ma:.9g}, std {st[5]:.9g} vs {math.sqrt(va):.9g}, "
          f"max |adv - adv64| {np.abs(out['adv'] - want).max():.3g}")
    ET.check(tn, "adv|stats", (a - st[4]) / (st[5] + 1e-8), want, 1e-5, 1e-5)
    ET.check(tn, "advantages", out["adv"], want, 1e-5, 1e-5)


def _check_prepare(tn, case: PrepCase, vec=None, monkeypatch=None):
    rig, B = PrepRig(case), case.N * case.H
    rms0 = [case.rms0[0][0], case.rms0[1][0], case.rms0[2]]
    v64 = case.val.reshape(-1).astype(np.float64)
    # ---- both switches off: the raw returns and advantages; nothing else moves
    raw = rig.run(0, 0, vec, monkeypatch)
    assert _same(raw["val"], case.val.reshape(-1)) and np.array_equal(raw["rms"], rms0)
    _check_raw(tn, case, raw, False)
    if B < 2:
        return
    # ---- normalize_advantage alone: the advantages of the run above, normalised; values, returns, val_rms stay
    out = rig.run(0, 1, vec, monkeypatch)
    assert _same(out["val"], raw["val"]) and _same(out["ret"], raw["ret"]) and np.array_equal(out["rms"], rms0)
    _check_adv_norm(f"{tn}_nv0na1", out, raw["adv"])
    # ---- normalize_value alone.  The bootstrap is now denormalised by the statistics before the merge, so this
    # run has raw arrays of its own: its advantages come out raw, and its raw returns are advantages + values (the
    # kernel forms adv = ret - val, exact whenever ret and val are within a factor of two -- the large-mean family
    # throughout -- and otherwise off by at most half an ulp of the advantage, 3e-8 of it)
    on = rig.run(1, 0, vec, monkeypatch)
    sub = f"{tn}_nv1na0"
    _check_raw(sub, case, on, True, ret=False)
    raw_adv = on["adv"].astype(np.float64)
    raw_ret = raw_adv + v64
    m1, s1, c1 = R.rms64(v64[:, None], *case.rms0)
    m2, s2, c2 = R.rms64(raw_ret[:, None], m1, s1, c1)
    got, st = on["rms"], on["stats"]
    assert got[2] == c2 == case.rms0[2] + 2 * B, "val_rms count"
    # fp64 sums in another order: n eps mean|x|.  After the returns, also what adv + val can miss the raw return
    # by: nothing where the two are provably within a factor of two (then the kernel's ret - val was exact), half
    # an ulp of the advantage elsewhere -- no such element in the large-mean family on matched statistics (on
    # fresh ones the bootstrap is within +-5 and the last slots' returns fall to it)
    a_v, a_r = np.abs(v64), np.abs(raw_ret)
    exact = (np.sign(raw_ret) == np.sign(v64)) & (a_r >= a_v / 1.9) & (a_r <= 1.9 * a_v)
    assert exact.all() or (case.family, case.start) != ("large", "matched")
    mean_tol_v = 2 * B * 2.0 ** -52 * float(a_v.mean())
    mean_tol = 2 * B * 2.0 ** -52 * float(np.concatenate([a_v, a_r]).mean()) \
        + float(np.abs(raw_adv[~exact]).sum()) * 2.0 ** -24 / c2
    print(f"{sub}: val_rms mean {got[0]:.13g} vs {m2[0]:.13g} (|d| {abs(got[0] - m2[0]):.3g}, tol {mean_tol:.3g}), var "
          f"{got[1]:.9g} vs {s2[0]:.9g}; after the values ({st[0]:.13g}, {st[1]:.9g}) vs ({m1[0]:.13g}, {s1[0]:.9g}; "
          f"|d| {abs(st[0] - m1[0]):.3g}, tol {mean_tol_v:.3g})")
    ET.record(sub, "var", np.array([st[1], got[1]]), np.array([s1[0], s2[0]]))
    assert abs(got[0] - m2[0]) <= mean_tol and abs(st[0] - m1[0]) <= mean_tol_v, "val_rms mean"
    assert got[1] >= 0 and st[1] >= 0, "negative variance"
    assert st[2] == got[0] and st[3] == got[1]
    # what the update sees, formed in float64 from either side's statistics ...
    ET.check(sub, "values|stats", _norm64(v64, st[0], st[1]), _norm64(v64, m1[0], s1[0]), 1e-5, 1e-5)
    ET.check(sub, "returns|stats", _norm64(raw_ret, got[0], got[1]), _norm64(raw_ret, m2[0], s2[0]), 1e-5, 1e-5)
    # ... and what the kernel stores
    dv = np.abs(on["val"] - _norm64(v64, m1[0], s1[0])).max()
    dr = np.abs(on["ret"] - _norm64(raw_ret, m2[0], s2[0])).max()
    print(f"{sub}: max |values - values64| {dv:.3g}, max |returns - returns64| {dr:.3g}")
    ET.check(sub, "values", on["val"], _norm64(v64, m1[0], s1[0]), 1e-5, 1e-5)
    ET.check(sub, "returns", on["ret"], _norm64(raw_ret, m2[0], s2[0]), 1e-5, 1e-5)
    # ---- both switches: the same values, returns and statistics, the advantages of that run normalised
    both = rig.run(1, 1, vec, monkeypatch)
    assert _same(both["val"], on["val"]) and _same(both["ret"], on["ret"]) and _same(both["rms"], on["rms"])
    _check_adv_norm(f"{tn}_nv1na1", both, on["adv"])


# N, H, USV_GAE_VEC (None: the horizon leaves only the loop), dones, constants, family, start of val_rms
PREP_CASES = [
    (1, 16, 1, "all0", "yaml", "benign", "fresh"),
    (1, 16, 0, "all1", "alt", "benign", "fresh"),
    (255, 16, 1, "rand30", "yaml", "benign", "fresh"),
    (255, 16, 0, "all0", "yaml", "benign", "fresh"),
    (257, 16, 1, "mixed", "alt", "benign", "fresh"),
    (257, 16, 0, "mixed", "yaml", "benign", "fresh"),
    (1000, 16, 1, "all1", "yaml", "benign", "fresh"),
    (1000, 16, 0, "rand30", "alt", "benign", "fresh"),
    (257, 8, None, "mixed", "yaml", "benign", "fresh"),
    (257, 24, None, "rand30", "alt", "benign", "fresh"),
    (262145, 1, None, "rand30", "yaml", "benign", "fresh"),
    (257, 16, 1, "all0", "yaml", "large", "fresh"),
    (257, 16, 1, "all0", "yaml", "large", "matched"),
    (1000, 16, 0, "all0", "alt", "large", "matched"),
    (257, 24, None, "all0", "yaml", "large", "matched"),
    (262145, 1, None, "all0", "yaml", "large", "fresh"),
    (262145, 1, None, "all0", "yaml", "large", "matched"),
    (257, 16, 1, "all0", "yaml", "below64", "matched"),
    (257, 16, 1, "all0", "yaml", "above64", "matched"),
]


@pytest.mark.parametrize("N,H,vec,dones,consts,family,start", PREP_CASES,
                         ids=["-".join(str(x) for x in p) for p in PREP_CASES])
def test_prepare_vs_float64(N, H, vec, dones, consts, family, start, monkeypatch):
    case = PrepCase(N, H, dones, consts, family, start)
    # the conditions on the case itself
    assert vec is not None or H % 16 != 0, "only a horizon of 16 has the vector form"
    if N == 262145:
        assert (N + GAE_TB - 1) // GAE_TB == 1025, "1,025 partial rows: the fold's second round (4 x 256 per round)"
    if dones == "mixed":
        assert case.done[0].all() and (N < 3 or (case.done[1].sum() == 1 and case.done[2, H - 1] == 1))
        assert N < 2 or 0 < (case.last_done != 0).sum() < N
    if dones == "rand30" and N > 100:
        assert 0.2 < case.done.mean() < 0.4
    if family in ("below64", "above64"):   # 48 and 76 sd: the fp32 difference at its worst, the double one at its start
        m1, s1, _ = R.rms64(case.val.reshape(-1).astype(np.float64)[:, None], *case.rms0)
        ratio = abs(m1[0]) / math.sqrt(s1[0] + 1e-5)
        assert (40 < ratio < 0.9 * WIDE_RATIO) if family == "below64" else (1.1 * WIDE_RATIO < ratio < 100), ratio
    _check_prepare(f"ppo_prep_{N}x{H}_{'loop' if not vec else 'vec'}_{dones}_{consts}_{family}_{start}", case,
                   vec, monkeypatch)


# ---------------------------------------------------------------- the rollout forward on the stress families
H_ROLL = 16
VAL_RMS = (0.3, 2.5, 10.0)


def _roll_case(family, N):
    """Parameters, raw observations, observation statistics and injected draws: rows of the family's 128-row case
    (those with a column on the +-5 clip first), its own two-pass statistics, Wv x 8 for values past +-5."""
    case = R.make_case(family, 128)
    mean, var, _ = R.rms64(case.obs)
    P = {k: v.copy() for k, v in case.P.items()}
    P["Wv"] = (P["Wv"] * F(8)).astype(F)
    xn = R.norm64(case.obs, mean, var)
    on_clip = (np.abs(xn) >= 5.0).any(1)
    # A single row is a fair case only where the oracle's own fp32 error is an ordinary one (a row the oracle happens
    # to hit exactly would leave the kernel FACTOR x nothing).  So the first row is the clip row, its value inside
    # the clamp, on which the smaller of the oracle's two misses (mu, value) is largest, each measured at the size
    # of the head's terms, sum |h2| |W| + |b|; the other clip rows follow, then the rest.
    mu64, v64 = R._forward64(P, xn)
    # (row by row: the oracle's matrix products sum in another order for another batch size)
    xn32, fwd = PO.RMS(mean, var, 129.0).norm(case.obs), R._oracle_namespace(True, None)["forward"]
    mu32, v32 = (np.concatenate([fwd(P, xn32[i:i + 1])[q] for i in range(len(xn32))]) for q in (2, 3))
    val64 = v64 * math.sqrt(VAL_RMS[1] + 1e-5) + VAL_RMS[0]
    val32 = PO.RMS(np.array([VAL_RMS[0]]), np.array([VAL_RMS[1]]), VAL_RMS[2]).denorm(v32)[:, 0]
    p64 = {k: np.asarray(v, np.float64) for k, v in P.items()}
    h2 = np.abs(np.tanh(np.tanh(xn @ p64["W1"].T + p64["b1"]) @ p64["W2"].T + p64["b2"]))
    s_mu = (h2 @ np.abs(p64["Wmu"]).T + np.abs(p64["bmu"])).max(1)
    s_v = (h2 @ np.abs(p64["Wv"]).T + np.abs(p64["bv"]))[:, 0] * math.sqrt(VAL_RMS[1] + 1e-5) + abs(VAL_RMS[0])
    miss = np.minimum(np.abs(mu32 - mu64).max(1) / s_mu, np.abs(val32 - val64) / s_v)
    miss = np.where(on_clip & (np.abs(v64) < 5.0), miss, -1.0)
    first = int(np.argmax(miss))
    assert miss[first] >= 2.0 ** -27, "no clip row on which the oracle misses float64 by an eighth of an ulp"
    key = np.where(np.arange(len(miss)) == first, 0, np.where(on_clip, 1, 2))
    order = np.argsort(key, kind="stable")
    obs = np.ascontiguousarray(case.obs[order][:N])
    eps = np.random.default_rng(N).normal(0, 1, (N, 2)).astype(F)
    return P, obs, mean, var, eps


@pytest.mark.parametrize("rw", ["1", "0"])
@pytest.mark.parametrize("N,grid", [(1, None), (33, None), (100, "3")])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_rollout_forward_vs_float64(family, N, grid, rw, monkeypatch):
    from omniisaacgymenvs_loop_amd import _capi as c
    monkeypatch.setenv("USV_POLICY_RW", rw)
    if grid:
        monkeypatch.setenv("USV_POLICY_GRID", grid)
        assert (N + 31) // 32 == 4 and int(grid) == 3      # 4 tiles of 32 rows on 3 workgroups, the last tile ragged
    else:
        monkeypatch.delenv("USV_POLICY_GRID", raising=False)
    P, obs, mean, var, eps = _roll_case(family, N)
    H, t = H_ROLL, 5
    kc = _cfg(N, H, normalize_value=1)
    T = lambda a, **k: torch.tensor(np.ascontiguousarray(a), device=_dev(), **k)
    params, obs_d, eps_d = T(PO.flatten(P)), T(obs), T(eps)
    obs_rms = T(np.concatenate([mean, var, [129.0]]))
    val_rms = T(np.array(VAL_RMS))
    dones_prev_np = (np.arange(N) % 3 == 1).astype(np.int64) * 5
    dones_prev = T(dones_prev_np)
    B = N * H
    bufs = {"obs": _guarded(B * PO.NIN), "act": _guarded(B * 2), "nlp": _guarded(B), "val": _guarded(B),
            "mu": _guarded(B * 2), "sigma": _guarded(B * 2), "actions": _guarded(N * 2), "values": _guarded(N)}
    done = torch.full((B + PAD,), 0xA5, device=_dev(), dtype=torch.uint8)
    c.call("ppo_policy_step", c.byref(kc), c.ptr(params), c.ptr(obs_rms), c.ptr(val_rms), c.ptr(obs_d), t,
           c.ptr(bufs["obs"]), c.ptr(bufs["act"]), c.ptr(bufs["nlp"]), c.ptr(bufs["val"]), c.ptr(bufs["mu"]),
           c.ptr(bufs["sigma"]), c.ptr(done), c.ptr(dones_prev), c.ptr(bufs["actions"]), 1, 0, None, c.ptr(eps_d),
           c.stream_ptr())
    c.call("ppo_value", c.byref(kc), c.ptr(params), c.ptr(obs_rms), c.ptr(val_rms), c.ptr(obs_d), c.ptr(bufs["values"]),
           c.stream_ptr())
    _sync()
    # ---- float64 forward and the fp32 oracle forward with the kernel's tanh
    xn = R.norm64(obs, mean, var)
    mu64, v64 = R._forward64(P, xn)
    logstd = np.asarray(P["sigma"], np.float64)
    sigma64 = np.exp(logstd) * np.ones_like(mu64)
    sd = math.sqrt(VAL_RMS[1] + 1e-5)
    val64 = np.clip(v64, -5.0, 5.0) * sd + VAL_RMS[0]
    orms = PO.RMS(mean, var, 129.0)
    _, _, mu32, v32 = R._oracle_namespace(True, None)["forward"](P, orms.norm(obs))
    val32 = PO.RMS(np.array([VAL_RMS[0]]), np.array([VAL_RMS[1]]), VAL_RMS[2]).denorm(v32)[:, 0]
    # the regime, on the float64 forward: a column on the clip, saturated units, values on either side of the clamp
    assert (np.abs(xn[0]) >= 5.0).any(), "the first row has no observation on the +-5 clip"
    if N >= 33:
        assert (np.abs(v64) > 5.0).any() and (np.abs(v64) < 5.0).any(), "the value clamp is not straddled"
        z1 = xn @ np.asarray(P["W1"], np.float64).T + P["b1"]
        assert np.abs(z1).max() > 6
    # ---- slot t of every env written, every other slot untouched, nothing behind the buffers
    slot = np.arange(N) * H + t
    others = np.setdiff1d(np.arange(B), slot)

    def rows(name, width):
        a = _np(bufs[name][:B * width]).reshape(B, width)
        assert (a[others].view(np.int32) == SENT_BITS).all(), f"{name}: another slot written"
        return a[slot]
    for name, t_, n in [(k, v, {"obs": B * PO.NIN, "act": B * 2, "mu": B * 2, "sigma": B * 2, "actions": N * 2,
                                "values": N}.get(k, B)) for k, v in bufs.items()]:
        assert _pad_ok(t_, n), f"floats behind {name} written"
    dn = _np(done)
    assert (dn[B:] == 0xA5).all() and (dn[:B][others] == 0xA5).all()
    np.testing.assert_array_equal(dn[:B][slot], (dones_prev_np != 0).astype(np.uint8))
    assert _same(rows("obs", PO.NIN), obs), "exp_obs is not the observation bit for bit"
    mu, sigma, act = rows("mu", 2), rows("sigma", 2), rows("act", 2)
    val, nlp = rows("val", 1)[:, 0], rows("nlp", 1)[:, 0]
    tn = f"ppo_roll_{family}_{N}_rw{rw}"
    for q, got, x32, x64 in (("mu", mu, mu32, mu64), ("value", val, val32, val64),
                             ("ppo_value", _np(bufs["values"][:N]), val32, val64)):
        model, err = float(np.abs(x32 - x64).max()), float(np.abs(got - x64).max())
        print(f"{tn}: {q}: kernel {err:.3g}, oracle {model:.3g}, tol {R.FACTOR * model:.3g}")
        ET.record(tn, f"model {q}", model, 0.0)
        ET.record(tn, f"err/model {q}", err / model if model > 0 else float(err > 0), 0.0, tol=(f"<={R.FACTOR}", 0))
        assert np.isfinite(got).all() and err <= R.FACTOR * model, f"{tn}: {q} {err:.3g} > {R.FACTOR} x {model:.3g}"
    ET.check(tn, "sigma", sigma, sigma64, 1e-5, 1e-5, ["s0", "s1"])
    ET.check(tn, "action", act, mu64 + sigma64 * eps, 1e-5, 1e-5, ["a0", "a1"])
    # neglogp of the fp32 action the kernel stored (models.py:400)
    z = (act.astype(np.float64) - mu64) / sigma64
    ET.check(tn, "neglogp", nlp, 0.5 * (z ** 2).sum(-1) + 0.5 * math.log(2 * math.pi) * 2 + logstd.sum(), 1e-5, 1e-5)
    assert _same(_np(bufs["actions"][:N * 2]).reshape(N, 2), np.clip(act, F(-1), F(1))), "actions_out != clamp(action)"


