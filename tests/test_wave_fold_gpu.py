"""The cross-lane folds of csrc/usv_device.h (wave_sum / wave_max / wave_min, the 16- and 8-lane ascending sums, the
cross-half pair sum) in their DPP / lane-swap forms against the shuffle forms they replaced, through
usv_wave_fold_selftest: the same partner at every level in the same order, so EVERY lane's result has the same bits.

Inputs: 64 lanes x k waves (k <= 64), one launch per case."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = ("sum64", "max64", "min64", "sum16", "sum8", "pair32")
K = 64


def _cases():
    rng = np.random.default_rng(20)
    n = 64 * K
    out = {}
    # seeded normals spread over 30 binades
    out["normals_30_binades"] = (rng.normal(0, 1, n) * np.exp2(rng.integers(-15, 15, n))).astype(np.float32)
    # mixed signs with cancellation: every value next to its negation plus a small remainder
    big = (rng.normal(0, 1, n // 2) * 1e6).astype(np.float32)
    canc = np.empty(n, np.float32)
    canc[0::2] = big
    canc[1::2] = -big + rng.normal(0, 1e-3, n // 2).astype(np.float32)
    out["cancellation"] = rng.permutation(canc.reshape(K, 64), axis=1).reshape(-1)
    # +0 / -0 only (wave 0 all -0, wave 1 all +0, the rest mixed), and zeros among values
    z = np.where(rng.integers(0, 2, n) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    z[:64] = -0.0
    z[64:128] = 0.0
    out["signed_zeros"] = z
    zv = out["normals_30_binades"].copy()
    zv[rng.integers(0, 3, n) == 0] = -0.0
    out["zeros_among_values"] = zv
    # denormals: alone, and beside the smallest normals
    den = (rng.integers(1, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31))
    out["denormals"] = den.view(np.float32)
    mix = out["denormals"].copy()
    mix[::5] = np.float32(1.1754944e-38) * rng.choice(np.array([-1, 1], np.float32), len(mix[::5]))
    out["denormals_and_min_normals"] = mix
    # +inf / -inf in a few lanes of finite values: waves with +inf only, -inf only (sums stay infinite) and, from
    # wave 32 on, both (sums NaN -- compared through the NaN masks)
    inf = rng.normal(0, 1, n).astype(np.float32).reshape(K, 64)
    for w in range(K):
        lanes = rng.choice(64, 3, replace=False)
        inf[w, lanes[0]] = np.inf if w % 2 == 0 or w >= 32 else -np.inf
        if w >= 32:
            inf[w, lanes[1]] = -np.inf
    out["infinities"] = inf.reshape(-1)
    # one quiet NaN in one lane of every wave (lane w: every position once)
    nan = rng.normal(0, 1, n).astype(np.float32).reshape(K, 64)
    for w in range(K):
        nan[w, w] = np.float32(np.nan)
    out["one_quiet_nan"] = nan.reshape(-1)
    return out


CASES = _cases()


def _run(x):
    from omniisaacgymenvs_loop_amd import _capi as c
    k = x.size // 64
    xin = torch.tensor(x, device=DEV)
    assert torch.equal(xin.view(torch.int32).cpu(), torch.tensor(x.view(np.int32)))   # the bits went up unchanged
    new = torch.full((len(ROWS), k * 64), -7.25, device=DEV)
    old = torch.full((len(ROWS), k * 64), -9.5, device=DEV)
    c.call("usv_wave_fold_selftest", c.ptr(xin), k, c.ptr(new), c.ptr(old), c.stream_ptr())
    torch.cuda.synchronize()
    return new.cpu().numpy(), old.cpu().numpy()


@pytest.mark.parametrize("case", sorted(CASES))
def test_dpp_folds_have_the_shuffle_folds_bits_in_every_lane(case):
    x = CASES[case]
    new, old = _run(x)
    nan_new, nan_old = np.isnan(new), np.isnan(old)
    for r, name in enumerate(ROWS):
        assert np.array_equal(nan_new[r], nan_old[r]), f"{case} {name}: NaN lanes differ"
        ok = ~nan_old[r]
        a, b = new[r].view(np.int32)[ok], old[r].view(np.int32)[ok]
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (f"{case} {name}: {bad.size} lanes differ, first at {np.flatnonzero(ok)[bad[0]]}: "
                               f"{a[bad[0]]:#x} vs {b[bad[0]]:#x}")
    if case not in ("one_quiet_nan", "infinities"):
        assert not nan_old.any(), case
    # the result is the whole group's in all of its lanes
    for r, width in ((0, 64), (1, 64), (2, 64), (3, 16), (4, 8)):
        g = new[r].view(np.int32).reshape(-1, width)
        same = (g == g[:, :1]) | np.isnan(new[r].reshape(-1, width))
        assert same.all(), f"{case} {ROWS[r]}: lanes of one group disagree"


def test_shuffle_folds_are_the_stated_butterfly():
    """The shuffle forms (the reference above) are themselves the butterfly this float32 restatement spells out:
    partners 32, 16, .., 1 for the 64-lane folds, 1, 2, 4 (, 8) for the group sums -- on the finite case."""
    x = CASES["normals_30_binades"]
    _, old = _run(x)
    lane = np.arange(64)

    def fold(v, offs, op):
        v = v.reshape(-1, 64).copy()
        for m in offs:
            v = op(v, v[:, lane ^ m]).astype(np.float32)
        return v.reshape(-1)

    down = (32, 16, 8, 4, 2, 1)
    want = (fold(x, down, np.add), fold(x, down, np.maximum), fold(x, down, np.minimum), fold(x, (1, 2, 4, 8), np.add),
            fold(x, (1, 2, 4), np.add), fold(x, (32,), np.add))
    for r, name in enumerate(ROWS):
        assert np.array_equal(old[r].view(np.int32), want[r].view(np.int32)), name
