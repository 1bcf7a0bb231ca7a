"""The analysis stage on the host: the numpy restatement of the reference's analysis tool (tests/analysis_restate.py)
fed the recorded index draws against the fixture the tool itself produced (tests/golden/analysis_golden.npz) bit
for bit, the Philox index rule against hand-computed words, the argument statuses of the three entry points
(csrc/usv_analysis.hip) without a device, and the compare_policies overrides."""
import ctypes
import os

import numpy as np
import pytest

from omniisaacgymenvs_loop_amd._abi import DEFINES as D
from tests import analysis_restate as AR


@pytest.fixture(scope="module")
def fx(golden):
    return golden("analysis_golden.npz")


def frame_of(fx, tag):
    pre = f"{tag}_frame_"
    return {k[len(pre):]: fx[k] for k in fx if k.startswith(pre)}


def streams(fx, key):
    flat, off = fx[f"{key}_draws"], fx[f"{key}_draws_off"]
    return {name: AR.Replay(flat[off[i]:off[i + 1]]) for i, name in enumerate(AR.METRIC_NAMES)}


def same(a, b, msg=""):
    """Equal bit for bit, NaN equal to NaN."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), msg
    assert np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64)), (msg, a, b)


def test_fixture_frames_are_the_builders(fx):
    """The fixture's inputs are what the tests build their tables from, and they hold the cases the issue names."""
    for tag, (frame, S, R) in (("a", AR.frame_a()), ("b", AR.frame_b())):
        got = frame_of(fx, tag)
        assert set(got) == set(frame) and fx[f"{tag}_SR"].tolist() == [S, R]
        for k in frame:
            same(got[k], frame[k], k)
    f, S, R = AR.frame_a()
    t, c = f["group"] == AR.TREAT, f["group"] == AR.CONTROL
    assert 4 not in f["scene_idx"][t] and 9 not in f["scene_idx"][c]                 # a scene missing in one group
    assert (f["scene_idx"][t] == 11).sum() == R - 1                                   # a rollout missing
    assert not f["success"][c & (f["scene_idx"] == 6)].any()                          # fails in every rollout
    assert np.array_equal(np.isnan(f["time_to_goal_sec"]), f["success"] == 0.0)      # NaN on failures
    assert fx["b_pair_n"].tolist()[-3:] == [1, 1, 0]                                  # the n = 1 and n = 0 rules


@pytest.mark.parametrize("tag", ["a", "b"])
def test_paired_restatement_equals_the_reference(fx, tag):
    frame, n_boot = frame_of(fx, tag), int(fx["settings"][0])
    rngs = streams(fx, f"{tag}_pair")
    rows = AR.paired(frame, n_boot, rngs)
    assert [r[0] for r in rows] == list(AR.METRIC_NAMES)
    assert [r[1] for r in rows] == fx[f"{tag}_pair_n"].tolist()
    for i, k in enumerate(("diff", "lo", "hi")):
        same([r[2 + i] for r in rows], fx[f"{tag}_pair_{k}"], k)
    assert all(r.pos == len(r.flat) for r in rngs.values())   # every recorded draw was used


def test_unpaired_restatement_equals_the_reference(fx):
    frame, n_boot = frame_of(fx, "a"), int(fx["settings"][1])
    rngs = streams(fx, "a_unp")
    rows = AR.unpaired(frame, n_boot, rngs)
    assert [r[1] for r in rows] == fx["a_unp_nt"].tolist() and [r[2] for r in rows] == fx["a_unp_nc"].tolist()
    for i, k in enumerate(("diff", "lo", "hi")):
        same([r[3 + i] for r in rows], fx[f"a_unp_{k}"], k)
    assert all(r.pos == len(r.flat) for r in rngs.values())


def test_stratified_restatement_equals_the_reference(fx):
    frame = frame_of(fx, "a")
    _, _, n_boot, n_bins, min_per_bin, _ = (int(v) for v in fx["settings"])
    rng = AR.Replay(fx["a_strat_draws"])
    rows = AR.stratified(frame, AR.STRATA_A, n_bins, min_per_bin, n_boot, rng)
    assert rng.pos == len(rng.flat)
    assert [AR.STRATA_A.index(r["strat_col"]) for r in rows] == fx["a_strat_col"].tolist()
    assert "d_const" not in {r["strat_col"] for r in rows}          # fewer than 3 edges
    for c in AR.STRAT_COLUMNS[4:]:
        if c in ("bin", "n", "n_treat", "n_control"):
            assert [r[c] for r in rows] == fx[f"a_strat_{c}"].tolist(), c
        else:
            same([r[c] for r in rows], fx[f"a_strat_{c}"], c)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_pair_deltas_restatement_on_tables(tag):
    """usv_ana_pair_deltas' numpy restatement on the tables built from a frame gives the reference's per-scene deltas
    (NaN where it skips the scene): the tables carry what the frame holds."""
    frame, S, R = AR.frame_a() if tag == "a" else AR.frame_b()
    tabs = AR.frame_tables(frame, S, R)
    n = tabs[AR.CONTROL][0].shape[1]
    got = AR.pair_deltas_host(*tabs[AR.CONTROL], *tabs[AR.TREAT], n, S, R, 1, AR.REWARD_SCALE)
    same(got, AR.pair_delta_rows(frame, S))


def test_philox_words_and_the_index_rule():
    """Philox4x32-10 against the published known-answer vectors, and the index rule worked by hand on them:
    idx = (word * len) >> 32."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        assert tuple(int(w) for w in AR.philox4x32_10(ctr, key)) == want
    # 0x6627E8D5 / 2^32 = 0.39904..., so len 1000 -> 399; 0x9B00DBD8 / 2^32 = 0.60548... -> 605
    assert (0x6627E8D5 * 1000) >> 32 == 399 and (0x9B00DBD8 * 1000) >> 32 == 605
    seed, j, b, length = 0x1234567890ABCDEF, 3, 5, 11
    got = AR.philox_indices(seed, j, b, length)
    want = []
    for i in range(length):
        w = AR.philox4x32_10((i >> 2, b, j, D["USV_ANA_SITE"]), (seed & 0xFFFFFFFF, seed >> 32))
        want.append((int(w[i & 3]) * length) >> 32)
    assert got.tolist() == want and min(want) >= 0 and max(want) < length
    assert AR.philox_indices(seed, j, b, 0).shape == (0,) and AR.philox_indices(seed, j, b, 1).tolist() == [0]
    # the project's other host Philox (scenario.sampling) agrees
    from omniisaacgymenvs_loop_amd.scenario.sampling import _philox
    w2 = _philox()((np.arange(3, dtype=np.uint64), b, j, D["USV_ANA_SITE"]), (seed & 0xFFFFFFFF, seed >> 32))
    w1 = AR.philox4x32_10((np.arange(3, dtype=np.uint64), b, j, D["USV_ANA_SITE"]), (seed & 0xFFFFFFFF, seed >> 32))
    assert all(np.array_equal(np.asarray(a, np.uint64), np.asarray(c, np.uint64)) for a, c in zip(w1, w2))
    # the largest index bias of the multiply-shift rule is len / 2^32: every index is reachable at len = 2^26
    assert (0xFFFFFFFF * D["USV_SCN_MAX_COUNT"]) >> 32 == D["USV_SCN_MAX_COUNT"] - 1


def test_lerp_rule_is_numpys():
    """The quantile rule usv_ana_quantiles states (include/usv_hip.h) gives np.quantile's bits."""
    rng = np.random.default_rng(5)
    for m in (1, 2, 31, 2000):
        v = np.sort(rng.normal(size=m))
        for q in (0.0, 0.025, 0.5, 0.975, 1.0, 1.0 / 3.0):
            pos = q * (m - 1)
            lo = int(np.floor(pos))
            g, a, b = pos - lo, v[lo], v[min(lo + 1, m - 1)]
            got = a + (b - a) * g if g < 0.5 else b - (b - a) * (1.0 - g)
            same([got], [np.quantile(v, q)], (m, q))


def _lib():
    from omniisaacgymenvs_loop_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libusv_hip.so not built (run __graft_entry__.build())")
    return _capi.lib()


def test_argument_statuses():
    """1 = a NULL or out-of-range argument, 2 = an unsupported size, before any device work (there is no device
    here: the pointers are host scratch that is never dereferenced on the device)."""
    from omniisaacgymenvs_loop_amd._abi import UsvEval
    lib = _lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf) % 16)

    def ev(K=1, episodes=p):
        e = UsvEval()
        e.acc, e.episodes, e.ep_count, e.max_episodes, e.action_scale, e.control_dt = None, episodes, p, K, 1.0, 0.2
        return e

    def deltas(c=None, t=None, n=8, S=3, R=2, K=1, out=p):
        c, t = c or ev(), t or ev()
        return lib.usv_ana_pair_deltas(ctypes.byref(c), ctypes.byref(t), n, S, R, K, 1.0, out, None)

    assert lib.usv_ana_pair_deltas(None, ctypes.byref(ev()), 8, 3, 2, 1, 1.0, p, None) == 1
    assert deltas(out=None) == 1 and deltas(S=0) == 1 and deltas(c=ev(episodes=None)) == 1
    assert deltas(K=2) == 2                        # K != ceil(S R / n)
    assert deltas(t=ev(K=2)) == 2                  # the two tables keep different max_episodes
    assert deltas(S=D["USV_SCN_MAX_COUNT"] + 1) == 2

    def off(*v):
        a = np.asarray(v, np.int64)
        return a, a.ctypes.data_as(ctypes.c_void_p)

    def boot(values=p, seg=(0, 4, 9), J=2, B=7, inj=None, inj_off=None, idx_out=None, means=p):
        keep, seg_p = off(*seg)
        keep2, inj_p = off(*inj_off) if inj_off is not None else (None, None)
        return lib.usv_ana_bootstrap(values, seg_p, J, B, 1, inj, inj_p, idx_out, means, None)

    assert boot(values=None) == 1 and boot(means=None) == 1 and boot(J=0) == 1 and boot(B=0) == 1
    assert lib.usv_ana_bootstrap(p, None, 2, 7, 1, None, None, None, p, None) == 1
    assert boot(seg=(0, 4, 3)) == 1                                            # offsets that decrease
    assert boot(inj=p) == 1 and boot(idx_out=p) == 1                           # without inj_off
    assert boot(inj=p, inj_off=(0, 28, 62)) == 1                               # 34 < B len = 35
    assert boot(B=D["USV_ANA_MAX_BOOT"] + 1) == 2
    assert boot(seg=(0, 4, 4 + D["USV_SCN_MAX_COUNT"] + 1)) == 2

    def quant(x=p, J=2, B=7, q=p, nq=2, mode=D["USV_ANA_NAN_PROPAGATE"], out=p):
        return lib.usv_ana_quantiles(x, J, B, q, nq, mode, out, None)

    assert quant(x=None) == 1 and quant(q=None) == 1 and quant(out=None) == 1
    assert quant(J=0) == 1 and quant(B=0) == 1 and quant(nq=0) == 1 and quant(mode=2) == 1
    assert quant(B=D["USV_ANA_MAX_BOOT"] + 1) == 2 and quant(nq=D["USV_ANA_MAX_Q"] + 1) == 2


def test_compare_policies_overrides_parse_and_default_to_off():
    from omniisaacgymenvs_loop_amd.scripts import compare_policies as CP
    opt, rest = CP.split_overrides(CP.parse_overrides(["scenario_npz=x.npz", "num_envs=64"]))
    assert rest == {"num_envs": 64}
    a = CP.analysis_options(opt)
    assert a == {"n_boot": 0, "strata": [], "n_bins": 5, "min_per_bin": 5, "seed": 0}
    opt, _ = CP.split_overrides(CP.parse_overrides([
        "compare.bootstrap=16", "compare.strata=straight_line_dist,d_spawn,d_goal,d_corr,d_oo,density,start_speed",
        "compare.n_bins=4", "compare.min_per_bin=3", "compare.boot_seed=9"]))
    a = CP.analysis_options(opt)
    assert a == {"n_boot": 16, "strata": list(CP.STRATA), "n_bins": 4, "min_per_bin": 3, "seed": 9}
    with pytest.raises(SystemExit):
        CP.analysis_options(CP.split_overrides(CP.parse_overrides(["compare.strata=altitude"]))[0])
    with pytest.raises(SystemExit):
        CP.analysis_options(CP.split_overrides(CP.parse_overrides(["compare.bootstrap=5000"]))[0])
    with pytest.raises(SystemExit):
        CP.split_overrides(CP.parse_overrides(["compare.boot=16"]))
    assert sorted(CP.ANALYSIS_FILES.values()) == ["layer0_paired_summary.csv", "layer0_summary.csv",
                                                  "stratified_effects.csv"]
