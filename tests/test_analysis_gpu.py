"""The analysis stage on the device: usv_ana_pair_deltas, usv_ana_bootstrap and usv_ana_quantiles
(csrc/usv_analysis.hip) against their host restatements (tests/analysis_restate.py) and numpy, and
scenario.analysis / scripts.compare_policies end to end on the fixture the reference's tool produced
(tests/golden/analysis_golden.npz) with its recorded index draws injected."""
import csv
import json
import os
import warnings

import numpy as np
import pytest
import torch

from omniisaacgymenvs_loop_amd._abi import DEFINES as D
from tests import analysis_restate as AR
from tests import compare_restate as CR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE20 = os.path.join(ROOT, "tests", "golden", "scenario_pre20.npz")
DEV = "cuda:0"
EPS = 2.0 ** -52
LDS = D["USV_ANA_LDS_DOUBLES"]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_nan(a, b, msg=""):
    assert np.array_equal(np.isnan(a), np.isnan(b)), msg


class Arm:
    """What scenario.compare.ArmTable holds, from host arrays."""

    def __init__(self, tab, cnt, K):
        from omniisaacgymenvs_loop_amd import _capi
        from omniisaacgymenvs_loop_amd._abi import UsvEval
        self.table, self.ep_count = torch.tensor(tab, device=DEV), torch.tensor(cnt, device=DEV)
        ev = UsvEval()
        ev.acc, ev.episodes, ev.ep_count = None, _capi.ptr(self.table), _capi.ptr(self.ep_count)
        ev.max_episodes, ev.action_scale, ev.control_dt = K, 1.0, 0.2
        self.ev = ev


@pytest.fixture(scope="module")
def fx(golden):
    return golden("analysis_golden.npz")


def frame_arms(tag):
    frame, S, R = AR.frame_a() if tag == "a" else AR.frame_b()
    tabs = AR.frame_tables(frame, S, R)
    n = tabs[AR.CONTROL][0].shape[1]
    return frame, S, R, n, tabs, Arm(*tabs[AR.CONTROL], 1), Arm(*tabs[AR.TREAT], 1)


# ------------------------------------------------------------------------------------------ usv_ana_pair_deltas
def check_deltas(control, treat, tabs, n, S, R, K, scale):
    from omniisaacgymenvs_loop_amd.scenario import analysis as A
    want = AR.pair_deltas_host(*tabs[0], *tabs[1], n, S, R, K, scale)
    got = A.pair_deltas(control, treat, n, S, R, K, scale).cpu().numpy()
    assert got.shape == (D["USV_ANA_PD_ROWS"], S)
    same_nan(got, want)
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-12, atol=0)
    again = A.pair_deltas(control, treat, n, S, R, K, scale).cpu().numpy()
    assert np.array_equal(bits(again), bits(got))
    return got, want


@pytest.mark.parametrize("S,R,K,n,missing", [(3, 2, 1, 8, ()), (5, 3, 2, 8, (7,))])
def test_pair_deltas_on_hand_tables(S, R, K, n, missing):
    (ta, ca), (tb, cb) = CR.hand_tables(S, R, K, n, missing_in_b=missing)
    got, want = check_deltas(Arm(ta, ca, K), Arm(tb, cb, K), ((ta, ca), (tb, cb)), n, S, R, K, 0.37)
    assert np.isfinite(want[D["USV_ANA_PD_RET_RAW"]]).all()           # every scenario keeps a row on both sides
    assert np.isnan(want[D["USV_ANA_PD_TIME_SUCC"]:]).any()           # ... but not a finite success-only mean


@pytest.mark.parametrize("tag", ["a", "b"])
def test_pair_deltas_on_the_fixture_frames(fx, tag):
    frame, S, R, n, tabs, control, treat = frame_arms(tag)
    got, want = check_deltas(control, treat, (tabs[AR.CONTROL], tabs[AR.TREAT]), n, S, R, 1, AR.REWARD_SCALE)
    ref = AR.pair_delta_rows(frame, S)                                # the reference's own deltas
    same_nan(got, ref)
    np.testing.assert_allclose(got[~np.isnan(ref)], ref[~np.isnan(ref)], rtol=1e-12, atol=0)
    assert (~np.isnan(got)).sum(1).tolist() == fx[f"{tag}_pair_n"].tolist()
    from omniisaacgymenvs_loop_amd import _capi
    other = Arm(*tabs[AR.TREAT], 2)
    out = torch.zeros((D["USV_ANA_PD_ROWS"], S), device=DEV, dtype=torch.float64)
    assert _capi.call_rc("usv_ana_pair_deltas", _capi.byref(control.ev), _capi.byref(other.ev), n, S, R, 1, 1.0,
                         _capi.ptr(out), _capi.stream_ptr()) == 2


# ------------------------------------------------------------------------------------------ usv_ana_bootstrap
def segments():
    """Lengths 0, 1, 2, 63, 64, 65 and 1000, a segment with NaNs, an all-NaN one, one an element longer than the LDS
    staging capacity and one of exactly that capacity (the last that is staged: the whole 128 KB)."""
    rng = np.random.default_rng(11)
    lens = [0, 1, 2, 63, 64, 65, 1000, 50, 5, LDS + 1, LDS]
    segs = [rng.normal(3.0, 40.0, n) for n in lens]
    segs[7][::3] = np.nan
    segs[8][:] = np.nan
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return np.concatenate(segs), off


def seg_bound(values, off):
    """len x 2^-52 x max|v| per segment: both means are sums of len doubles, each within len x 2^-53 x max|v|."""
    out = []
    for j in range(len(off) - 1):
        v = values[off[j]:off[j + 1]]
        v = v[np.isfinite(v)]
        out.append(len(values[off[j]:off[j + 1]]) * EPS * (np.abs(v).max() if v.size else 0.0))
    return np.asarray(out)


def check_means(got, want, bound):
    same_nan(got, want)
    err = np.abs(np.where(np.isnan(want), 0.0, got - want))
    assert (err <= bound[:, None]).all(), (err.max(1), bound)


@pytest.mark.parametrize("B", [1, 7, 64])
def test_bootstrap_injected_draws(B):
    from omniisaacgymenvs_loop_amd.scenario import analysis as A
    values, off = segments()
    lens = np.diff(off)
    rng = np.random.default_rng(100 + B)
    inj = [rng.integers(0, max(n, 1), size=(B, n)) for n in lens]
    inj_off = np.concatenate([[0], np.cumsum(B * lens)]).astype(np.int64)
    inj_dev = torch.tensor(np.concatenate([i.reshape(-1) for i in inj]).astype(np.int32), device=DEV)
    got = A.bootstrap_means(torch.tensor(values, device=DEV), off, B, inject=(inj_dev, inj_off)).cpu().numpy()
    want = AR.bootstrap_means_host(values, off, lambda j, b, n: inj[j][b], B)
    check_means(got, want, seg_bound(values, off))
    assert np.isnan(got[0]).all() and np.isnan(got[8]).all()          # len = 0 and all-NaN: NaN exactly
    assert np.array_equal(bits(got[1]), bits(np.full(B, values[off[1]])))   # len = 1: the value itself
    assert np.isfinite(got[[2, 3, 4, 5, 6, 9, 10]]).all()


def test_bootstrap_injected_index_outside_the_segment_is_a_nan_draw():
    from omniisaacgymenvs_loop_amd.scenario import analysis as A
    v = torch.tensor([1.0, 2.0, 4.0], device=DEV, dtype=torch.float64)
    inj = torch.tensor([0, 3, 2, -1, -1, 7], device=DEV, dtype=torch.int32)
    got = A.bootstrap_means(v, [0, 3], 2, inject=(inj, [0, 6])).cpu().numpy()
    assert got[0, 0] == 2.5 and np.isnan(got[0, 1])


def test_bootstrap_philox():
    """idx_out is the host Philox restatement exactly (every index, every segment, B = 7), the means are the host
    means over those indices, the same seed gives the same bits, another seed other ones, and idx_out = NULL
    changes nothing."""
    from omniisaacgymenvs_loop_amd.scenario import analysis as A
    values, off = segments()
    lens, B, seed = np.diff(off), 7, 0x1234567890ABCDEF
    inj_off = np.concatenate([[0], np.cumsum(B * lens)]).astype(np.int64)
    vd = torch.tensor(values, device=DEV)
    idx = torch.full((int(inj_off[-1]),), -7, device=DEV, dtype=torch.int32)
    got = A.bootstrap_means(vd, off, B, seed, inject=(None, inj_off), idx_out=idx).cpu().numpy()
    idx = idx.cpu().numpy()
    want_idx = {(j, b): AR.philox_indices(seed, j, b, int(lens[j])) for j in range(len(lens)) for b in range(B)}
    for (j, b), w in want_idx.items():
        g = idx[inj_off[j] + b * lens[j]:inj_off[j] + (b + 1) * lens[j]]
        assert np.array_equal(g, w), (j, b)
    assert len({tuple(want_idx[(6, b)]) for b in range(B)}) == B       # the replicates differ
    want = AR.bootstrap_means_host(values, off, lambda j, b, n: want_idx[(j, b)], B)
    check_means(got, want, seg_bound(values, off))
    plain = A.bootstrap_means(vd, off, B, seed).cpu().numpy()
    assert np.array_equal(bits(plain), bits(got))
    assert np.array_equal(bits(A.bootstrap_means(vd, off, B, seed).cpu().numpy()), bits(plain))
    other = A.bootstrap_means(vd, off, B, seed + 1).cpu().numpy()
    assert all(not np.array_equal(bits(other[j]), bits(plain[j])) for j in (6, 9, 10))


def test_bootstrap_gathered_segments_past_the_l2_size():
    """Two segments of 300,000 doubles (4.8 MB together: past the 4 MiB at which the gathered launch holds one
    workgroup per CU) beside a staged one, B = 1: indices and means against the host restatement."""
    from omniisaacgymenvs_loop_amd.scenario import analysis as A
    rng = np.random.default_rng(31)
    lens = np.asarray([300000, 100, 300000], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    values, B, seed = rng.normal(1.0, 20.0, int(off[-1])), 1, 5
    idx = torch.full((int(off[-1]),), -7, device=DEV, dtype=torch.int32)
    got = A.bootstrap_means(torch.tensor(values, device=DEV), off, B, seed, inject=(None, off), idx_out=idx).cpu().numpy()
    idx = idx.cpu().numpy()
    want_idx = {(j, 0): AR.philox_indices(seed, j, 0, int(lens[j])) for j in range(3)}
    for j in range(3):
        assert np.array_equal(idx[off[j]:off[j + 1]], want_idx[(j, 0)]), j
    check_means(got, AR.bootstrap_means_host(values, off, lambda j, b, n: want_idx[(j, b)], B), seg_bound(values, off))
    assert np.isfinite(got).all()


def test_bootstrap_more_segments_than_one_launch_carries():
    """130 short segments (the offsets travel as kernel arguments, 64 segments per launch: three launches): indices
    and means of every segment against the host restatement, so the segment index of the Philox counter and of the
    output row is the call's, not the launch's."""
    from omniisaacgymenvs_loop_amd.scenario import analysis as A
    rng = np.random.default_rng(21)
    lens = np.asarray([(7 * j) % 41 for j in range(130)], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    values, B, seed = rng.normal(-2.0, 9.0, int(off[-1])), 5, 77
    inj_off = np.concatenate([[0], np.cumsum(B * lens)]).astype(np.int64)
    idx = torch.full((int(inj_off[-1]),), -7, device=DEV, dtype=torch.int32)
    got = A.bootstrap_means(torch.tensor(values, device=DEV), off, B, seed, inject=(None, inj_off),
                            idx_out=idx).cpu().numpy()
    idx = idx.cpu().numpy()
    want_idx = {(j, b): AR.philox_indices(seed, j, b, int(lens[j])) for j in range(len(lens)) for b in range(B)}
    for (j, b), w in want_idx.items():
        assert np.array_equal(idx[inj_off[j] + b * lens[j]:inj_off[j] + (b + 1) * lens[j]], w), (j, b)
    check_means(got, AR.bootstrap_means_host(values, off, lambda j, b, n: want_idx[(j, b)], B), seg_bound(values, off))
    assert np.isnan(got[lens == 0]).all() and np.isfinite(got[lens > 0]).all()


# ------------------------------------------------------------------------------------------ usv_ana_quantiles
@pytest.mark.parametrize("B", [1, 2, 31, 2000])
def test_quantiles_equal_numpy(B):
    from omniisaacgymenvs_loop_amd.scenario import analysis as A
    rng = np.random.default_rng(B)
    x = rng.normal(0.0, 5.0, (6, B))
    x[1] = np.round(x[1]) + 0.0                 # ties (no -0.0: its place among the zeros is not defined)
    x[2] = 1.25                                 # one value
    x[3, ::2] = np.nan                          # NaNs (every value when B = 1)
    x[4, -1] = np.nan
    x[5] = np.nan                               # all NaN
    q = (0.025, 0.975, 0.5, 0.0, 1.0, 1.0 / 3.0)
    xd = torch.tensor(x, device=DEV)
    for mode, fn in ((A.NAN_PROPAGATE, np.quantile), (A.NAN_IGNORE, np.nanquantile)):
        got = A.quantiles(xd, q, mode).cpu().numpy()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            want = np.stack([fn(row, q) for row in x])
        same_nan(got, want, mode)
        ok = ~np.isnan(want)
        assert np.array_equal(bits(got[ok]), bits(want[ok])), (mode, got, want)
        assert ok[:3].all() and not ok[5].any()
    assert np.isnan(A.quantiles(xd, q, A.NAN_PROPAGATE).cpu().numpy()[4]).all()
    if B > 1:
        assert np.isfinite(A.quantiles(xd, q, A.NAN_IGNORE).cpu().numpy()[4]).all()


# ------------------------------------------------------------------------------------------ the fixture, end to end
def ci_bound(*segs):
    """3 x sum over the segments a replicate's value is formed from of len x 2^-52 x max|v|: order statistics are
    1-Lipschitz in the replicate values, a replicate's mean is within len x 2^-52 x max|v| of the restatement's (a
    difference of two means within the sum of the two), and the lerp adds two roundings."""
    return 3.0 * sum(len(v) * EPS * (np.abs(v[np.isfinite(v)]).max() if np.isfinite(v).any() else 0.0) for v in segs)


def close(got, want, bound, msg):
    if np.isnan(want):
        assert np.isnan(got), msg
    else:
        assert abs(got - want) <= bound, (msg, got, want, bound)


def inject_of(chunks):
    """(inj_idx on the device, inj_off) from one [B][len] index array per segment."""
    off = np.concatenate([[0], np.cumsum([c.size for c in chunks])]).astype(np.int64)
    flat = np.concatenate([c.reshape(-1) for c in chunks]) if chunks else np.zeros(0)
    return torch.tensor(flat.astype(np.int32), device=DEV), off


@pytest.mark.parametrize("tag", ["a", "b"])
def test_paired_bootstrap_reproduces_the_reference(fx, tag):
    from omniisaacgymenvs_loop_amd.scenario import analysis as A
    frame, S, R, n, tabs, control, treat = frame_arms(tag)
    B = int(fx["settings"][0])
    flat, off, ns = fx[f"{tag}_pair_draws"], fx[f"{tag}_pair_draws_off"], fx[f"{tag}_pair_n"]
    chunks = [flat[off[m]:off[m + 1]].astype(np.int64).reshape(B, ns[m]) if ns[m] >= 2
              else np.zeros((B, ns[m]), np.int64) for m in range(len(ns))]       # n < 2: the reference draws nothing
    rows = A.paired_bootstrap(control, treat, n, S, R, 1, AR.REWARD_SCALE, n_boot=B, inject=inject_of(chunks))
    assert [r["metric"] for r in rows] == list(AR.METRIC_NAMES)
    assert [r["n_pairs"] for r in rows] == ns.tolist()
    deltas = AR.pair_delta_rows(frame, S)
    for m, r in enumerate(rows):
        want = fx[f"{tag}_pair_diff"][m]
        assert (np.isnan(want) and np.isnan(r["diff_treat_minus_control"])) or \
            bits([r["diff_treat_minus_control"]])[0] == bits([want])[0], r
        v = deltas[m][np.isfinite(deltas[m])]
        for k in ("lo", "hi"):
            close(r[f"ci95_{k}"], fx[f"{tag}_pair_{k}"][m], ci_bound(v), (r["metric"], k))
    if tag == "b":
        one = rows[D["USV_ANA_PD_TIME_SUCC"]]
        assert one["n_pairs"] == 1 and one["ci95_lo"] == one["ci95_hi"] == one["diff_treat_minus_control"]
        assert all(np.isnan(rows[-1][k]) for k in ("diff_treat_minus_control", "ci95_lo", "ci95_hi"))


def test_unpaired_bootstrap_reproduces_the_reference(fx):
    from omniisaacgymenvs_loop_amd.scenario import analysis as A
    frame, S, R, n, tabs, control, treat = frame_arms("a")
    B = int(fx["settings"][1])
    flat, off, nt, nc = fx["a_unp_draws"], fx["a_unp_draws_off"], fx["a_unp_nt"], fx["a_unp_nc"]
    chunks = []
    for m in range(len(nt)):
        d = flat[off[m]:off[m + 1]].astype(np.int64).reshape(B, nt[m] + nc[m])   # per replicate: treat, then control
        chunks += [d[:, :nt[m]], d[:, nt[m]:]]
    rows = A.unpaired_bootstrap(control, treat, n, S, R, 1, AR.REWARD_SCALE, n_boot=B, inject=inject_of(chunks))
    assert [r["n_treat"] for r in rows] == nt.tolist() and [r["n_control"] for r in rows] == nc.tolist()
    for m, (r, (_, col, so)) in enumerate(zip(rows, AR.METRICS)):
        assert bits([r["diff_treat_minus_control"]])[0] == bits([fx["a_unp_diff"][m]])[0], r
        bound = ci_bound(AR.group_values(frame, col, so, AR.TREAT), AR.group_values(frame, col, so, AR.CONTROL))
        for k in ("lo", "hi"):
            close(r[f"ci95_{k}"], fx[f"a_unp_{k}"][m], bound, (r["metric"], k))


def test_stratified_effects_reproduce_the_reference(fx):
    from omniisaacgymenvs_loop_amd.scenario import analysis as A
    frame, S, R, n, tabs, control, treat = frame_arms("a")
    _, _, B, n_bins, min_per_bin, _ = (int(v) for v in fx["settings"])
    nt, nc = fx["a_strat_n_treat"], fx["a_strat_n_control"]
    flat, pos, chunks = fx["a_strat_draws"].astype(np.int64), 0, []
    for q in range(len(nt)):                     # per kept bin and replicate: success t, c, return_scaled t, c
        w = 2 * (nt[q] + nc[q])
        d = flat[pos:pos + B * w].reshape(B, w)
        pos += B * w
        chunks += [d[:, :nt[q]], d[:, nt[q]:nt[q] + nc[q]], d[:, nt[q] + nc[q]:2 * nt[q] + nc[q]],
                   d[:, 2 * nt[q] + nc[q]:]]
    assert pos == flat.size
    rows, bins = A.stratified_effects(control, treat, n, S, R, 1, AR.REWARD_SCALE, strata=AR.strata_a(frame, S, R),
                                      n_bins=n_bins, min_per_bin=min_per_bin, n_boot=B, inject=inject_of(chunks),
                                      labels=("group", "treat", "control"), return_bins=True)
    assert list(rows[0]) == A.STRAT_COLUMNS == list(AR.STRAT_COLUMNS)
    assert [AR.STRATA_A.index(r["strat_col"]) for r in rows] == fx["a_strat_col"].tolist()
    for c in ("bin", "n", "n_treat", "n_control"):
        assert [r[c] for r in rows] == fx[f"a_strat_{c}"].tolist(), c
    for c in ("bin_lo", "bin_hi", "delta_success", "delta_return_scaled"):      # edges and point estimates: exact
        assert np.array_equal(bits([r[c] for r in rows]), bits(fx[f"a_strat_{c}"])), c
    p = (frame["scene_idx"] * R + frame["rollout"]).astype(int)
    assert "d_const" not in bins
    for name in ("d_row", "d_goal", "d_tied"):                                   # bin membership: exact
        edges, want = AR.strat_bins(frame[name], n_bins)
        assert np.array_equal(bins[name][0], edges) and np.array_equal(bins[name][1][p], want), name
    g = frame["group"]
    for q, r in enumerate(rows):
        _, member = AR.strat_bins(frame[r["strat_col"]], n_bins)
        mt, mc = (member == r["bin"]) & (g == AR.TREAT), (member == r["bin"]) & (g == AR.CONTROL)
        for col, key in (("success", "delta_success"), ("return_scaled", "delta_return_scaled")):
            bound = ci_bound(frame[col][mt], frame[col][mc])
            for k in ("lo", "hi"):
                close(r[f"{key}_ci95_{k}"], fx[f"a_strat_{key}_ci95_{k}"][q], bound, (q, key, k))


# ------------------------------------------------------------------------------------------ what is resampled
def test_resampling_is_over_scenarios_not_pairs():
    """S = 64 scenarios whose R = 3 rollouts are identical: the pairs of a scenario carry one observation, so the
    interval of a bootstrap over scenarios is about sqrt(3) wider than cmp_totals' normal interval over the 192
    pairs."""
    from omniisaacgymenvs_loop_amd.scenario import analysis as A
    from omniisaacgymenvs_loop_amd.scenario import compare as C
    S, R, n = 64, 3, 192
    ra, rb = {}, {}
    for s in range(S):
        a_ok, b_ok = s % 2 == 0, s % 3 != 0
        for r in range(R):
            ra[s * R + r] = (CR.GOAL if a_ok else CR.OTHER, 50.0, 1.0, 0.5, 1.5)
            rb[s * R + r] = (CR.GOAL if b_ok else CR.COLL, 60.0, 2.0, 0.25, 1.0)
    (ta, ca), (tb, cb) = CR.make_table(n, 1, ra), CR.make_table(n, 1, rb)
    control, treat = Arm(ta, ca, 1), Arm(tb, cb, 1)
    tot = C.cmp_totals(C.cmp_to_dict(C.cmp_fold_device(control.ev, treat.ev, n, S, R, 1, 1.2, DEV)))
    sd = tot["success_diff"]
    normal_half = (sd["ci95_hi"] - sd["ci95_lo"]) / 2
    row = A.paired_bootstrap(control, treat, n, S, R, 1, n_boot=2000, seed=3)[0]
    assert row["metric"] == "success_rate" and row["n_pairs"] == S
    assert row["diff_treat_minus_control"] == pytest.approx(sd["mean"], abs=1e-12)
    half = (row["ci95_hi"] - row["ci95_lo"]) / 2
    print(f"paired half-width {half:.4f}, normal half-width over pairs {normal_half:.4f}")
    assert half > normal_half
    assert half == pytest.approx(normal_half * np.sqrt(R), rel=0.15)   # 2000 replicates: the quantiles' own noise


# ------------------------------------------------------------------------------------------ a real comparison
def test_analyse_on_a_compare_result():
    """scenario_pre20, 64 envs, 12-step episodes, R = 3, the same policy in two arms: every paired delta is exactly
    0, every interval [0, 0], n_pairs the scenarios present (the success-only metrics: those with a success)."""
    from omniisaacgymenvs_loop_amd.loopz import LoopzTeacher
    from omniisaacgymenvs_loop_amd.scenario import ScenarioRunner, load_table
    from omniisaacgymenvs_loop_amd.scenario import analysis as A
    from omniisaacgymenvs_loop_amd.scenario import compare as C
    from tests.test_compare_gpu import _actor, _task
    table, n, R_ = load_table(PRE20), 64, 3
    actor = _actor(33)
    res = C.compare(lambda: ScenarioRunner(_task(n), table, rollouts=R_),
                    {"teacher": lambda r: LoopzTeacher(actor, DEV), "teacher_again": lambda r: LoopzTeacher(actor, DEV)})
    S = res["S"]
    strata = {"d_goal": np.linspace(0.0, 1.0, S), "row": np.arange(S * R_, dtype=np.float64)}
    out = A.analyse(res, reward_scale=0.5, n_boot=64, seed=1, strata=strata, n_bins=3, min_per_bin=2)
    assert list(out) == ["teacher_again"]
    with_success = int((res["arms"]["teacher"]["fold"]["success_rate"] > 0).sum())
    for r, (_, _, succ_only) in zip(out["teacher_again"]["paired"], A.METRICS):
        assert r["n_pairs"] == (with_success if succ_only else S), r
        for k in ("diff_treat_minus_control", "ci95_lo", "ci95_hi"):
            assert (r[k] == 0.0) if r["n_pairs"] else np.isnan(r[k]), r
    for r in out["teacher_again"]["unpaired"]:
        assert r["n_treat"] == r["n_control"] and (r["diff_treat_minus_control"] == 0.0 or r["n_treat"] == 0), r
    strat = out["teacher_again"]["stratified"]
    assert {r["strat_col"] for r in strat} == {"d_goal", "row"} and len(strat) == 6
    assert all(r["delta_success"] == 0.0 and r["delta_return_scaled"] == 0.0 and r["n_treat"] == r["n_control"]
               for r in strat)
    assert sum(r["n"] for r in strat if r["strat_col"] == "row") == 2 * S * R_


def test_compare_policies_writes_the_analysis_only_when_asked(tmp_path, monkeypatch):
    """loopz_train for one update at 64 envs, then the command line on scenario_pre20 with two teacher arms: with
    compare.bootstrap=16 the three CSVs with the reference's headers, without it none of them."""
    from omniisaacgymenvs_loop_amd.scenario import analysis as A
    from omniisaacgymenvs_loop_amd.scripts import compare_policies as CP
    from omniisaacgymenvs_loop_amd.scripts import loopz_train as LT
    from tests.test_compare_gpu import _cfg
    monkeypatch.chdir(tmp_path)
    cfg = _cfg(64, 3)
    cfg["environment"]["max_time"] = 0.16
    cfg["environment"]["eval_every_n"] = 1
    LT.train(cfg, max_updates=1, log=lambda *a: None)
    ckpt = str(tmp_path / "runs" / "USV" / "nn" / "full_1.pt")
    common = ["num_envs=64", "task.env.maxEpisodeLength=12", f"scenario_npz={PRE20}", f"checkpoint={ckpt}",
              "compare.arms=teacher,teacher_wrong_tail", "compare.n_rollouts=3"]
    off_dir, on_dir = str(tmp_path / "off"), str(tmp_path / "on")
    CP.main(common + [f"out_dir={off_dir}"])
    assert sorted(os.listdir(off_dir)) == ["compare.meta.json", "compare_pairs.csv", "compare_scenarios.csv"]
    assert "analysis" not in json.load(open(os.path.join(off_dir, "compare.meta.json")))
    CP.main(common + [f"out_dir={on_dir}", "compare.bootstrap=16", "compare.n_bins=2", "compare.min_per_bin=2",
                      "compare.strata=straight_line_dist,d_spawn,d_goal,d_corr,d_oo,density,start_speed"])
    assert sorted(os.listdir(on_dir)) == ["compare.meta.json", "compare_pairs.csv", "compare_scenarios.csv",
                                          "teacher_wrong_tail_vs_teacher"]
    for name in ("compare_pairs.csv", "compare_scenarios.csv"):     # what was written before is written as before
        assert open(os.path.join(on_dir, name)).read() == open(os.path.join(off_dir, name)).read(), name
    arm_dir = os.path.join(on_dir, "teacher_wrong_tail_vs_teacher")
    assert sorted(os.listdir(arm_dir)) == sorted(CP.ANALYSIS_FILES.values())
    heads = {"layer0_summary.csv": ["metric", "n_treat", "n_control", "diff_treat_minus_control", "ci95_lo", "ci95_hi"],
             "layer0_paired_summary.csv": ["metric", "n_pairs", "diff_treat_minus_control", "ci95_lo", "ci95_hi"],
             "stratified_effects.csv": list(AR.STRAT_COLUMNS)}
    for name, head in heads.items():
        rows = list(csv.reader(open(os.path.join(arm_dir, name))))
        assert rows[0] == head, name
        if name != "stratified_effects.csv":
            assert [r[0] for r in rows[1:]] == list(A.METRIC_NAMES)
    paired = list(csv.DictReader(open(os.path.join(arm_dir, "layer0_paired_summary.csv"))))
    assert int(paired[0]["n_pairs"]) == 20
    strat = list(csv.DictReader(open(os.path.join(arm_dir, "stratified_effects.csv"))))
    assert {r["strat_col"] for r in strat} <= set(CP.STRATA) and len(strat) >= 2
    meta = json.load(open(os.path.join(on_dir, "compare.meta.json")))
    assert meta["analysis"]["n_boot"] == 16 and meta["analysis"]["n_bins"] == 2 and len(meta["analysis"]["strata"]) == 7
