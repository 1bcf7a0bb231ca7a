"""Fixed-horizon success-rate evaluation without a GPU: the numpy restatement of the streaming rules
(tests/task_eval_restate.py) against the reference-derived fixture (tests/golden/task_eval_golden.npz, written by
tests/golden/make_task_eval_golden.py), the entry points' argument checks, usv_teval_channels per kind, and the
report's column names and group keys."""
import csv
import ctypes
import json
import os

import numpy as np
import pytest

from tests import task_eval_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "omniisaacgymenvs_loop_amd", "cfg", "task", "USV")
KIND_YAML = {"GoToXY": R.GO_TO_XY, "KeepXY": R.KEEP_XY, "GoToPose": R.GO_TO_POSE, "TrackXYVelocity": R.TRACK_XY,
             "TrackXYOVelocity": R.TRACK_XYO}


@pytest.fixture(scope="module")
def tg():
    return R.load_golden()


def _check_against_fixture(g, prefix, kind, obs, rew, reset, msg):
    thr, levels = g[f"{prefix}_thr"], g[f"{prefix}_levels"]
    T = obs.shape[0]
    tab = R.restate(kind, obs, rew, reset, thr, levels, horizon=T)
    assert (tab[R.STEPS] == T).all()
    for c in range(len(R.CHANNELS[kind])):
        rec = R.channel_records(tab, c)
        R.assert_channel(rec, R.golden_channel(g, prefix, c), msg=f"{msg} channel {c}")
        # the rates have pandas' bits (mean() * 100, and the share of stayed envs); the time-under shares np.mean's
        np.testing.assert_array_equal(np.array(R.rates(rec)), g[f"{prefix}_rates"][c], err_msg=f"{msg} rates {c}")
        np.testing.assert_array_equal(R.time_under(rec, T), g[f"{prefix}_time_under"][c], err_msg=f"{msg} time {c}")
    return tab


@pytest.mark.parametrize("name", ["pose", "track"])
def test_restatement_reproduces_reference_on_synthetic_set(tg, name):
    """T = 24, n = 70: every branch of the rule in every channel, the float32 neighbours of thr, thr / 2 and
    thr * 7.5 in the scalar and norm channels; integers and flags exactly."""
    kind, obs, rew, reset, thr, levels = R.synthetic(tg, name)
    assert obs.shape == (24, 70, 33)
    tab = _check_against_fixture(tg, f"A_{name}", kind, obs, rew, reset, f"synthetic {name}")
    names = [str(s) for s in tg[f"A_{name}_case_names"]]
    for c in range(2):
        rec = R.channel_records(tab, c)
        i = names.index
        assert rec["first_thr"][i("never_reached_in_margin")] == -1 and rec["stay"][i("never_reached_in_margin")]
        assert rec["first_thr"][i("never_reached_out_of_margin")] == -1
        assert not rec["stay"][i("never_reached_out_of_margin")]
        assert rec["first_thr"][i("reached_at_0")] == 0 and rec["first_thr"][i("reached_at_last")] == 23
        assert rec["first_thr"][i("reached_then_out")] == 5 and not rec["stay"][i("reached_then_out")]
        assert rec["stay"][i("out_then_reached_and_stayed")] and rec["first_thr2"][i("reached_thr_never_thr2")] == -1
        assert rec["stay"][i("nan_before_reach")] and not rec["stay"][i("nan_after_reach")]
        assert not rec["stay"][i("nan_never_reached")] and np.isnan(rec["err_sum"][i("nan_never_reached")])
        if (name, c) != ("pose", 1):   # the heading channel keeps a gap from every level (its atan2 is the device's)
            assert rec["first_thr"][i("exact_thr_below")] == 7 and rec["first_thr"][i("exact_thr_at")] == -1
            assert rec["first_thr2"][i("exact_thr2_below")] == 7 and rec["first_thr2"][i("exact_thr2_at")] == -1
            assert rec["stay"][i("exact_margin_below")] and not rec["stay"][i("exact_margin_at")]
    assert (tab[R.RESETS] == reset.sum(0)).all() and tab[R.RESETS].sum() > 0
    np.testing.assert_allclose(tab[R.RETURN], rew.astype(np.float64).sum(0), rtol=1e-12)


@pytest.mark.parametrize("variant", sorted(R.FIXTURE_KIND))
def test_restatement_reproduces_reference_on_recorded_observations(tg, golden, variant):
    d = golden(f"episode_{variant}.npz")
    kind = R.FIXTURE_KIND[variant]
    _check_against_fixture(tg, f"B_{variant}", kind, d["obs"], d["rew"], d["reset"], f"episode_{variant}")
    # the gap the generator asserted: ten times the device's observation tolerance
    x = R.errors(kind, d["obs"]).astype(np.float64)
    for c in range(x.shape[0]):
        lv = [float(v) for v in R.derived_levels(tg[f"B_{variant}_thr"][c])] + [float(v) for v in
                                                                               tg[f"B_{variant}_levels"][c]]
        assert all(np.abs(x[c] - q).min() >= 1e-4 * (1 + q) for q in lv)


def test_a_step_past_the_horizon_changes_nothing_but_steps(tg):
    kind, obs, rew, reset, thr, levels = R.synthetic(tg, "pose")
    a = R.restate(kind, obs, rew, reset, thr, levels, horizon=10, steps=10)
    b = R.restate(kind, obs, rew, reset, thr, levels, horizon=10)
    assert (b[R.STEPS] == 24).all() and (a[R.STEPS] == 10).all()
    b[R.STEPS] = a[R.STEPS]
    np.testing.assert_array_equal(a, b)


def test_summary_restatement():
    tab = R.begin_table(3)
    tab[R.STEPS] = [5, 5, 6]
    tab[R.RESETS] = [0, 2, 1]
    tab[R.RETURN] = [1.0, 2.0, 6.0]
    tab[R.FIRST_THR] = [-1, 0, 3]
    tab[R.STAY] = [1, 0, 1]
    tab[R.UNDER0] = [0, 5, 2]
    out = R.summarize(tab, 1)
    assert list(out[:6]) == [3, 1, 5, 6, 3, 2]
    assert list(out[R.S_CH:R.S_CH + 6]) == [2, 0, 2, 7, 0, 0]
    assert out[R.S_RETURN] == 3 and out[R.S_RETURN + 1] == 3.0
    assert out[R.S_RETURN + 2] == pytest.approx(np.std([1.0, 2.0, 6.0]))


def _yaml_of(name):
    from omniisaacgymenvs_loop_amd.tasks.usv_config import load_yaml
    return load_yaml(os.path.join(CFG, f"USV_Virtual_{name}.yaml"))


def _cfg_of(name):
    from omniisaacgymenvs_loop_amd.tasks.usv_config import build_usv_cfg
    return build_usv_cfg(_yaml_of(name))


def test_argument_checks_precede_device_work():
    """NULL table / env buffers / output -> 1; horizon < 1 or a bad threshold or level of a used channel -> 2;
    CaptureXY -> 3; before any launch (there is no device here; the pointers are never dereferenced)."""
    from omniisaacgymenvs_loop_amd import _capi
    from omniisaacgymenvs_loop_amd._abi import DEFINES, UsvBufs, UsvTEval
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libusv_hip.so not built (run __graft_entry__.build())")
    lib = _capi.lib()
    cfg = _cfg_of("GoToPose")
    assert cfg.task_kind == DEFINES["USV_TASK_GO_TO_POSE"]
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)
    b = UsvBufs()
    b.n = 64
    b.obs = b.rew = b.reset_buf = p

    def tv_of(table=p, horizon=10, thr=(0.1, 0.1), levels=((0.3, 0.2, 0.1), (0.3, 0.2, 0.1))):
        tv = UsvTEval()
        tv.table, tv.horizon = table, horizon
        for c in range(2):
            tv.thr[c] = thr[c]
            for l in range(3):
                tv.level[c][l] = levels[c][l]
        return tv

    def calls(cfg_, b_, tv_, out=p):
        c, bb, t = _capi.byref(cfg_), _capi.byref(b_), _capi.byref(tv_)
        return [lib.usv_teval_begin(c, bb, t, None), lib.usv_teval_step(c, bb, t, None),
                lib.usv_teval_summary(c, bb, t, out, None)]

    assert calls(cfg, b, tv_of(table=None)) == [1, 1, 1]
    c, bb, ok = _capi.byref(cfg), _capi.byref(b), tv_of()
    assert lib.usv_teval_summary(c, bb, _capi.byref(ok), None, None) == 1   # no output
    assert lib.usv_teval_begin(None, bb, _capi.byref(ok), None) == 1
    assert lib.usv_teval_begin(c, None, _capi.byref(ok), None) == 1
    assert lib.usv_teval_begin(c, bb, None, None) == 1
    for missing in ("obs", "rew", "reset_buf"):   # env buffers missing: the kernel that reads them refuses
        b1 = UsvBufs()
        ctypes.memmove(ctypes.byref(b1), ctypes.byref(b), ctypes.sizeof(b))
        setattr(b1, missing, None)
        assert lib.usv_teval_step(c, _capi.byref(b1), _capi.byref(ok), None) == 1
    b0 = UsvBufs()
    assert calls(cfg, b0, ok) == [1, 1, 1]   # n = 0
    for h in (0, -3):
        assert calls(cfg, b, tv_of(horizon=h)) == [2, 2, 2]
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        assert calls(cfg, b, tv_of(thr=(bad, 0.1))) == [2, 2, 2]
        assert calls(cfg, b, tv_of(thr=(0.1, bad))) == [2, 2, 2]
        assert calls(cfg, b, tv_of(levels=((0.3, 0.2, 0.1), (0.3, bad, 0.1)))) == [2, 2, 2]
    cap =_cfg_of("GoToPose")
    cap.task_kind = DEFINES["USV_TASK_CAPTURE_XY"]
    assert calls(cap, b, ok) == [3, 3, 3]


def test_one_channel_kind_ignores_the_unused_channel():
    """Status 2 is about the channels a kind uses: with horizon < 1 ruled out first, GoToXY with junk in channel 1
    fails only on a NULL output (status 1), i.e. it passed the value checks."""
    from omniisaacgymenvs_loop_amd import _capi
    from omniisaacgymenvs_loop_amd._abi import UsvBufs, UsvTEval
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libusv_hip.so not built (run __graft_entry__.build())")
    lib = _capi.lib()
    dummy = ctypes.create_string_buffer(64)
    b = UsvBufs()
    b.n = 64
    tv = UsvTEval()
    tv.table, tv.horizon = ctypes.addressof(dummy), 5
    tv.thr[0], tv.thr[1] = 0.1, float("nan")
    for l in range(3):
        tv.level[0][l] = 0.1
    for name in ("GoToXY", "KeepXY", "TrackXYVelocity"):
        cfg = _cfg_of(name)
        assert lib.usv_teval_summary(_capi.byref(cfg), _capi.byref(b), _capi.byref(tv), None, None) == 1
    for name in ("GoToPose", "TrackXYOVelocity"):
        cfg = _cfg_of(name)
        assert lib.usv_teval_summary(_capi.byref(cfg), _capi.byref(b), _capi.byref(tv), None, None) == 2


def test_channels_per_kind():
    from omniisaacgymenvs_loop_amd import _capi
    from omniisaacgymenvs_loop_amd._abi import DEFINES
    from omniisaacgymenvs_loop_amd.eval import CHANNELS, default_thresholds
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libusv_hip.so not built (run __graft_entry__.build())")
    lib = _capi.lib()
    for name, kind in KIND_YAML.items():
        cfg = _cfg_of(name)
        assert cfg.task_kind == kind
        assert lib.usv_teval_channels(_capi.byref(cfg)) == len(R.CHANNELS[kind]) == len(CHANNELS[kind])
        assert CHANNELS[kind] == R.CHANNELS[kind]
        assert len(default_thresholds(cfg)) == len(CHANNELS[kind])
    cfg.task_kind = DEFINES["USV_TASK_CAPTURE_XY"]
    assert lib.usv_teval_channels(_capi.byref(cfg)) == 0 and lib.usv_teval_channels(None) == 0
    # the defaults: the task's own tolerance, the reference function's where the kind has none
    pose, xyo = _cfg_of("GoToPose"), _cfg_of("TrackXYOVelocity")
    tp = _yaml_of("GoToPose")["env"]["task_parameters"], _yaml_of("TrackXYOVelocity")["env"]["task_parameters"]
    assert default_thresholds(pose) == (float(tp[0]["position_tolerance"]), 0.087)   # the yaml's decimals
    assert default_thresholds(xyo) == (float(tp[1]["lin_vel_tolerance"]), float(tp[1]["ang_vel_tolerance"]))
    assert np.float32(default_thresholds(pose)[0]) == np.float32(pose.position_tolerance)
    pose.position_tolerance = 0.0
    assert default_thresholds(pose) == (0.02, 0.087)


def test_report_column_names_group_keys_and_csv(tmp_path):
    from omniisaacgymenvs_loop_amd._abi import DEFINES
    from omniisaacgymenvs_loop_amd.eval import (format_task_summary, task_column_names, task_csv_columns,
                                                write_summary_json, write_task_csv)
    from omniisaacgymenvs_loop_amd.eval.report import task_records_from_table, task_summary_from_device
    # the reference's names, formatted as its f-strings format them
    assert task_column_names("position", 0.02) == ("success_rate_0.02_m", "success_rate_0.01_m",
                                                   "success_and_stay_within_0.15_m")
    assert task_column_names("heading", 0.087) == (f"success_rate_0.087_rad", f"success_rate_{0.087 / 2}_rad",
                                                   f"success_and_stay_within_{0.087 * 7.5}_rad")
    assert task_column_names("xy_velocity", 0.15)[0] == "success_rate_0.15_m/s"
    assert task_column_names("omega_velocity", 0.3)[2] == f"success_and_stay_within_{0.3 * 7.5}_rad/s"
    n, T = 4, 6
    tab = R.begin_table(n)
    tab[R.STEPS] = T
    tab[R.RETURN] = [1.0, 2.0, 3.0, 6.0]
    tab[R.FIRST_THR] = [-1, 0, 3, 2]
    tab[R.FIRST_THR2] = [-1, -1, 4, 2]
    tab[R.STAY] = [1, 0, 1, 1]
    tab[R.UNDER0], tab[R.UNDER0 + 1], tab[R.UNDER0 + 2] = [0, 6, 3, 4], [0, 5, 3, 4], [0, 0, 2, 4]
    tab[R.ERR_SUM], tab[R.ERR_LAST] = [6.0, 0.6, 1.2, 0.3], [1.0, 0.1, 0.2, 0.05]
    tab[R.CH_STRIDE + R.FIRST_THR] = [1, 1, 1, -1]
    ch = ("position", "heading")
    s = task_summary_from_device(R.summarize(tab, 2), ch, (0.02, 0.087), (np.float32(0.02), np.float32(0.087)),
                                 ((0.05, 0.02, 0.01), (0.2175, 0.087, 0.0435)), T)
    assert s["envs"] == n and s["channels"] == ["position", "heading"] and s["resets"] == 0
    assert list(s["position"]["table"]) == list(task_column_names("position", 0.02))
    assert list(s["heading"]["table"]) == list(task_column_names("heading", 0.087))
    assert list(s["position"]["table"].values()) == [75.0, 50.0, 75.0]
    assert s["heading"]["table"]["success_rate_0.087_rad"] == 75.0
    assert list(s["position"]["time_under"]) == ["PT_0.05", "PT_0.02", "PT_0.01"]
    assert list(s["heading"]["time_under"]) == ["OT_0.2175", "OT_0.087", "OT_0.0435"]
    assert list(s["position"]["time_under"].values()) == [13 / 24 * 100, 12 / 24 * 100, 6 / 24 * 100]
    assert s["return_raw"]["mean"] == 3.0 and s["return_raw"]["count"] == 4
    txt = format_task_summary(s)
    assert "success_and_stay_within_0.15_m: 75.0000" in txt and "WARNING" not in txt
    tab[R.RESETS] = [0, 1, 0, 2]
    s2 = task_summary_from_device(R.summarize(tab, 2), ch, (0.02, 0.087), (0.02, 0.087),
                                  ((0.05, 0.02, 0.01), (0.2175, 0.087, 0.0435)), T)
    assert s2["resets"] == 3 and s2["envs_reset"] == 2
    assert "WARNING: 2 env(s) were reset inside the horizon" in format_task_summary(s2)
    write_summary_json(str(tmp_path / "s.json"), s2)
    assert json.load(open(tmp_path / "s.json"))["position"]["table"]["success_rate_0.02_m"] == 75.0
    rec = task_records_from_table(tab, ch, T)
    path = str(tmp_path / "t.csv")
    assert write_task_csv(path, rec, ch) == n
    rows = list(csv.reader(open(path)))
    assert tuple(rows[0]) == task_csv_columns(ch) and len(rows) == n + 1
    assert rows[0][:6] == ["env", "steps", "return_raw", "resets", "position_first_thr", "position_first_thr2"]
    assert rows[1][4] == "-1" and rows[3][4] == "3" and float(rows[1][10]) == 1.0 and rows[0][10] == "position_err_mean"
    assert DEFINES["USV_TEV_ROWS"] == R.ROWS and DEFINES["USV_TEVS_N"] == R.S_N
    for k, v in (("FIRST_THR", R.FIRST_THR), ("FIRST_THR2", R.FIRST_THR2), ("STAY", R.STAY), ("UNDER0", R.UNDER0),
                 ("ERR_SUM", R.ERR_SUM), ("ERR_LAST", R.ERR_LAST), ("CH_STRIDE", R.CH_STRIDE), ("STEPS", R.STEPS),
                 ("RETURN", R.RETURN), ("RESETS", R.RESETS)):
        assert DEFINES[f"USV_TEV_{k}"] == v
    for k, v in (("CH", R.S_CH), ("CH_STRIDE", R.S_CH_STRIDE), ("RETURN", R.S_RETURN), ("RESET_ENVS", R.S_RESET_ENVS)):
        assert DEFINES[f"USV_TEVS_{k}"] == v
