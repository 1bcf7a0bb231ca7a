"""Batched policy evaluation without a GPU: the entry points' argument checks, the numpy restatement of the
per-episode records against the reference-derived fixture (tests/golden/eval_golden.npz, written by
tests/golden/make_eval_golden.py), and the CSV / summary host code."""
import csv
import ctypes
import json
import math
import os

import numpy as np
import pytest

from tests import eval_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_YAML = os.path.join(ROOT, "omniisaacgymenvs_loop_amd", "cfg", "task", "USV", "IROS2024",
                         "USV_Virtual_CaptureXY_SysID-TEST.yaml")


@pytest.fixture(scope="module")
def eg():
    return dict(np.load(os.path.join(R.GOLDEN, "eval_golden.npz"), allow_pickle=False))


def test_argument_checks_precede_device_work():
    """NULL buffers -> 1, max_episodes < 1 -> 2, a task kind other than CaptureXY -> 3, for each of the four
    entry points, before any launch (there is no device here; the pointers are never dereferenced)."""
    from omniisaacgymenvs_loop_amd import _capi
    from omniisaacgymenvs_loop_amd._abi import DEFINES, UsvBufs, UsvEval
    from omniisaacgymenvs_loop_amd.tasks.usv_config import build_usv_cfg, load_yaml
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libusv_hip.so not built (run __graft_entry__.build())")
    lib = _capi.lib()
    cfg = build_usv_cfg(load_yaml(TEST_YAML))
    assert cfg.task_kind == DEFINES["USV_TASK_CAPTURE_XY"]
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)
    b = UsvBufs()
    b.n = 64
    for k in ("px", "py", "yaw", "tgt_x", "tgt_y", "obst", "rew", "reset_buf", "just_reset", "done_succ", "done_coll"):
        setattr(b, k, p)

    def ev_of(acc=p, episodes=p, ep_count=p, k=1):
        ev = UsvEval()
        ev.acc, ev.episodes, ev.ep_count, ev.max_episodes, ev.action_scale, ev.control_dt = (acc, episodes, ep_count,
                                                                                            k, 1.0, 0.2)
        return ev

    def calls(cfg_, b_, ev_, actions=p, out=p):
        c, bb, e = _capi.byref(cfg_), _capi.byref(b_), _capi.byref(ev_)
        return [lib.usv_eval_begin(c, bb, e, None), lib.usv_eval_mark(c, bb, e, None),
                lib.usv_eval_step(c, bb, e, actions, None), lib.usv_eval_summary(c, bb, e, out, None)]

    for ev in (ev_of(acc=None), ev_of(episodes=None), ev_of(ep_count=None)):
        assert calls(cfg, b, ev) == [1, 1, 1, 1]
    c, bb, ok = _capi.byref(cfg), _capi.byref(b), ev_of()
    assert lib.usv_eval_step(c, bb, _capi.byref(ok), None, None) == 1      # no actions
    assert lib.usv_eval_summary(c, bb, _capi.byref(ok), None, None) == 1   # no output
    assert lib.usv_eval_begin(None, bb, _capi.byref(ok), None) == 1
    b_null = UsvBufs()
    b_null.n = 64   # env buffers missing: the kernels that read them refuse
    assert lib.usv_eval_mark(c, _capi.byref(b_null), _capi.byref(ok), None) == 1
    assert lib.usv_eval_step(c, _capi.byref(b_null), _capi.byref(ok), p, None) == 1
    for k in (0, -3):
        assert calls(cfg, b, ev_of(k=k)) == [2, 2, 2, 2]
    b_big = UsvBufs()
    ctypes.memmove(ctypes.byref(b_big), ctypes.byref(b), ctypes.sizeof(b))
    b_big.n = 1 << 20
    assert calls(cfg, b_big, ev_of(k=1 << 12)) == [2, 2, 2, 2]   # max_episodes x n past 2^31 - 1
    for kind in ("USV_TASK_GO_TO_POSE", "USV_TASK_TRACK_XYO"):
        cfg.task_kind = DEFINES[kind]
        assert calls(cfg, b, ev_of()) == [3, 3, 3, 3]


def _cfg_thresholds(cfg_d):
    from omniisaacgymenvs_loop_amd.tasks.usv_config import build_usv_cfg
    return R.thresholds(build_usv_cfg(cfg_d))


@pytest.mark.parametrize("variant", ["A", "S"])
def test_restatement_reproduces_reference_records_of_fixture(eg, variant):
    tr, d, cfg_d = R.fixture_traj(variant, eg)
    got, dropped = R.restate(tr, _cfg_thresholds(cfg_d), R.K_EPISODES, float(eg[f"{variant}_control_dt"]))
    want = R.golden_records(eg, variant)
    R.assert_records(got, want, msg=f"episode_{variant}")
    assert dropped == int(eg[f"{variant}_dropped"])
    counts = {r: int((want["done_reason"] == i).sum()) for i, r in enumerate(R.REASONS)}
    assert counts == ({"collision": 10, "out_of_bounds": 2, "goal_tolerance": 0, "other": 0} if variant == "A" else
                      {"collision": 6, "out_of_bounds": 0, "goal_tolerance": 0, "other": 12})
    assert len(want["env"]) == int(d["reset"].sum())
    if variant == "S":   # every record names the scene its episode ran
        ends = np.argwhere(d["reset"].T != 0)   # (env, step) in env order
        by = {(int(e), int(k)): i for i, (e, k) in enumerate(zip(want["env"], want["episode"]))}
        seen = {}
        for e, t in ends:
            k = seen.get(int(e), 0)
            seen[int(e)] = k + 1
            assert want["scene_idx"][by[(int(e), k)]] == d["scene_last"][t, e]


def test_restatement_reproduces_reference_records_of_synthetic_set(eg):
    """The synthetic set has every branch (asserted when the fixture was written): success, collision, out of
    bounds, time-out, both priorities, a one-step episode, a still episode, the saturation threshold's float32
    neighbours, a dropped fourth ending, an env without an ending; also as one-env trajectories (n = 1)."""
    tr = R.synthetic_traj(eg)
    cfg_d = R.fixture_traj("A", eg)[2]
    thr = _cfg_thresholds(cfg_d)
    np.testing.assert_array_equal(np.float32(eg["C_thresholds"]), np.float32(list(thr.values())))
    assert tr["px"].shape == (24, 70)
    want = R.golden_records(eg, "C")
    got, dropped = R.restate(tr, thr, R.K_EPISODES, float(eg["C_control_dt"]))
    R.assert_records(got, want, msg="synthetic")
    assert dropped == int(eg["C_dropped"]) > 0
    assert set(want["done_reason"]) == {0, 1, 2, 3} and np.isnan(want["action_smoothness_mean"]).any()
    assert (want["path_length"] == 0).any() and not set(range(70)) <= set(want["env"])
    e = R.ENV_FOUR_ENDINGS
    got1, dropped1 = R.restate(R.select_env(tr, e), thr, R.K_EPISODES, float(eg["C_control_dt"]))
    sel = want["env"] == e
    want1 = {k: (np.zeros(sel.sum(), np.int32) if k == "env" else v[sel]) for k, v in want.items()}
    R.assert_records(got1, want1, msg="synthetic n=1")
    assert dropped1 == 1


def _hand_table():
    from omniisaacgymenvs_loop_amd._abi import DEFINES
    from omniisaacgymenvs_loop_amd.eval.report import table_to_episodes
    n, K = 3, 2
    tab = np.zeros((DEFINES["USV_EV_ROWS"], K * n))
    ep_count = np.array([2, 0, 3], np.int32)   # env 1 finished nothing, env 2 dropped one
    row = lambda k: DEFINES[f"USV_EV_{k}"]   # noqa: E731
    cols = [0, 2, 3, 5]
    tab[row("REASON"), cols] = [0, 3, 1, 3]
    tab[row("COLLISION"), cols] = [1, 0, 0, 0]
    tab[row("OOB"), cols] = [0, 0, 1, 0]
    tab[row("LEN_STEPS"), cols] = [5, 1, 7, 200]
    tab[row("TIME_TO_GOAL")] = np.nan
    tab[row("SMOOTH_MEAN"), cols] = [0.25, np.nan, 0.5, 0.125]
    tab[row("RETURN"), cols] = [1.5, -2.0, 0.1 + 0.2, 4.0]
    tab[row("PATH_EFF"), cols] = [0.5, 1.0, 0.75, 0.25]
    tab[row("SAT_RATE"), cols] = [0.0, 0.5, 1.0, 0.25]
    tab[row("SCENE_IDX")] = -1
    tab[row("END_YAW"), cols] = np.float32([0.1, -3.0, 2.5, 0.0])
    return table_to_episodes(tab, ep_count, K), int(np.maximum(ep_count - K, 0).sum())


def test_csv_columns_nan_rendering_and_round_trip(tmp_path):
    from omniisaacgymenvs_loop_amd.eval import CSV_COLUMNS, write_csv
    ep, _ = _hand_table()
    assert list(ep["env"]) == [0, 2, 0, 2] and list(ep["episode"]) == [0, 0, 1, 1]
    path = str(tmp_path / "eval.csv")
    assert write_csv(path, ep, control_dt=0.2, reward_scale=0.5) == 4
    rows = list(csv.reader(open(path)))
    assert tuple(rows[0]) == CSV_COLUMNS
    # the reference's columns first, in its order, then this project's
    assert rows[0][:16] == ["success", "done_reason", "episode_len_steps", "time_to_goal_sec", "return_raw",
                            "return_scaled", "path_length", "straight_line_dist", "path_efficiency",
                            "action_smoothness_mean", "action_smoothness_sum", "action_saturation_rate", "collision",
                            "out_of_bounds", "control_dt", "reward_scale"]
    assert rows[0][16:] == ["env", "episode", "scene_idx", "start_x", "start_y", "goal_x", "goal_y", "end_x", "end_y",
                            "end_yaw", "min_obs_dist_end", "min_obs_dist_episode", "env_done_succ", "env_done_coll"]
    recs = [dict(zip(rows[0], r)) for r in rows[1:]]
    assert [r["done_reason"] for r in recs] == ["collision", "other", "out_of_bounds", "other"]
    assert all(r["time_to_goal_sec"] == "nan" for r in recs) and recs[1]["action_smoothness_mean"] == "nan"
    assert [r["episode_len_steps"] for r in recs] == ["5", "1", "7", "200"] and recs[0]["scene_idx"] == "-1"
    assert float(recs[2]["return_raw"]) == 0.1 + 0.2 and float(recs[2]["return_scaled"]) == (0.1 + 0.2) * 0.5
    assert np.float32(float(recs[1]["end_yaw"])) == np.float32(-3.0) and recs[0]["control_dt"] == "0.2"


def test_summary_host_code_and_all_nan_metric(tmp_path):
    from omniisaacgymenvs_loop_amd._abi import DEFINES
    from omniisaacgymenvs_loop_amd.eval import (SUMMARY_METRICS, format_summary, summarize_host, summary_from_device,
                                                write_summary_json)
    ep, dropped = _hand_table()
    s = summarize_host(ep, dropped)
    assert s["episodes"] == 4 and s["dropped"] == 1 and s["collision"] == 1 and s["out_of_bounds"] == 1
    assert s["done_reason"] == {"collision": 1, "out_of_bounds": 1, "goal_tolerance": 0, "other": 2}
    ttg = s["metrics"]["time_to_goal_sec"]   # no finite value: count 0, mean NaN
    assert ttg["count"] == 0 and math.isnan(ttg["mean"]) and math.isnan(ttg["std"]) and math.isnan(ttg["ci95_lo"])
    sm = s["metrics"]["action_smoothness_mean"]   # NaN of the one-step episode left out
    assert sm["count"] == 3 and sm["mean"] == pytest.approx((0.25 + 0.5 + 0.125) / 3)
    ret = s["metrics"]["return_raw"]
    v = np.array([1.5, -2.0, 0.1 + 0.2, 4.0])
    assert ret["mean"] == pytest.approx(v.mean()) and ret["std"] == pytest.approx(v.std())
    assert ret["ci95_hi"] - ret["mean"] == pytest.approx(1.96 * v.std() / 2.0)
    # the device vector maps to the same dict
    out = np.zeros(DEFINES["USV_EVS_N"])
    out[:8] = [4, 1, 1, 1, 0, 2, 1, 1]
    for i, k in enumerate(SUMMARY_METRICS):
        m = s["metrics"][k]
        out[8 + 3 * i:11 + 3 * i] = [m["count"], m["mean"], m["std"]]
    s_dev = summary_from_device(out)
    assert json.dumps(s_dev, sort_keys=True) == json.dumps(s, sort_keys=True)
    txt = format_summary(s)
    assert "time_to_goal_sec: mean=nan std=nan 95%CI=[nan, nan]" in txt and txt.count("95%CI") == 6
    path = str(tmp_path / "summary.json")
    write_summary_json(path, s)
    back = json.load(open(path))   # strict JSON: NaN written as null
    assert back["metrics"]["time_to_goal_sec"] == {"count": 0, "mean": None, "std": None, "ci95_lo": None,
                                                  "ci95_hi": None}
    assert back["metrics"]["return_raw"]["mean"] == ret["mean"]
