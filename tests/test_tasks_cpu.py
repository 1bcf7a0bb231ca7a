"""GoToXY / KeepXY / TrackXYVelocity on the CPU: the packaged configs, the ABI, the fixtures' own conditions and
the restatement (tests/task_restate.py) against the reference's recorded episodes X / K / V
(tests/golden/make_task_golden.py).  Dones and goal counters exactly; floats at rtol = atol = 1e-5."""
import json
import os

import numpy as np
import pytest

from omniisaacgymenvs_loop_amd import _abi
from omniisaacgymenvs_loop_amd.tasks.usv_config import TASK_KINDS, build_usv_cfg, load_yaml, stat_names
from tests import task_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "omniisaacgymenvs_loop_amd", "cfg", "task", "USV")
FIXTURE = {"X": "GoToXY", "K": "KeepXY", "V": "TrackXYVelocity"}
STATE_STATS = ["normed_linear_vel", "normed_angular_vel", "cmd_neg_rate", "u_mean", "u_low_rate", "u_sum"]
TASK_STATS = {"GoToXY": ["distance_reward", "alignment_reward", "position_error", "boundary_penalty", "boundary_dist"],
              "KeepXY": ["position_reward", "position_error", "boundary_penalty", "boundary_dist"],
              "TrackXYVelocity": ["velocity_reward", "velocity_error"]}
STATE_KEYS = ("px", "py", "yaw", "vx", "vy", "wz")


def _yaml(name):
    return load_yaml(os.path.join(CFG, f"USV_Virtual_{name}.yaml"))


@pytest.mark.parametrize("name", sorted(FIXTURE.values()))
def test_packaged_yaml_loads(name):
    y = _yaml(name)
    c = build_usv_cfg(y)
    assert c.task_kind == TASK_KINDS[name] == _abi.DEFINES[{"GoToXY": "USV_TASK_GO_TO_XY", "KeepXY": "USV_TASK_KEEP_XY",
                                                            "TrackXYVelocity": "USV_TASK_TRACK_XY"}[name]]
    names = [k for k, _ in stat_names(c)]
    pens = ["angular_vel_penalty", "angular_vel_variation_penalty", "energy_penalty"]
    if name == "GoToXY":   # the reference's GoToXY yaml turns penalize_action_variation on
        assert c.pen_actv_kind == _abi.PEN["PEN_EXPABS"]
        pens.append("action_variation_penalty")
    else:
        assert c.pen_actv_kind == 0
    assert names == TASK_STATS[name] + pens + ["success", "collision"] + STATE_STATS
    slots = [s for _, s in stat_names(c)]
    assert len(set(slots)) == len(slots) and max(slots) < _abi.DEFINES["USV_NSTAT"]
    assert slots[:len(TASK_STATS[name])] == list(range(len(TASK_STATS[name])))
    assert c.kill_after_ge == (0 if name == "TrackXYVelocity" else 1)
    tp = y["env"]["task_parameters"]
    assert c.kill_after_n == tp["kill_after_n_steps_in_tolerance"] and c.kill_dist == pytest.approx(tp["kill_dist"])
    if name == "TrackXYVelocity":
        assert (c.goal_random_velocity, c.tk_tol[0], c.tk_mode[0], c.tk_coeff[0]) == pytest.approx((0.75, 0.01, 2, 0.25))
    elif name == "KeepXY":
        assert (c.tk_mode[0], c.tk_coeff[0], c.spawn_rmin, c.spawn_rmax) == pytest.approx((2, 0.25, 0.3, 3.0))
    else:
        assert (c.reward_mode, c.position_scale, c.exp_coeff, c.goal_reward, c.time_reward, c.boundary_cost) == \
            pytest.approx((0, 1.0, 0.25, 0.0, -0.1, 25.0))
        assert (c.align_la1, c.align_la2, c.align_la3) == pytest.approx((0.05, -10.0, -0.1))


@pytest.mark.parametrize("name", ["GoToXY", "KeepXY"])
def test_parameter_defaults_are_the_tasks_own(name):
    """GoToXYParameters / KeepXYParameters: 0.1 / 1 / 0 / 11 / 0.5 / 20 / 25 / 100 / -0.1, and a bare
    spawn_curriculum=True takes 0.2 / 3.0 / 30.0 / 250 / 1000 (GoToPose keeps 0.5 / 2.5 / 3.0 / 250 / 750)."""
    y = _yaml(name)
    y["env"]["task_parameters"] = {"name": name, "spawn_curriculum": True}
    y["env"]["reward_parameters"] = {"name": name}
    c = build_usv_cfg(y)
    assert c.curriculum_on == 1
    assert (c.cur_min_dist, c.cur_max_dist, c.cur_kill_dist, c.cur_warmup, c.cur_end) == \
        pytest.approx((0.2, 3.0, 30.0, 250.0, 1000.0))
    assert (c.position_tolerance, c.kill_after_n, c.goal_random_position, c.spawn_rmax, c.spawn_rmin, c.kill_dist,
            c.boundary_cost, c.goal_reward, c.time_reward) == pytest.approx((0.1, 1, 0.0, 11.0, 0.5, 20.0, 25.0, 100.0, -0.1))
    if name == "GoToXY":   # GoToXYReward
        assert (c.reward_mode, c.position_scale, c.exp_coeff, c.align_la1) == pytest.approx((2, 1.0, 0.15, 0.05))
    else:                  # KeepXYReward
        assert (c.tk_mode[0], c.tk_coeff[0]) == pytest.approx((0, 0.25))


def test_track_xy_velocity_defaults():
    y = _yaml("TrackXYVelocity")
    y["env"]["task_parameters"] = {"name": "TrackXYVelocity"}
    y["env"]["reward_parameters"] = {}
    c = build_usv_cfg(y)
    assert (c.tk_tol[0], c.kill_after_n, c.goal_random_velocity, c.kill_dist, c.tk_mode[0], c.tk_coeff[0]) == \
        pytest.approx((0.01, 50, 0.75, 500.0, 2, 0.25))


def test_action_variation_capture_xy_refuses_others_take_it():
    y = load_yaml(os.path.join(CFG, "IROS2024", "USV_Virtual_CaptureXY_SysID-TEST.yaml"))
    y["env"]["penalties_parameters"]["penalize_action_variation"] = True
    with pytest.raises(NotImplementedError):
        build_usv_cfg(y)
    y = _yaml("GoToPose")
    y["env"]["penalties_parameters"]["penalize_action_variation"] = True
    c = build_usv_cfg(y)
    assert c.pen_actv_kind == _abi.PEN["PEN_EXPABS"]
    assert ("action_variation_penalty", _abi.DEFINES["USV_ST_ACTION_VARIATION"]) in stat_names(c)


def test_abi_has_the_new_kinds_and_fields():
    names = {n: v for _, n, v in _abi.layout_entries()}
    assert (names["USV_TASK_CAPTURE_XY"], names["USV_TASK_GO_TO_POSE"], names["USV_TASK_TRACK_XYO"]) == (0, 1, 2)
    assert (names["USV_TASK_GO_TO_XY"], names["USV_TASK_KEEP_XY"], names["USV_TASK_TRACK_XY"]) == (3, 4, 5)
    assert names["USV_NSTAT"] == 28 and names["USV_NU_RESET"] == 718 and names["ST_SUCCESS"] == 11
    assert names["USV_ST_ACTION_VARIATION"] < names["ST_SUCCESS"]
    # appended after the fields that were there
    assert names["usv_cfg.inj_trig"] < names["usv_cfg.goal_random_velocity"] < names["usv_cfg.kill_after_ge"]
    assert names["usv_cfg.kill_after_ge"] + 4 <= names["sizeof usv_cfg"]
    with open(_abi.LAYOUT_GEN, encoding="utf-8") as f:
        assert f.read() == _abi.layout_header_text()


# ---------------------------------------------------------------------------------------------------------
# the recorded episodes
# ---------------------------------------------------------------------------------------------------------
def _replay(d):
    """The restatement over the fixture's recorded post-integration states; yields per-step results."""
    cfg_d = json.loads(bytes(d["config_json"]).decode())
    cfg = build_usv_cfg(cfg_d)
    T, n = d["obs"].shape[:2]
    names = [str(k) for k in d["extras_names"]]
    ep = R.Episode(cfg.task_kind, cfg, n, names, horizon=int(cfg_d["env"].get("horizon_length", 16)))
    for t in range(T):
        st = {k: d[k][t] for k in STATE_KEYS}
        cols, rew, dn, cnt, ex = ep.step(st, d["tgt"][t], d["actions"][t], d["reset_mask"][t], float(d["bias"][t]),
                                         d["u_step"][t])
        yield t, cfg, cols, rew, dn, cnt, ex, ep.cause


@pytest.mark.parametrize("variant", sorted(FIXTURE))
def test_restatement_reproduces_reference_episode(golden, variant):
    d = golden(f"episode_{variant}.npz")
    assert json.loads(bytes(d["config_json"]).decode())["env"]["task_parameters"]["name"] == FIXTURE[variant]
    c = build_usv_cfg(json.loads(bytes(d["config_json"]).decode()))
    assert [str(k) for k in d["extras_names"]] == [k for k, _ in stat_names(c)]   # the reference's own key order
    for t, cfg, cols, rew, dn, cnt, ex, _ in _replay(d):
        np.testing.assert_array_equal(dn, d["reset"][t], err_msg=f"dones t={t}")
        np.testing.assert_array_equal(cnt, d["goal_cnt"][t], err_msg=f"goal_cnt t={t}")
        np.testing.assert_allclose(cols, d["obs"][t][:, R.TASK_COLS], rtol=1e-5, atol=1e-5, err_msg=f"task cols t={t}")
        np.testing.assert_allclose(rew, d["rew"][t], rtol=1e-5, atol=1e-5, err_msg=f"rew t={t}")
        if ex is not None:
            np.testing.assert_allclose(ex, d["extras"][t], rtol=1e-5, atol=1e-5, err_msg=f"extras t={t}")


@pytest.mark.parametrize("variant", sorted(FIXTURE))
def test_fixture_holds_every_done_cause(golden, variant):
    """X, V: a done by the goal counter, by distance and by time-out; K: by distance and time-out, goal_cnt
    identically 0; resets in at least 10 different steps; at most 12 envs x 64 steps, no larger than episode_A."""
    d = golden(f"episode_{variant}.npz")
    T, n = d["obs"].shape[:2]
    assert T <= 64 and n <= 12
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", f"episode_{variant}.npz"))
    assert size <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "episode_A.npz"))
    assert int((d["reset_mask"].sum(1) > 0).sum()) >= 10
    by = {"counter": 0, "distance": 0, "timeout": 0}
    for t, cfg, cols, rew, dn, cnt, ex, cause in _replay(d):
        done = d["reset"][t].astype(bool)
        by["timeout"] += int((done & cause["timeout"]).sum())
        by["counter"] += int((done & ~cause["timeout"] & cause["counter"]).sum())
        by["distance"] += int((done & ~cause["timeout"] & ~cause["counter"] & cause["die"]).sum())
    assert by["timeout"] > 0 and by["distance"] > 0, by
    if variant == "K":
        assert by["counter"] == 0 and not d["goal_cnt"].any(), by
    else:
        assert by["counter"] > 0 and d["goal_cnt"].max() > 0, by
    if variant == "X":   # the action-variation penalty carries information (penalties_use_thrust_u off)
        i = [str(k) for k in d["extras_names"]].index("action_variation_penalty")
        assert np.abs(d["extras"][np.isfinite(d["extras"][:, i]), i]).max() > 0
    if variant == "K":   # the curriculum clock crosses warmup and end inside the episode
        c = build_usv_cfg(json.loads(bytes(d["config_json"]).decode()))
        assert c.curriculum_on and 1 / 16 < c.cur_warmup < c.cur_end < T / 16
