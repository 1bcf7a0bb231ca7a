"""Generate the GoToXY / KeepXY / TrackXYVelocity episode fixtures (episode_X / episode_K / episode_V.npz) by
running the REFERENCE's task classes on the CPU under make_golden.py's harness.

Run only where the reference checkout exists (see make_golden.py):
    python tests/golden/make_task_golden.py [--only X|K|V]

The stubs, the fake Heron / world, the torch.rand / torch.cos / torch.sin recorders and the draw mapping are
make_golden's; the config is the TEST yaml with the task's own task / reward parameters, as variants P / T / Q.
Harness steps the three task classes need on the current glue, beyond those of P / T:
  * TrackXYVelocityTask.update_kills() takes no step argument (the glue passes one);
  * KeepXYTask.compute_reward reads self.positionposition and prints it each step: the attribute is set and
    stdout swallowed.
The format is episode_P's (without tgt_h: these tasks have no third target component).

What each fixture must hold (asserted by tests/test_tasks_cpu.py): a done by every cause its task has -- X and
V: goal counter, distance, time-out; K: distance and time-out with goal_cnt identically 0 -- and resets in at
least 10 different steps.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

OUT = MG.OUT
N_ENVS, STEPS = 8, 60
TASK_OF = {"X": "GoToXY", "K": "KeepXY", "V": "TrackXYVelocity"}
# the reset path's torch.cos / torch.sin calls of the three tasks -> RU_TRIG offsets (spawn angle 0 / 1, half yaw 2 / 3)
MG.TRIG_SITES.update({("USV_go_to_xy.py", 309): 0, ("USV_go_to_xy.py", 312): 1, ("USV_go_to_xy.py", 319): 2,
                      ("USV_go_to_xy.py", 320): 3, ("USV_keep_xy.py", 268): 0, ("USV_keep_xy.py", 271): 1,
                      ("USV_keep_xy.py", 278): 2, ("USV_keep_xy.py", 279): 3,
                      ("USV_track_xy_velocity.py", 168): 2, ("USV_track_xy_velocity.py", 169): 3})
# TrackXYVelocityTask.get_spawns draws the yaw only (the generic get_spawns mapping starts at the spawn radius)
MG.POSE_SITES[("USV_track_xy_velocity.py", 167)] = MG.RU["YAW"]


def task_cfg(variant: str):
    cfg = MG.load_task_cfg("A")   # the TEST yaml, scene replay off
    env = cfg["env"]
    if variant == "X":
        # GoToXY: the three kill causes within short episodes; penalize_action_variation on, fed the policy's
        # actions (penalties_use_thrust_u off: with it the reference compares a tensor with itself)
        env["task_parameters"] = dict(name="GoToXY", goal_random_position=2.0, position_tolerance=0.5,
                                      min_spawn_dist=0.3, max_spawn_dist=3.0, kill_dist=3.5,
                                      kill_after_n_steps_in_tolerance=3, boundary_cost=25.0, goal_reward=10.0,
                                      time_reward=-0.1)
        env["reward_parameters"] = dict(name="GoToXY", reward_mode="exponential", exponential_reward_coeff=0.25)
        env["penalties_parameters"]["penalize_action_variation"] = True
        env["action_processing"]["penalties_use_thrust_u"] = False
        env["maxEpisodeLength"] = 25
    elif variant == "K":
        # KeepXY with the spawn curriculum across warmup and end within 60 steps, as variant Q
        env["task_parameters"] = dict(name="KeepXY", goal_random_position=2.0, position_tolerance=0.5,
                                      kill_after_n_steps_in_tolerance=1, spawn_curriculum=True,
                                      spawn_curriculum_min_dist=0.2, spawn_curriculum_max_dist=1.5,
                                      spawn_curriculum_kill_dist=2.5, spawn_curriculum_warmup=1,
                                      spawn_curriculum_end=3, min_spawn_dist=0.3, max_spawn_dist=3.0, kill_dist=3.5)
        env["reward_parameters"] = dict(name="KeepXY", reward_mode="exponential", exponential_reward_coeff=0.25)
        env["maxEpisodeLength"] = 9
    elif variant == "V":
        env["task_parameters"] = dict(name="TrackXYVelocity", lin_vel_tolerance=0.5,
                                      kill_after_n_steps_in_tolerance=2, kill_dist=2.5, goal_random_velocity=0.75)
        env["reward_parameters"] = dict(name="TrackXYVelocity", reward_mode="exponential",
                                        exponential_reward_coeff=0.25)
        env["maxEpisodeLength"] = 12
    else:
        raise ValueError(variant)
    return cfg


def build(torch, n, variant):
    cfg = task_cfg(variant)
    load = MG.load_task_cfg
    MG.load_task_cfg = lambda _v: cfg
    try:
        usv, heron, world, cfg = MG.build_usv(torch, n, "P")   # P: the A20 harness fixes (task_data block, markers)
    finally:
        MG.load_task_cfg = load
    t = usv.task
    assert type(t).__name__ == TASK_OF[variant] + "Task", type(t).__name__
    if variant == "V":
        t.update_kills = lambda *a: type(t).update_kills(t)
    if variant == "K":
        t.positionposition = 0
    return usv, heron, world, cfg


def _targets(task):
    tgt = task._target_velocities if hasattr(task, "_target_velocities") else task._target_positions
    return tgt.numpy().copy()


def gen_episode(torch, variant, n=N_ENVS, steps=STEPS, seed=11):
    torch.manual_seed(seed)
    usv, heron, world, cfg = build(torch, n, variant)
    ve = MG.make_vecenv(torch, usv, world)
    rec, trec = MG.RandRecorder(torch), MG.TrigRecorder(torch)
    rng = np.random.default_rng(seed)
    quiet = contextlib.redirect_stdout(io.StringIO())
    with rec, trec:
        usv.post_reset()
        usv.update_state()   # the cached root_* state of the first step (make_golden's module doc)
        init_tgt = _targets(usv.task)
        usv.task.reset(torch.arange(n))
        rec.take()
        trec.take()
    keys = ("actions", "obs", "rew", "reset", "progress", "px", "py", "yaw", "vx", "vy", "wz", "fl", "fr", "reset_mask",
            "u_step", "mass", "com", "k_drag", "thr_l", "thr_r", "k_iz", "obst", "tgt", "extras", "goal_cnt", "bias",
            "terms")
    data = {k: [] for k in keys}
    reset_U = []
    noise = ("add_noise_on_vel", "add_noise_on_heading", "add_noise_on_pos", "add_noise_on_act")
    with rec, trec, quiet:
        for t in range(steps):
            reset_mask = usv.reset_buf.numpy().astype(bool).copy() if t > 0 else np.ones(n, bool)
            if t == 0:
                usv.reset()
                act = np.zeros((n, 2), np.float32)
            else:
                act = MG.policy_actions(rng, n, t)
            bias_active = (usv._initial_action_bias_steps > 0 and
                           usv._action_bias_step_count < usv._initial_action_bias_steps)
            obs_dict, rew, resets, extras = ve.step(torch.from_numpy(act))
            draws = rec.take()
            Us, _ = MG.map_step_draws(draws, n)
            k = int(reset_mask.sum())
            trig = trec.take()
            reset_draws = [d for d in draws if d[0] not in noise]
            if k:
                Ur = MG.map_reset_draws(reset_draws, k)
                Ur[:, MG.RU["TRIG"]:MG.RU["TRIG"] + 6] = MG.map_reset_trig(trig, k)
                reset_U.append(Ur)
            else:
                assert not reset_draws and not trig, (reset_draws, trig)
            data["actions"].append(act)
            data["bias"].append(np.float32(usv._initial_action_bias if bias_active else 0.0))
            data["obs"].append(obs_dict["obs"]["state"].numpy().copy())
            data["rew"].append(rew.numpy().copy())
            data["reset"].append(resets.numpy().copy())
            data["progress"].append(usv.progress_buf.numpy().copy())
            data["reset_mask"].append(reset_mask)
            data["u_step"].append(Us)
            for key in ("px", "py", "yaw", "vx", "vy", "wz"):
                data[key].append(getattr(heron, key).numpy().copy())
            cf = usv.thrusters_dynamics.current_forces.numpy().copy()
            data["fl"].append(cf[:, 0])
            data["fr"].append(cf[:, 1])
            data["mass"].append(usv.MDD.platforms_mass[:, 0].numpy().copy())
            data["com"].append(usv.MDD.platforms_CoM.numpy().copy())
            data["k_drag"].append(usv.hydrodynamics.drag_scale[:, 0].numpy().copy())
            td = usv.thrusters_dynamics
            assert not td._use_separate_randomization   # the TEST yaml's coupled thruster multiplier
            data["thr_l"].append(td.thruster_multiplier[:, 0].numpy().copy())
            data["thr_r"].append(td.thruster_multiplier[:, 0].numpy().copy())
            data["k_iz"].append(usv.k_Iz[:, 0].numpy().copy())
            data["obst"].append(np.zeros((n, 16, 2), np.float32))
            data["terms"].append(np.zeros((n, 15), np.float32))
            data["tgt"].append(_targets(usv.task))
            data["goal_cnt"].append(usv.task._goal_reached.numpy().copy())
            ex = extras.get("episode", {})
            data["extras"].append(np.array([float(ex[k]) if k in ex else np.nan for k in usv.episode_sums.keys()],
                                           np.float32))
    out = {k: np.stack(v) for k, v in data.items()}
    out["reset_U"] = np.concatenate(reset_U, 0)
    out["init_tgt"] = init_tgt
    out["grid_lin"] = np.zeros(150, np.float32)
    out["config_json"] = np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8)
    out["bias_steps"] = np.int64(usv._initial_action_bias_steps)
    out["extras_names"] = np.array(list(usv.episode_sums.keys()))
    np.savez_compressed(os.path.join(OUT, f"episode_{variant}.npz"), **out)
    print(f"episode_{variant}: resets per step", out["reset_mask"].sum(1).tolist(), "goal_cnt max",
          int(out["goal_cnt"].max()), "keys", list(usv.episode_sums.keys()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(TASK_OF), default=None)
    args = ap.parse_args()
    MG.install_stubs()
    import torch
    torch.set_num_threads(1)
    for v in ([args.only] if args.only else ["X", "K", "V"]):
        gen_episode(torch, v)


if __name__ == "__main__":
    main()
