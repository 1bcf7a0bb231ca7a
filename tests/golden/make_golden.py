"""Generate the golden fixtures under tests/golden/ by importing the REFERENCE
(loop-Z/omniisaacgymenvs_loop at /root/reference) in the build container.

Run only where /root/reference exists:
    python tests/golden/make_golden.py [--only NAME]

Nothing here ships or runs on the GPU box; the committed .npz files are data
(inputs + reference outputs).  The reference needs Isaac Sim / PhysX / gym /
pytorch3d, none of which exist offline, so:
  * top-level modules omni, pxr, carb, gym, ray, tensorboardX, wandb, hydra,
    omegaconf, matplotlib are replaced by auto-stub modules;
  * pytorch3d.transforms.quaternion_to_matrix is restated (real-first quaternion);
  * PhysX is replaced by a fake Heron articulation view whose World.step()
    integrates the reference-computed forces with this build's 3-DoF
    semi-implicit Euler (the reference has no integrator of its own);
  * every torch.rand / torch.rand_like call is recorded with its call site so
    the oracle/kernels can replay the exact draws.
The task's cached root_* tensors are left as the reference leaves them: the
first substep after a reset computes drag and disturbances from the pre-reset
state.  The one harness step: update_state() runs once after
post_reset, so the very first step's cache holds the initial pose (the
reference zero-initialises root_quats, USV_Virtual.py:605, and
quaternion_to_matrix of a zero quaternion is 0/0).
"""
from __future__ import annotations

import argparse
import copy
import importlib.abc
import importlib.machinery
import json
import math
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))


# --------------------------------------------------------------------------
# offline stubs
# --------------------------------------------------------------------------
_ROOTS = {"omni", "pxr", "carb", "ray", "tensorboardX", "gym", "wandb", "hydra", "omegaconf", "matplotlib"}


class _Meta(type):
    def __getattr__(cls, name):
        return MagicMock()


class _Mod(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        if name[:1].isupper():
            c = _Meta(name, (object,), {"__init__": lambda self, *a, **k: None})
            setattr(self, name, c)
            return c
        m = MagicMock()
        setattr(self, name, m)
        return m


class _Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, fullname, path, target=None):
        if fullname.split(".")[0] in _ROOTS:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        m = _Mod(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, module):
        pass


def install_stubs():
    np.Inf = np.inf  # the reference predates NumPy 2
    sys.meta_path.insert(0, _Finder())
    import torch
    p3d = types.ModuleType("pytorch3d")
    tr = types.ModuleType("pytorch3d.transforms")

    def quaternion_to_matrix(q):  # pytorch3d.transforms.quaternion_to_matrix restated
        r, i, j, k = torch.unbind(q, -1)
        two_s = 2.0 / (q * q).sum(-1)
        o = torch.stack((
            1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
            two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
            two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
        return o.reshape(q.shape[:-1] + (3, 3))

    tr.quaternion_to_matrix = quaternion_to_matrix
    p3d.transforms = tr
    sys.modules["pytorch3d"] = p3d
    sys.modules["pytorch3d.transforms"] = tr
    # gym.spaces must behave enough for Box/Dict construction
    gym = sys.modules.get("gym") or __import__("gym")
    spaces = types.ModuleType("gym.spaces")

    class Box:
        def __init__(self, low, high, shape=None, dtype=np.float32):
            self.low, self.high = np.asarray(low), np.asarray(high)
            self.shape = self.low.shape if shape is None else shape
            self.dtype = np.dtype(dtype)

    class Dict:
        def __init__(self, d):
            self.spaces = d

    spaces.Box, spaces.Dict = Box, Dict
    spaces.Discrete = type("Discrete", (), {})
    spaces.Tuple = type("Tuple", (), {})
    sys.modules["gym.spaces"] = spaces
    gym.spaces = spaces
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "rl_games"))


# --------------------------------------------------------------------------
# torch.rand recorder
# --------------------------------------------------------------------------
class RandRecorder:
    def __init__(self, torch):
        self.torch = torch
        self.log = []
        self._rand = torch.rand
        self._rand_like = torch.rand_like

    def __enter__(self):
        torch = self.torch
        rec = self

        def rand(*a, **k):
            t = rec._rand(*a, **k)
            f = sys._getframe(1)
            rec.log.append((f.f_code.co_name, f.f_lineno, os.path.basename(f.f_code.co_filename), t.detach().clone()))
            return t

        def rand_like(x, *a, **k):
            t = rec._rand_like(x, *a, **k)
            f = sys._getframe(1)
            rec.log.append((f.f_code.co_name, f.f_lineno, os.path.basename(f.f_code.co_filename), t.detach().clone()))
            return t

        torch.rand = rand
        torch.rand_like = rand_like
        return self

    def __exit__(self, *exc):
        self.torch.rand = self._rand
        self.torch.rand_like = self._rand_like

    def take(self):
        out, self.log = self.log, []
        return out


# --------------------------------------------------------------------------
# torch.cos / torch.sin recorder: the reference's own values on the reset's state path
# --------------------------------------------------------------------------
# (file, line) of the reference call -> offset in the RU_TRIG slots (include/usv_hip.h)
TRIG_SITES = {("USV_capture_xy_static_obs.py", 955): 0, ("USV_capture_xy_static_obs.py", 956): 1,
              ("USV_capture_xy_static_obs.py", 960): 2, ("USV_capture_xy_static_obs.py", 961): 3,
              ("USV_go_to_pose.py", 307): 0, ("USV_go_to_pose.py", 310): 1,
              ("USV_go_to_pose.py", 317): 2, ("USV_go_to_pose.py", 318): 3,
              ("USV_track_xyo_velocity.py", 217): 2, ("USV_track_xyo_velocity.py", 218): 3,
              ("USV_Virtual.py", 1449): 2, ("USV_Virtual.py", 1450): 3,
              ("USV_disturbances.py", 380): 4, ("USV_disturbances.py", 381): 5}


class TrigRecorder:
    """Records torch.cos / torch.sin at TRIG_SITES: on the CPU they are MKL VML HA (closed source, within 0.6 ulp),
    which the build cannot restate bit for bit; the parity tests inject these values (usv_cfg_t.inj_trig) to follow
    the reference's state exactly, and check the build's own usv_sincos_cr against them separately."""

    def __init__(self, torch):
        self.torch = torch
        self.log = []
        self._cos, self._sin = torch.cos, torch.sin

    def _wrap(self, fn):
        rec = self

        def g(x, *a, **k):
            t = fn(x, *a, **k)
            f = sys._getframe(1)
            site = (os.path.basename(f.f_code.co_filename), f.f_lineno)
            if site in TRIG_SITES:
                rec.log.append((TRIG_SITES[site], t.detach().clone()))
            return t
        return g

    def __enter__(self):
        self.torch.cos, self.torch.sin = self._wrap(self._cos), self._wrap(self._sin)
        return self

    def __exit__(self, *exc):
        self.torch.cos, self.torch.sin = self._cos, self._sin

    def take(self):
        out, self.log = self.log, []
        return out


_ORACLE = None


def _oracle():
    """This build's C oracle (its usv_sincos / usv_atan2 define the stand-in's quaternion and yaw)."""
    global _ORACLE
    if _ORACLE is None:
        sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
        from oracle import oracle as O
        _ORACLE = O
    return _ORACLE


# --------------------------------------------------------------------------
# fake Isaac Sim articulation view + world (planar, this build's integrator)
# --------------------------------------------------------------------------
HERON_Y = 0.37765
HERON_IZZ = 8.061


class _Body:
    def __init__(self, owner, kind):
        self.o, self.kind = owner, kind

    def apply_forces_and_torques_at_pos(self, forces=None, torques=None, is_global=False, **kw):
        assert not is_global
        if self.kind == "base":
            self.o.f_base = forces.detach().clone()
            self.o.t_base = torques.detach().clone()
        elif self.kind == "left":
            self.o.f_left = forces.detach().clone()
        else:
            self.o.f_right = forces.detach().clone()

    def set_masses(self, masses, indices=None):
        self.o.mass[indices.long()] = masses.float()

    def set_coms(self, coms, indices=None):
        self.o.com[indices.long()] = coms.reshape(-1, 3).float()

    def get_inertias(self, indices=None, clone=True):
        if indices is None:
            return self.o.inertia.clone()
        return self.o.inertia[indices.long()].clone()

    def set_inertias(self, values, indices=None):
        self.o.inertia[indices.long()] = values.float()


class FakeHeron:
    """Planar stand-in for HeronView (robots/articulations/views/heron_view.py)."""

    name = "heron"
    num_dof = 2

    def __init__(self, torch, n):
        self.t = torch
        self.n = n
        z = lambda *s: torch.zeros(*s, dtype=torch.float32)
        self.px, self.py, self.yaw = z(n), z(n), z(n)
        self.vx, self.vy, self.wz = z(n), z(n), z(n)
        self.pz = torch.full((n,), 0.5)
        self.mass = torch.full((n,), 34.96)
        self.com = z(n, 3)
        self.inertia = z(n, 9)
        self.inertia[:, 0], self.inertia[:, 4], self.inertia[:, 8] = 1.0, 2.0, HERON_IZZ
        self.base = _Body(self, "base")
        self.thruster_left = _Body(self, "left")
        self.thruster_right = _Body(self, "right")
        self.f_base = self.t_base = self.f_left = self.f_right = None

    def quat(self):
        """The stand-in's pose as PhysX returns it: (cos(yaw/2), 0, 0, sin(yaw/2)) by this build's usv_sincos
        (oracle.sincos == csrc/usv_device.h:usv_quat_rot's half-angle sincos)."""
        t = self.t
        s, c = _oracle().sincos((self.yaw * 0.5).numpy())
        q = t.zeros(self.n, 4)
        q[:, 0] = t.from_numpy(c)
        q[:, 3] = t.from_numpy(s)
        return q

    def get_world_poses(self, clone=True):
        p = self.t.stack([self.px, self.py, self.pz], 1)
        return p.clone(), self.quat()

    def get_velocities(self, clone=True):
        t = self.t
        v = t.zeros(self.n, 6)
        v[:, 0], v[:, 1], v[:, 5] = self.vx, self.vy, self.wz
        return v

    def get_joint_positions(self):
        return self.t.zeros(self.n, 2)

    def get_joint_velocities(self):
        return self.t.zeros(self.n, 2)

    def set_joint_positions(self, *a, **k):
        pass

    def set_joint_velocities(self, *a, **k):
        pass

    def set_world_poses(self, pos, rot, indices=None):
        idx = indices.long()
        self.px[idx] = pos[:, 0].float()
        self.py[idx] = pos[:, 1].float()
        self.pz[idx] = pos[:, 2].float()
        w, z = rot[:, 0].float().numpy(), rot[:, 3].float().numpy()
        # the stand-in keeps a yaw: 2 atan2(z, w) by this build's usv_atan2 (csrc/usv_device.h:usv_yaw_of_quat)
        a = _oracle().math3(np.ascontiguousarray(w), np.ascontiguousarray(z))[2]
        self.yaw[idx] = self.t.from_numpy(np.float32(2.0) * a)

    def set_velocities(self, vel, indices=None):
        idx = indices.long()
        self.vx[idx] = vel[:, 0].float()
        self.vy[idx] = vel[:, 1].float()
        self.wz[idx] = vel[:, 5].float()

    def integrate(self, dt):
        """This build's 3-DoF semi-implicit Euler, fp32."""
        t = self.t
        fl = self.f_left[:, 0]
        fr = self.f_right[:, 0]
        X = (fl + fr) + self.f_base[:, 0]   # csrc/usv_env.hip k_env_step: thrusters, then the base wrench
        Y = self.f_base[:, 1]
        comy = self.com[:, 1]
        N = self.t_base[:, 2] + (-(HERON_Y - comy) * fl + (HERON_Y + comy) * fr)
        # the body-frame wrench rotated by R = quaternion_to_matrix(quat()) (csrc/usv_device.h:usv_quat_rot): the
        # integrator's own definition, the same R the reference's drag reads back
        q = self.quat()
        w, z = q[:, 0], q[:, 3]
        two_s = 2.0 / (w * w + z * z)
        c = 1.0 - two_s * (z * z)
        s = two_s * (z * w)
        m = self.mass
        izz = self.inertia[:, 8]
        ax = (c * X - s * Y) / m
        ay = (s * X + c * Y) / m
        aw = N / izz
        self.vx = self.vx + ax * dt
        self.vy = self.vy + ay * dt
        self.wz = self.wz + aw * dt
        self.px = self.px + self.vx * dt
        self.py = self.py + self.vy * dt
        yw = self.yaw + self.wz * dt
        pi = np.float32(math.pi)
        yw = t.where(yw > pi, yw - np.float32(2 * math.pi), yw)
        yw = t.where(yw <= -pi, yw + np.float32(2 * math.pi), yw)
        self.yaw = yw


class FakeWorld:
    def __init__(self, heron, dt):
        self.h, self.dt = heron, dt

    def is_playing(self):
        return True

    def step(self, render=False):
        self.h.integrate(self.dt)


def load_task_cfg(variant: str):
    import yaml
    with open(os.path.join(REF, "omniisaacgymenvs/cfg/task/USV/IROS2024/USV_Virtual_CaptureXY_SysID-TEST.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["env"]["scene_replay"]["enabled"] = False
    cfg["physics_engine"] = "physx"
    if variant == "B":
        # second parity variant: bias ends early, independent (non-coupled)
        # randomisations, centered priv encoding, exponential reward, pos noise
        env = cfg["env"]
        env["action_processing"]["initial_action_bias_steps"] = 3
        env["disturbances"]["coupling"]["mass_driven"]["enabled"] = False
        env["disturbances"]["drag"]["use_drag_scale_randomization"] = True
        env["disturbances"]["thruster"]["use_thruster_randomization"] = True
        env["disturbances"]["thruster"]["use_separate_randomization"] = True
        env["disturbances"]["thruster"]["left_rand"] = 0.3
        env["disturbances"]["thruster"]["right_rand"] = 0.2
        env["disturbances"]["observations"]["add_noise_on_pos"] = True
        env["privileged_params"]["mode"] = "centered"
        env["reward_parameters"]["reward_mode"] = "exponential"
        env["task_parameters"]["goal_random_position"] = 0.0
        env["maxEpisodeLength"] = 40
    if variant == "C":
        # disturbance variant: constant + sinusoidal force and torque disturbances
        # (USV_disturbances.py:268-530) and a water current (Hydrodynamics.py:224-237)
        env = cfg["env"]
        for key in ("use_force_disturbance", "use_constant_force", "use_sinusoidal_force"):
            env["disturbances"]["forces"][key] = True
        for key in ("use_torque_disturbance", "use_constant_torque", "use_sinusoidal_torque"):
            env["disturbances"]["torques"][key] = True
        env["water_current"]["use_water_current"] = True
        env["water_current"]["flow_velocity"] = [0.3, -0.2, 0.0]
        env["maxEpisodeLength"] = 30
    if variant == "D":
        # 8f-4 modes: priv_dim 4 (the 29-column obs of every reference yaml but TEST) and a
        # global observation frame (USV_core.py:103-112)
        env = cfg["env"]
        env.pop("mass_dim", None)
        env["priv_dim"] = 4
        env["observation_frame"] = "global"
        env["maxEpisodeLength"] = 30
    if variant == "E":
        # privileged tail from the base (nominal) mass / CoM, raw encodings (USV_Virtual.py:455-520)
        env = cfg["env"]
        m = env["disturbances"]["mass"]
        m["masscom_obs_source"] = "base"
        m["mass_obs_mode"] = "raw"
        m["com_obs_mode"] = "raw"
        env["privileged_params"]["mode"] = "raw"
        env["maxEpisodeLength"] = 30
    if variant == "S":
        # scene replay (8f-2): deterministic scenes from tests/golden/scenes_S.npz
        sr = cfg["env"]["scene_replay"]
        sr.update(enabled=True, npz_path=os.path.join(OUT, "scenes_S.npz"), start_index=2, cycle=True,
                  strict_hash=True)
        cfg["env"]["maxEpisodeLength"] = 24
    if variant in ("P", "T", "Q"):
        # SURVEY A20 tasks on the TEST glue: the task's own yaml task/reward parameters
        # (cfg/task/USV/USV_Virtual_GoToPose.yaml, USV_Virtual_TrackXYOVelocity.yaml)
        import yaml
        name = "USV_Virtual_TrackXYOVelocity.yaml" if variant == "T" else "USV_Virtual_GoToPose.yaml"
        with open(os.path.join(REF, "omniisaacgymenvs/cfg/task/USV", name)) as f:
            tcfg = yaml.safe_load(f)
        env = cfg["env"]
        env["task_parameters"] = dict(tcfg["env"]["task_parameters"])
        env["reward_parameters"] = dict(tcfg["env"]["reward_parameters"])
        if variant in ("P", "Q"):
            env["task_parameters"]["goal_random_position"] = 2.0
            env["task_parameters"]["position_tolerance"] = 0.3   # reachable within the short episode
        env["maxEpisodeLength"] = 40
        if variant == "Q":
            # the GoToPose spawn curriculum (USV_go_to_pose.py:188-202, 266-290) across its three regimes
            # within 64 steps: USVVirtual.step = steps / 16 < warmup 1, between 1 and 3, > end 3; short
            # episodes so resets land in every regime, kill distances small enough to kill
            env["task_parameters"].update(spawn_curriculum=True, spawn_curriculum_min_dist=0.2,
                                          spawn_curriculum_max_dist=1.5, spawn_curriculum_kill_dist=2.5,
                                          spawn_curriculum_warmup=1, spawn_curriculum_end=3,
                                          min_spawn_dist=0.3, max_spawn_dist=3.0, kill_dist=3.5)
            env["maxEpisodeLength"] = 9
    return cfg


def build_usv(torch, n, variant):
    from omniisaacgymenvs.tasks.base import rl_task
    from omniisaacgymenvs.tasks import USV_Virtual as UV

    def rl_init(self, name, env, offset=None):
        self.test = False
        self._device = "cpu"
        self.randomize_actions = False
        self.randomize_observations = False
        self.clip_obs = self._cfg["task"]["env"].get("clipObservations", np.inf)
        self.clip_actions = self._cfg["task"]["env"].get("clipActions", np.inf)
        self.rl_device = "cpu"
        self.control_frequency_inv = self._cfg["task"]["env"].get("controlFrequencyInv", 1)
        self._env = env
        self._num_agents = 1
        self._num_states = 0
        self.cleanup()

    rl_task.RLTask.__init__ = rl_init
    for prop, attr in (("num_envs", "_num_envs"), ("num_observations", "_num_observations"),
                       ("num_actions", "_num_actions"), ("num_states", "_num_states"),
                       ("num_agents", "_num_agents"), ("device", "_device")):
        setattr(rl_task.RLTask, prop, property(lambda self, a=attr: getattr(self, a)))
    task_cfg = load_task_cfg(variant)
    task_cfg["env"]["numEnvs"] = n
    sim_config = types.SimpleNamespace(config={"sim_device": "cpu", "test": False, "rl_device": "cpu",
                                               "task": task_cfg},
                                       task_config=task_cfg)
    heron = FakeHeron(torch, n)
    world = FakeWorld(heron, task_cfg["sim"]["dt"])
    fake_env = types.SimpleNamespace(_world=world)
    usv = UV.USVVirtual("USVVirtual", sim_config, fake_env)
    usv._heron = heron
    usv._env_pos = torch.zeros((n, 3))
    usv.task._env = usv
    if variant in ("P", "T", "Q"):
        # the live glue cannot run these tasks; minimal harness fixes:
        # Core's 20-column task_data block, the marker buffer set_targets reads, and
        # update_kills(step) called with the extra current_state argument
        t = usv.task
        t._task_data = torch.zeros((n, t._num_observations - 3 - t.action_dim - t.priv_dim))
        t._blue_pin_positions = torch.zeros((n, 16, 3))
        orig_kills = t.update_kills
        t.update_kills = lambda step, *a: orig_kills(step)
    usv.get_USV_dynamics()
    usv._marker = None
    usv._blue_markers = [None] * 16
    return usv, heron, world, task_cfg


def make_vecenv(torch, usv, world):
    from omniisaacgymenvs.envs import vec_env_rlgames as VE
    ve = VE.VecEnvRLGames.__new__(VE.VecEnvRLGames)
    ve._task = usv
    ve._world = world
    ve._render = False
    ve.sim_frame_count = 0
    ve._loopz_first_step_trace_done = True
    return ve


# --------------------------------------------------------------------------
# draw-site mapping into the kernel layouts (include/usv_hip.h RU_* / SU_*)
# --------------------------------------------------------------------------
RU = dict(MASS=0, COM=1, KIZ=4, KDRAG=5, THR=6, DRAG=8, SPAWN_R=20, SPAWN_TH=21, YAW=22, OBST=23,
          RESAMPLE=55, VX=695, VY=696, GOAL=697, FSIN=699, FCONST=704, TSIN=706, TCONST=709)
NU_RESET, NU_STEP = 718, 8
RU["GOAL_H"] = 711
RU["TRIG"] = 712
# draw sites of the GoToPose / TrackXYOVelocity spawn + goal generators
POSE_SITES = {("USV_go_to_pose.py", 240): RU["GOAL"], ("USV_go_to_pose.py", 248): RU["GOAL_H"],
              ("USV_go_to_pose.py", 305): RU["SPAWN_R"], ("USV_go_to_pose.py", 306): RU["SPAWN_TH"],
              ("USV_go_to_pose.py", 316): RU["YAW"], ("USV_track_xyo_velocity.py", 187): RU["GOAL"],
              ("USV_track_xyo_velocity.py", 193): RU["GOAL_H"], ("USV_track_xyo_velocity.py", 216): RU["YAW"]}
# draw sites of the disturbance generators (USV_disturbances.py line -> slot)
DIST_SITES = {("generate_force", 342): RU["FSIN"], ("generate_force", 347): RU["FSIN"] + 1,
              ("generate_force", 352): RU["FSIN"] + 2, ("generate_force", 357): RU["FSIN"] + 3,
              ("generate_force", 362): RU["FSIN"] + 4, ("generate_force", 369): RU["FCONST"],
              ("generate_force", 374): RU["FCONST"] + 1, ("generate_torque", 484): RU["TSIN"],
              ("generate_torque", 489): RU["TSIN"] + 1, ("generate_torque", 494): RU["TSIN"] + 2,
              ("generate_torque", 500): RU["TCONST"], ("generate_torque", 506): RU["TCONST"] + 1}


def map_reset_draws(draws, k):
    U = np.full((k, NU_RESET), np.nan, np.float32)
    it = 0
    vel = 0
    spawn = 0
    for fn, line, fname, t in draws:
        a = t.numpy().astype(np.float32)
        if (fname, line) in POSE_SITES:
            slot = POSE_SITES[(fname, line)]
            w = 2 if slot == RU["GOAL"] else 1
            U[:, slot:slot + w] = a.reshape(k, w)
        elif fn == "randomize_masses":
            U[:, RU["MASS"]] = a.reshape(k)
        elif fn == "_randomize_com":
            U[:, RU["COM"]:RU["COM"] + a.reshape(k, -1).shape[1]] = a.reshape(k, -1)
        elif fn == "_sample_k_drag":
            U[:, RU["KDRAG"]] = a.reshape(k)
        elif fn == "_sample_k_iz":
            U[:, RU["KIZ"]] = a.reshape(k)
        elif fn == "reset_thruster_randomization":
            col = RU["THR"] + (1 if (not np.isnan(U[0, RU["THR"]]) and fn == "reset_thruster_randomization") else 0)
            U[:, col] = a.reshape(k)
        elif fn == "reset_coefficients":
            off = RU["DRAG"] if np.isnan(U[0, RU["DRAG"]]) else RU["DRAG"] + 6
            U[:, off:off + 6] = a.reshape(k, 6)
        elif fn == "get_spawns":
            if a.ndim == 1:
                U[:, [RU["SPAWN_R"], RU["SPAWN_TH"], RU["YAW"]][spawn]] = a
                spawn += 1
            elif a.shape[1:] == (16, 2) and np.isnan(U[0, RU["OBST"]]):
                U[:, RU["OBST"]:RU["OBST"] + 32] = a.reshape(k, 32)
            else:
                U[:, RU["RESAMPLE"] + it * 32:RU["RESAMPLE"] + (it + 1) * 32] = a.reshape(k, 32)
                it += 1
        elif fn == "reset_idx":
            U[:, [RU["VX"], RU["VY"]][vel]] = a.reshape(k)
            vel += 1
        elif fn == "get_goals":
            U[:, RU["GOAL"]:RU["GOAL"] + 2] = a.reshape(k, 2)
        elif (fn, line) in DIST_SITES:
            U[:, DIST_SITES[(fn, line)]] = a.reshape(k)
        else:
            raise RuntimeError(f"unmapped reset draw site {fn}:{line} ({fname})")
    return U


def map_reset_trig(trig, k):
    """The recorded torch.cos / torch.sin values of one reset batch -> [k][6] (RU_TRIG offsets; NaN: not called)."""
    T = np.full((k, 6), np.nan, np.float32)
    for off, t in trig:
        T[:, off] = t.numpy().astype(np.float32).reshape(k)
    return T


def map_step_draws(draws, n):
    U = np.zeros((n, NU_STEP), np.float32)
    vel = [d for d in draws if d[0] == "add_noise_on_vel"]
    head = [d for d in draws if d[0] == "add_noise_on_heading"]
    pos = [d for d in draws if d[0] == "add_noise_on_pos"]
    act = [d for d in draws if d[0] == "add_noise_on_act"]
    if vel:
        v = vel[-1][3].numpy()
        U[:, 0], U[:, 1], U[:, 2] = v[:, 0], v[:, 1], v[:, 5]
    if head:
        U[:, 3] = head[-1][3].numpy()
    if pos:
        U[:, 4:6] = pos[-1][3].numpy()[:, :2]
    if act:
        U[:, 6:8] = act[-1][3].numpy()
    other = [d for d in draws if d[0] not in ("add_noise_on_vel", "add_noise_on_heading", "add_noise_on_pos",
                                             "add_noise_on_act")]
    return U, other


# --------------------------------------------------------------------------
# fixtures
# --------------------------------------------------------------------------
def gen_lut(torch):
    from omniisaacgymenvs.envs.USV.ThrusterDynamics import DynamicsFirstOrder
    cfg = load_task_cfg("A")
    th = cfg["dynamics"]["thrusters"]
    tcfg = cfg["env"]["disturbances"]["thruster"]
    res = {}
    tables = {
        "test": (th["interpolation"]["interpolationPointsFromRealDataLeft"],
                 th["interpolation"]["interpolationPointsFromRealDataRight"]),
        "sym": ([-40.0, -36.0, -32.0, -28.0, -24.0, -20.0, -16.0, -12.0, -8.0, -4.0, 0.0, 8.0, 16.0, 24.0, 32.0,
                 40.0, 48.0, 56.0, 64.0, 72.0, 80.0],
                [-3.8, -3.8, -3.6, -3.6, -1.6, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 4.0, 10.0, 15.0,
                 21.0, 23.0, 22.0]),
    }
    for name, (tl, tr) in tables.items():
        d = DynamicsFirstOrder(tcfg, 64, "cpu", th["timeConstant"], cfg["sim"]["dt"], 1000, tl, tr,
                               [0.0] * 5, [0.0] * 5, -1.0, 1.0)
        res[f"{name}_table_l"] = np.asarray(tl, np.float32)
        res[f"{name}_table_r"] = np.asarray(tr, np.float32)
        res[f"{name}_lut_l"] = d.y_linear_interp_left.numpy()
        res[f"{name}_lut_r"] = d.y_linear_interp_right.numpy()
        # index mapping + lag sequence
        g = torch.Generator().manual_seed(3)
        cmds = torch.rand((64, 2), generator=g) * 2 - 1
        cmds[:4] = torch.tensor([[-1.0, 1.0], [0.0, 0.5], [1.0, -1.0], [0.001, 0.999]])
        d.set_target_force(cmds)
        res[f"{name}_cmds"] = cmds.numpy()
        res[f"{name}_targets"] = d.thruster_forces_before_dynamics.numpy().copy()
        lag = []
        for _ in range(12):
            out = d.update_forces()
            lag.append(out[:, [0, 3]].numpy().copy())
        res[f"{name}_lag"] = np.stack(lag)
    np.savez_compressed(os.path.join(OUT, "lut.npz"), **res)


def gen_forces(torch):
    from omniisaacgymenvs.envs.USV.Hydrodynamics import HydrodynamicsObject
    cfg = load_task_cfg("A")
    hd = cfg["dynamics"]["hydrodynamics"]
    n = 256
    g = torch.Generator().manual_seed(5)
    dcfg = dict(cfg["env"]["disturbances"]["drag"])
    dcfg["use_drag_scale_randomization"] = True
    h = HydrodynamicsObject(dcfg, n, "cpu", 1000, -9.81, hd["linear_damping"], hd["quadratic_damping"],
                            hd["linear_damping_forward_speed"], hd["offset_linear_damping"],
                            hd["offset_lin_forward_damping_speed"], hd["offset_nonlin_damping"],
                            hd["scaling_damping"], 0.0, 1.0, 0.3, -10.0)
    kd = 1.0 + 0.5 * torch.rand((n, 1), generator=g)
    h.drag_scale[:, :] = kd
    yaw = (torch.rand(n, generator=g) * 2 - 1) * math.pi
    q = torch.zeros(n, 4)
    q[:, 0] = torch.cos(yaw * 0.5)
    q[:, 3] = torch.sin(yaw * 0.5)
    vel = torch.zeros(n, 6)
    vel[:, 0] = (torch.rand(n, generator=g) * 2 - 1) * 3
    vel[:, 1] = (torch.rand(n, generator=g) * 2 - 1) * 3
    vel[:, 5] = (torch.rand(n, generator=g) * 2 - 1) * 2
    drag = h.ComputeHydrodynamicsEffects(0.01, q, vel, False, [0, 0, 0])
    np.savez_compressed(os.path.join(OUT, "forces.npz"), yaw=yaw.numpy(), quat=q.numpy(), vel=vel.numpy(),
                        k_drag=kd.numpy()[:, 0], drag=drag.numpy(),
                        local_vel=h.local_velocities.numpy())


def gen_hydrostatics(torch):
    """HydrostaticsObject.compute_archimedes_metacentric_local (Hydrostatics.py:63-133) on the TEST
    config's constants, fed as USVVirtual.update_state feeds it (USV_Virtual.py:785-798): submerged
    volume from the root height, euler angles from USVVirtual.get_euler_angles (:815-835).  Rows
    0..127: random attitudes; rows 128..255: level attitudes (roll = pitch = 0, the planar model)."""
    import types as _types
    from omniisaacgymenvs.envs.USV.Hydrostatics import HydrostaticsObject
    from omniisaacgymenvs.tasks.USV_Virtual import USVVirtual
    cfg = load_task_cfg("A")
    hs = cfg["dynamics"]["hydrostatics"]
    grav = float(cfg["sim"]["gravity"][2])
    n = 256
    g = torch.Generator().manual_seed(23)
    h = HydrostaticsObject(n, "cpu", hs["water_density"], grav, hs["box_width"] / 2, hs["box_length"] / 2,
                           hs["average_hydrostatics_force_value"], hs["amplify_torque"], 0.0, 1.0, 0.3, -10.0)
    q = torch.randn((n, 4), generator=g)
    yaw = (torch.rand(n // 2, generator=g) * 2 - 1) * math.pi
    q[n // 2:, 0] = torch.cos(yaw * 0.5)
    q[n // 2:, 1] = 0.0
    q[n // 2:, 2] = 0.0
    q[n // 2:, 3] = torch.sin(yaw * 0.5)
    q[:n // 2] = q[:n // 2] / q[:n // 2].norm(dim=1, keepdim=True)
    z = (torch.rand(n, generator=g) * 2 - 1) * 0.6
    zero_h = float(hs["heron_zero_height"])
    max_volume = hs["box_width"] * hs["box_length"] * (zero_h + 20)
    high = torch.clamp(zero_h - z, 0, zero_h + 20)
    vol = torch.clamp(high * hs["waterplane_area"], 0, max_volume)
    ns = _types.SimpleNamespace(euler_angles=torch.zeros((n, 3)))
    USVVirtual.get_euler_angles(ns, q)
    w = h.compute_archimedes_metacentric_local(vol, ns.euler_angles, q)
    np.savez_compressed(os.path.join(OUT, "hydrostatics.npz"), quat=q.numpy(), z=z.numpy(),
                        volume=vol.numpy(), euler=ns.euler_angles.numpy(), wrench=w.numpy(),
                        gravity=np.float32(grav))


class ScriptedExpert:
    """A frozen flat_expert for the imitation fixture (PPO(flat_expert=...) calls only .evaluate(obs),
    ppo.py:253-256): a fixed smooth map of the observation to actions in (-1, 1)."""

    def __init__(self, torch):
        g = torch.Generator().manual_seed(5)
        self.w = torch.randn((33, 2), generator=g) * 0.2
        self.torch = torch

    def evaluate(self, obs):
        with self.torch.no_grad():
            return self.torch.tanh(obs @ self.w)


def gen_loopz(torch, n=16, T=24, seed=7, sampling="in_order", expert=False):
    """The loopz trainer's PPO (omniisaacgymenvs/algo/ppo/{ppo,storage,module}.py) as
    scripts/rlgames_train.py:273-328 builds it (MLPEncode_wrap actor / critic, LeakyReLU, tanh actor
    output, squashed Gaussian init std 0.3, gamma 0.997, lambda 0.95, 4 x 4 in-order minibatches,
    lr 5e-4, max grad norm 0.5), fed a scripted rollout: T steps of observe() / step() on recorded
    observations, rewards and dones, then update().  Every Normal.sample draw is recorded (eps) and
    formed as loc + scale * eps; the squashed actions, log-probs, values, GAE returns / advantages,
    the parameters before and after the update, the Adam state and the mean losses are stored."""
    import torch.nn as nn
    tb = types.ModuleType("torch.utils.tensorboard")

    class _Writer:
        def __init__(self, *a, **k):
            pass

        def add_scalar(self, *a, **k):
            pass

    tb.SummaryWriter = _Writer
    sys.modules["torch.utils.tensorboard"] = tb
    import omniisaacgymenvs.algo.ppo.module as M
    import omniisaacgymenvs.algo.ppo.ppo as P
    gen = torch.Generator().manual_seed(seed + 100)
    draws = []

    class RecNormal(torch.distributions.Normal):
        def sample(self, sample_shape=torch.Size()):
            eps = torch.randn(self.loc.shape, generator=gen)
            draws.append(eps.numpy().copy())
            return self.loc + self.scale * eps

    M.Normal = RecNormal
    batches = []
    if sampling == "shuffle":   # record the minibatch indices of storage.mini_batch_generator_shuffle
        import omniisaacgymenvs.algo.ppo.storage as S

        class RecBatchSampler(S.BatchSampler):
            def __iter__(self):
                for b in super().__iter__():
                    batches.append(np.asarray(list(b), np.int32))
                    yield b

        S.BatchSampler = RecBatchSampler
    torch.manual_seed(seed)
    ob_dim, act_dim = 33, 2
    kw = dict(speed_dim=3, mass_dim=8, mass_latent_dim=8, mass_encoder_shape=(64, 16))
    actor = M.Actor(M.MLPEncode_wrap([128, 128], nn.LeakyReLU, ob_dim, act_dim, nn.Tanh, False, **kw),
                    M.SquashedGaussianDiagonalCovariance(act_dim, 0.3, action_scale=1.0), "cpu")
    critic = M.Critic(M.MLPEncode_wrap([128, 128], nn.LeakyReLU, ob_dim, 1, **kw), "cpu")
    fe = ScriptedExpert(torch) if expert else None
    ppo = P.PPO(actor=actor, critic=critic, num_envs=n, num_transitions_per_env=T, num_learning_epochs=4,
                gamma=0.997, lam=0.95, num_mini_batches=4, device="cpu", log_dir="/tmp/loopz_golden",
                mini_batch_sampling=sampling, learning_rate=5e-4, flat_expert=fe)
    if expert:
        ppo.update_rl_coeff(0.3)   # the trainer's value (rlgames_train.py:352-354)
    sd = lambda m: {k: v.detach().clone().numpy() for k, v in m.state_dict().items()}
    init = {"actor": sd(actor.architecture), "dist": sd(actor.distribution), "critic": sd(critic.architecture)}
    rng = np.random.default_rng(seed)
    obs = rng.uniform(-2.5, 2.5, (T + 1, n, ob_dim)).astype(np.float32)
    obs[..., 25:] = rng.uniform(-1, 1, (T + 1, n, 8)).astype(np.float32)
    rew = rng.normal(0.0, 1.0, (T, n)).astype(np.float32)
    done = rng.uniform(0, 1, (T, n)) < 0.06
    acts = []
    for t in range(T):
        acts.append(ppo.observe(obs[t]))
        ppo.step(value_obs=obs[t], rews=rew[t], dones=done[t], infos=[])
    losses = {}
    orig = ppo._train_step

    def train_step():
        mv, ms, inf = orig()
        losses["value"], losses["surrogate"] = mv, ms
        return mv, ms, inf

    ppo._train_step = train_step
    ppo.update(actor_obs=obs[T], value_obs=obs[T], log_this_iteration=False, update=0)
    st = ppo.storage
    after = {"actor": sd(actor.architecture), "dist": sd(actor.distribution), "critic": sd(critic.architecture)}
    opt = ppo.optimizer.state_dict()
    actor.distribution.enforce_minimum_std(torch.ones(act_dim) * 0.05)
    out = {"obs": obs, "rew": rew, "done": done.astype(np.uint8), "eps": np.stack(draws[:T]),
           "actions": np.stack(acts), "logp": st.actions_log_prob.numpy()[..., 0], "values": st.values.numpy()[..., 0],
           "returns": st.returns.numpy()[..., 0], "advantages": st.advantages.numpy()[..., 0],
           "loss_value": np.float64(losses["value"]), "loss_surrogate": np.float64(losses["surrogate"]),
           "std_enforced": actor.distribution.std.detach().numpy().copy(),
           "adam_step": np.float64(opt["state"][0]["step"])}
    for tag, d in (("init", init), ("after", after)):
        for net, sdict in d.items():
            for k, v in sdict.items():
                out[f"{tag}/{net}/{k}"] = v
    for i, s_ in opt["state"].items():
        out[f"adam_m_{i}"] = s_["exp_avg"].numpy()
        out[f"adam_v_{i}"] = s_["exp_avg_sq"].numpy()
    if sampling == "shuffle":
        out["batches"] = np.stack(batches)   # [epochs * mini_batches][M] rows of the flattened [T * N] storage
    if expert:   # the expert's actions on the stored observations (storage-row order) and its weights
        out["expert_act"] = fe.evaluate(st.actor_obs.reshape(-1, ob_dim)).numpy()
        out["expert_w"] = fe.w.numpy()
        out["rl_coeff"] = np.float64(ppo.rl_coeff)
    name = "loopz_update" + ("" if sampling == "in_order" else f"_{sampling}") + ("_expert" if expert else "")
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)


def gen_field(torch):
    from omniisaacgymenvs.tasks.USV.d_multi_gemini import BatchedMapGPU
    res = {}
    g = torch.Generator().manual_seed(11)
    for name, k in (("b1", 1), ("b4", 4)):
        obs = torch.rand((k, 16, 2), generator=g) * 24 - 12
        if k == 4:
            obs[1, 3] = torch.tensor([999.0, 999.0])      # limbo obstacle
            obs[2, :6] = torch.tensor([[0.4, 0.0], [1.4, 0.0], [2.4, 0.0], [-1.0, 1.0], [-1.0, -1.0], [0.0, -1.2]])
            obs[3] = torch.tensor([999.0, 999.0])          # empty map
        tgt = torch.zeros((k, 2))
        if k == 4:
            tgt[1] = torch.tensor([2.3, -4.1])
        m = BatchedMapGPU(k, 150, 30.0, 0.5, device="cpu")
        occ, sdf = m.compute_occupancy_and_sdf(obs)
        cost = m.compute_cost_field_wavefront(occ, tgt)
        pot = m.compute_potential_field(cost, sdf)
        # convergence check: one more Jacobi sweep must not change the field
        m2 = BatchedMapGPU(k, 150, 30.0, 0.5, device="cpu")
        res[f"{name}_obst"] = obs.numpy()
        res[f"{name}_tgt"] = tgt.numpy()
        res[f"{name}_cost"] = cost.numpy()
        res[f"{name}_field"] = pot.numpy()
        res["grid_lin"] = m.grid_coords[0, 0, :, 0].numpy().copy()
    np.savez_compressed(os.path.join(OUT, "field.npz"), **res)


def policy_actions(rng, n, t):
    """Deterministic, varied action sequences (forward runs, turns, idle)."""
    a = np.zeros((n, 2), np.float32)
    for e in range(n):
        mode = e % 4
        if mode == 0:
            a[e] = [1.0, 1.0]
        elif mode == 1:
            a[e] = [1.0, 0.2 + 0.6 * math.sin(0.2 * t + e)]
        elif mode == 2:
            a[e] = rng.uniform(-1, 1, 2)
        else:
            a[e] = [0.6 + 0.4 * math.cos(0.3 * t), 1.0]
    return a


def _task_targets(task):
    """(target xy [n,2], target heading / yaw rate [n]) of the task object."""
    if hasattr(task, "_target_linear_velocities"):   # TrackXYOVelocityTask
        return (task._target_linear_velocities.numpy().copy(), task._target_angular_velocities.numpy().copy())
    h = task._target_headings.numpy().copy() if hasattr(task, "_target_headings") else None
    return task._target_positions.numpy().copy(), h


def make_scene_file():
    """tests/golden/scenes_S.npz: 7 scenes in build_usv_scenes.py's format (own writer)."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
    from omniisaacgymenvs_loop_amd.tasks.scene_replay import write_scenes_npz
    rng = np.random.default_rng(2024)
    S, M = 7, 16
    counts = np.array([16, 0, 5, 16, 9, 3, 12], np.int32)
    obs = np.full((S, M, 2), np.nan, np.float32)
    goal = rng.uniform(-2, 2, (S, 2)).astype(np.float32)
    for i in range(S):
        obs[i, :counts[i]] = goal[i] + rng.uniform(-12, 12, (counts[i], 2)).astype(np.float32)
    r = rng.uniform(9, 12, S)
    th = rng.uniform(0, 2 * np.pi, S)
    start = np.stack([r * np.cos(th), r * np.sin(th)], 1).astype(np.float32)
    yaw = rng.uniform(0, np.pi, S).astype(np.float32)
    vel = rng.uniform(-1.5, 1.5, (S, 2)).astype(np.float32)
    write_scenes_npz(os.path.join(OUT, "scenes_S.npz"), obs, counts, start, yaw, vel, goal, seed=2024,
                     generator_cfg={"task_name": "golden", "num_episodes": S})


def gen_episode(torch, variant, n, steps, seed):
    torch.manual_seed(seed)
    usv, heron, world, task_cfg = build_usv(torch, n, variant)
    ve = make_vecenv(torch, usv, world)
    rec = RandRecorder(torch)
    trec = TrigRecorder(torch)
    rng = np.random.default_rng(seed)
    with rec, trec:
        usv.post_reset()
        init_draws = rec.take()
        usv.update_state()   # the cached root_* state of the first step (see module doc)
        rec.take()
        init_tgt = _task_targets(usv.task)[0]
        usv.task.reset(torch.arange(n))   # flags only (reset via VecEnv.reset below)
        rec.take()
        trec.take()
    data = {k: [] for k in ("actions", "obs", "rew", "reset", "progress", "px", "py", "yaw", "vx", "vy", "wz",
                            "fl", "fr", "reset_mask", "u_step", "mass", "com", "k_drag", "thr_l", "thr_r",
                            "k_iz", "obst", "tgt", "extras", "goal_cnt", "bias", "terms")}
    reset_U = []
    usv.task.just_had_been_reset = torch.arange(n)
    with rec, trec:
        for t in range(steps):
            reset_mask = usv.reset_buf.numpy().astype(bool).copy() if t > 0 else np.ones(n, bool)
            if t == 0:
                usv.reset()
                act = np.zeros((n, 2), np.float32)
            else:
                act = policy_actions(rng, n, t)
            bias_active = (usv._initial_action_bias_steps > 0 and
                           usv._action_bias_step_count < usv._initial_action_bias_steps)
            obs_dict, rew, resets, extras = ve.step(torch.from_numpy(act))
            draws = rec.take()
            reset_draws = [d for d in draws if d[0] not in ("add_noise_on_vel", "add_noise_on_heading",
                                                             "add_noise_on_pos", "add_noise_on_act")]
            Us, _ = map_step_draws(draws, n)
            k = int(reset_mask.sum())
            trig = trec.take()
            if k:
                Ur = map_reset_draws(reset_draws, k)
                Ur[:, RU["TRIG"]:RU["TRIG"] + 6] = map_reset_trig(trig, k)
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
            for key, val in (("px", heron.px), ("py", heron.py), ("yaw", heron.yaw), ("vx", heron.vx),
                             ("vy", heron.vy), ("wz", heron.wz)):
                data[key].append(val.numpy().copy())
            cf = usv.thrusters_dynamics.current_forces.numpy().copy()
            data["fl"].append(cf[:, 0])
            data["fr"].append(cf[:, 1])
            data["mass"].append(usv.MDD.platforms_mass[:, 0].numpy().copy())
            data["com"].append(usv.MDD.platforms_CoM.numpy().copy())
            data["k_drag"].append(usv.hydrodynamics.drag_scale[:, 0].numpy().copy())
            td = usv.thrusters_dynamics
            if td._use_separate_randomization:
                data["thr_l"].append(td.thruster_left_multiplier[:, 0].numpy().copy())
                data["thr_r"].append(td.thruster_right_multiplier[:, 0].numpy().copy())
            else:
                data["thr_l"].append(td.thruster_multiplier[:, 0].numpy().copy())
                data["thr_r"].append(td.thruster_multiplier[:, 0].numpy().copy())
            data["k_iz"].append(usv.k_Iz[:, 0].numpy().copy())
            if variant in ("P", "T", "Q"):
                data["obst"].append(np.zeros((n, 16, 2), np.float32))
                data.setdefault("tgt_h", []).append(_task_targets(usv.task)[1])
            else:
                data["obst"].append(usv.task.xunlian_pos[:, :, :2].numpy().copy())
            data["tgt"].append(_task_targets(usv.task)[0])
            data["goal_cnt"].append(usv.task._goal_reached.numpy().copy())
            tk = usv.task
            pen = usv._penalties
            if variant in ("P", "T", "Q"):
                data["terms"].append(np.zeros((n, 15), np.float32))
            else:
              data["terms"].append(torch.stack([tk.distance_reward, tk.alignment_reward, tk.potential_shaping_reward,
                                           tk._turn_hazard_penalty, tk._speed_reward, tk._angular_reward,
                                           tk._heading_improve_reward, tk.collision_reward, tk._goal_reward,
                                           tk._total_reward, pen.angular_vel_penalty,
                                           pen.angular_vel_variation_penalty, pen.energy_penalty,
                                           tk._danger_factor, tk.prev_potential], 1).numpy().astype(np.float32))
            if variant == "S":
                data.setdefault("scene_last", []).append(usv.scene_replay_last_scene_idx.numpy().copy())
            if variant == "C":
                uf, td_ = usv.UF, usv.TD
                data.setdefault("dist", []).append(torch.stack([
                    uf.disturbance_forces_const[:, 0], uf.disturbance_forces_const[:, 1], uf._force_x_freq,
                    uf._force_y_freq, uf._force_x_shift, uf._force_y_shift, uf._force_amp,
                    td_.disturbance_torques_const[:, 2], td_._torque_freq, td_._torque_shift, td_._torque_amp],
                    0).numpy().copy())
            ex = extras.get("episode", {})
            names = STAT_NAMES if variant not in ("P", "T", "Q") else list(usv.episode_sums.keys())
            data["extras"].append(np.array([float(ex[k]) if k in ex else np.nan for k in names], np.float32))
    out = {k: np.stack(v) for k, v in data.items()}
    out["reset_U"] = np.concatenate(reset_U, 0) if reset_U else np.zeros((0, NU_RESET), np.float32)
    out["init_tgt"] = init_tgt
    out["grid_lin"] = (usv.task.gpu_map.grid_coords[0, 0, :, 0].numpy().copy() if hasattr(usv.task, "gpu_map")
                       else np.zeros(150, np.float32))
    out["config_json"] = np.frombuffer(json.dumps(task_cfg).encode(), dtype=np.uint8)
    out["bias_steps"] = np.int64(usv._initial_action_bias_steps)
    if variant in ("P", "T", "Q"):
        out["extras_names"] = np.array(list(usv.episode_sums.keys()))
    np.savez_compressed(os.path.join(OUT, f"episode_{variant}.npz"), **out)
    print(f"episode_{variant}: resets per step", out["reset_mask"].sum(1).tolist())


class ScriptedVecEnv:
    """Plays back fixed obs/rewards/dones; exposes what A2CBase.__init__ touches."""

    def __init__(self, torch, n, horizon, seed):
        g = torch.Generator().manual_seed(seed)
        self.t = torch
        self.n = n
        self.obs = [torch.randn((n, 33), generator=g) * 2.0 for _ in range(horizon + 1)]
        self.rew = [torch.randn((n,), generator=g) * 3.0 for _ in range(horizon)]
        self.dones = [(torch.rand((n,), generator=g) < 0.08).long() for _ in range(horizon)]
        self.k = 0
        self.actions_seen = []
        self.env = types.SimpleNamespace(_world=types.SimpleNamespace(step=lambda render=False: None),
                                         _task=types.SimpleNamespace(update_state=lambda: None))

    def reset(self):
        self.k = 0
        return {"obs": {"state": self.obs[0].clone()}, "states": self.t.zeros((self.n, 0))}

    def step(self, actions):
        self.actions_seen.append(actions.clone())
        k = self.k
        self.k += 1
        return ({"obs": {"state": self.obs[k + 1].clone()}, "states": self.t.zeros((self.n, 0))},
                self.rew[k].clone(), self.dones[k].clone(), {})

    def set_train_info(self, *a, **k):
        pass

    def get_env_state(self):
        return None


def gen_ppo(torch, n=32, horizon=16, minibatch=128, seed=5):
    import yaml
    from rl_games.algos_torch import a2c_continuous
    from rl_games.common.algo_observer import DefaultAlgoObserver
    from rl_games.common import tr_helpers
    with open(os.path.join(REF, "omniisaacgymenvs/cfg/train/USV/USV_PPOcontinuous_MLP.yaml")) as f:
        params = yaml.safe_load(f)["params"]
    cfg = params["config"]
    cfg.update(dict(name="golden", full_experiment_name="golden", device="cpu", device_name="cpu", num_actors=n,
                    minibatch_size=minibatch, max_epochs=10, train_dir="/tmp/golden_runs", print_stats=False))
    cfg["reward_shaper"] = tr_helpers.DefaultRewardsShaper(**cfg["reward_shaper"])
    cfg["features"] = {"observer": DefaultAlgoObserver()}
    spaces = sys.modules["gym.spaces"]
    env_info = {"action_space": spaces.Box(np.array([-1.0, -1.0], np.float32), np.array([1.0, 1.0], np.float32)),
                "observation_space": spaces.Dict({"state": spaces.Box(np.ones(33) * -np.inf, np.ones(33) * np.inf)})}
    env_info["observation_space"].spaces["state"].shape = (33,)
    cfg["env_info"] = env_info
    venv = ScriptedVecEnv(torch, n, horizon, seed)
    cfg["vec_env"] = venv
    params["seed"] = seed
    torch.manual_seed(seed)
    agent = a2c_continuous.A2CAgent("run", params)
    init_state = {k: v.detach().clone().numpy() for k, v in agent.model.state_dict().items()}
    agent.init_tensors()
    agent.obs = agent.env_reset()
    torch.manual_seed(seed + 1)
    recorded = {"losses": [], "kl": [], "lr": [], "mu_after": []}
    orig_train_ac = agent.train_actor_critic

    def train_ac(input_dict):
        res = orig_train_ac(input_dict)
        a_loss, c_loss, entropy, kl, last_lr, lr_mul, cmu, csigma, b_loss = res
        recorded["losses"].append([float(a_loss), float(c_loss), float(entropy), float(b_loss)])
        recorded["kl"].append(float(kl))
        return res

    agent.train_actor_critic = train_ac
    orig_update_lr = agent.update_lr

    def update_lr(lr):
        recorded["lr"].append(float(lr))
        return orig_update_lr(lr)

    agent.update_lr = update_lr
    exp_snap = {}
    orig_prepare = agent.prepare_dataset

    def prepare(batch_dict):
        for k, v in batch_dict.items():
            if hasattr(v, "numpy"):
                exp_snap["batch_" + k] = v.detach().clone().numpy()
        orig_prepare(batch_dict)
        for k, v in agent.dataset.values_dict.items():
            if hasattr(v, "numpy"):
                exp_snap["ds_" + k] = v.detach().clone().numpy()
            elif isinstance(v, dict):
                for kk, vv in v.items():
                    exp_snap[f"ds_{k}_{kk}"] = vv.detach().clone().numpy()

    agent.prepare_dataset = prepare
    agent.train_epoch()
    out = {f"init_{k.replace('.', '__')}": v for k, v in init_state.items()}
    out.update({f"final_{k.replace('.', '__')}": v.detach().clone().numpy() for k, v in agent.model.state_dict().items()})
    eb = agent.experience_buffer.tensor_dict
    for k in ("actions", "neglogpacs", "values", "mus", "sigmas", "dones", "rewards"):
        out["exp_" + k] = eb[k].detach().clone().numpy()
    out["exp_obses"] = eb["obses"]["state"].detach().clone().numpy() if isinstance(eb["obses"], dict) else \
        eb["obses"].detach().clone().numpy()
    out["env_obs"] = np.stack([o.numpy() for o in venv.obs])
    out["env_rew"] = np.stack([r.numpy() for r in venv.rew])
    out["env_dones"] = np.stack([d.numpy() for d in venv.dones])
    out["env_actions"] = np.stack([a.numpy() for a in venv.actions_seen])
    out.update(exp_snap)
    out["losses"] = np.asarray(recorded["losses"], np.float64)
    out["kl"] = np.asarray(recorded["kl"], np.float64)
    out["lr_seq"] = np.asarray(recorded["lr"], np.float64)
    opt = agent.optimizer.state_dict()
    for i in range(9):
        out[f"adam_m_{i}"] = opt["state"][i]["exp_avg"].numpy()
        out[f"adam_v_{i}"] = opt["state"][i]["exp_avg_sq"].numpy()
        out[f"adam_step_{i}"] = np.float64(opt["state"][i]["step"])
    out["hyper"] = np.array([n, horizon, minibatch, agent.mini_epochs_num], np.int64)
    out["game_rewards_mean"] = agent.game_rewards.get_mean()
    out["game_rewards_size"] = np.int64(agent.game_rewards.current_size)
    np.savez_compressed(os.path.join(OUT, "ppo_epoch.npz"), **out)
    print("ppo: lr", recorded["lr"][:6], "... kl", recorded["kl"][:4])


CKPT811 = os.path.join(REF, "811_3.5刹车_____（复件）", "last_USV_ep_5450_rew_38.54975.pth")


def gen_ckpt811(torch, rows=64, seed=8):
    """The reference's only checkpoint (rl_games, 13-input network of the Aug-11 task): its
    state_dict tensors and metadata, and the reference ModelA2CContinuousLogStd (built from the USV
    train yaml's network section, normalize_input / normalize_value as trained) evaluated on fixed
    13-dim observations: mus, sigmas, denormalised values, the sampled actions and their neglogp."""
    import codecs
    import yaml
    from rl_games.algos_torch import model_builder
    torch.serialization.add_safe_globals([(np._core.multiarray.scalar, "numpy.core.multiarray.scalar"), np.dtype,
                                          codecs.encode, np.dtypes.Float64DType, np.dtypes.Float32DType])
    ck = torch.load(CKPT811, weights_only=True, map_location="cpu")
    with open(os.path.join(REF, "omniisaacgymenvs/cfg/train/USV/USV_PPOcontinuous_MLP.yaml")) as f:
        params = yaml.safe_load(f)["params"]
    net = model_builder.ModelBuilder().load(params).build(
        {"actions_num": 2, "input_shape": {"state": (13,)}, "num_seqs": 1, "value_size": 1,
         "normalize_value": True, "normalize_input": True, "normalize_input_keys": ["state"]})
    net.load_state_dict(ck["model"])
    net.eval()
    g = torch.Generator().manual_seed(seed)
    obs = (torch.randn(rows, 13, generator=g) * 2.0).float()
    torch.manual_seed(seed)
    with torch.no_grad():
        res = net({"is_train": False, "obs": {"state": obs.clone()}, "prev_actions": None})
    out = {"obs": obs.numpy(), "mus": res["mus"].numpy(), "sigmas": res["sigmas"].numpy(),
           "values": res["values"].numpy(), "actions": res["actions"].numpy(),
           "neglogpacs": res["neglogpacs"].numpy(), "epoch": np.int64(ck["epoch"]), "frame": np.int64(ck["frame"]),
           "last_mean_rewards": np.float32(ck["last_mean_rewards"]),
           "opt_lr": np.float64(ck["optimizer"]["param_groups"][0]["lr"]),
           "opt_step": np.float64(ck["optimizer"]["state"][0]["step"]),
           "keys": np.array(list(ck["model"].keys())), "top_keys": np.array(list(ck.keys()))}
    for k, v in ck["model"].items():
        out["sd__" + k] = v.numpy()
    for i, st in ck["optimizer"]["state"].items():
        out[f"opt_m_{i}"] = st["exp_avg"].numpy()
        out[f"opt_v_{i}"] = st["exp_avg_sq"].numpy()
    np.savez_compressed(os.path.join(OUT, "ckpt811.npz"), **out)
    print("ckpt811: mus[0]", out["mus"][0], "values[0]", out["values"][0])


def gen_ref_cfg():
    """ref_cfg_resolved.json: what the reference's own train / TEST task yamls (unmodified) compose and resolve
    to under the overrides tests/test_hydra_cfg_cpu.py uses -- the train params and the task dict.  The scene
    replay's NPZ path (a file on the author's machine) is left out; no root key of config.yaml is recorded."""
    import json
    sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
    from omniisaacgymenvs_loop_amd.scripts.rlgames_train import build_config
    ref = build_config({"cfg_dir": os.path.join(REF, "omniisaacgymenvs", "cfg"), **REF_CFG_OVERRIDES})
    ref["task"]["env"]["scene_replay"].pop("npz_path", None)
    out = {"overrides": REF_CFG_OVERRIDES, "task_name": ref["task_name"], "train_params": ref["train"]["params"],
           "task": ref["task"]}
    with open(os.path.join(OUT, "ref_cfg_resolved.json"), "w", encoding="utf-8") as f:
        json.dump(out, f, indent=1, sort_keys=True, ensure_ascii=True)
        f.write("\n")


REF_CFG_OVERRIDES = {"num_envs": 1024, "seed": 7, "max_iterations": 11}

STAT_NAMES = [
    "total_reward", "distance_reward", "alignment_reward", "heading_improve_reward",
    "potential_shaping_reward", "speed_reward", "angular_reward", "turn_hazard_penalty",
    "goal_reward", "collision_reward", "time_reward", "success", "collision",
    "position_error", "boundary_penalty", "danger_mean", "danger_hi_rate", "g_gate_mean",
    "g_safe_mean", "angular_vel_penalty", "angular_vel_variation_penalty", "energy_penalty",
    "normed_linear_vel", "normed_angular_vel", "cmd_neg_rate", "u_mean", "u_low_rate", "u_sum",
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    install_stubs()
    import torch
    torch.set_num_threads(8)
    jobs = {
        "lut": lambda: gen_lut(torch),
        "forces": lambda: gen_forces(torch),
        "hydrostatics": lambda: gen_hydrostatics(torch),
        "field": lambda: gen_field(torch),
        "episodeA": lambda: gen_episode(torch, "A", 16, 64, 1234),
        "episodeB": lambda: gen_episode(torch, "B", 12, 56, 99),
        "episodeC": lambda: gen_episode(torch, "C", 12, 64, 77),
        "episodeD": lambda: gen_episode(torch, "D", 10, 48, 55),
        "episodeE": lambda: gen_episode(torch, "E", 10, 48, 56),
        "episodeP": lambda: gen_episode(torch, "P", 12, 64, 31),
        "episodeQ": lambda: gen_episode(torch, "Q", 12, 64, 33),
        "episodeS": lambda: (make_scene_file(), gen_episode(torch, "S", 6, 64, 41)),
        "episodeT": lambda: gen_episode(torch, "T", 12, 64, 32),
        "ppo": lambda: gen_ppo(torch),
        "loopz": lambda: gen_loopz(torch),
        "loopz_shuffle": lambda: gen_loopz(torch, sampling="shuffle"),
        "loopz_expert": lambda: gen_loopz(torch, expert=True),
        "ckpt811": lambda: gen_ckpt811(torch),
        "ref_cfg": gen_ref_cfg,
    }
    for name, fn in jobs.items():
        if args.only and name not in args.only.split(","):
            continue
        print("generating", name)
        fn()


if __name__ == "__main__":
    main()
