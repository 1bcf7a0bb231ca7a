"""Generate tests/golden/compare_golden.npz: the privileged-tail overrides of the REFERENCE's compare tool
(omniisaacgymenvs/scripts/rlgames_play_loopz_compare.py) on stand-in task objects.

Run only where the reference tree exists (make_golden.REF):
    python tests/golden/make_compare_golden.py

The reference's _compute_base_const_all_tail, _compute_wrong_random_tail and _override_obs_priv_tail are IMPORTED
and called.  The stand-in task is a SimpleNamespace holding the attributes those functions read, with the
reference's own USVVirtual._encode_centered_priv_param / _encode_minmax_priv_param and
MassDistributionDisturbances.get_base_masses bound to it.  Cases: every privileged_params_mode x coupling on / off
x mass raw / relative x CoM raw / scaled at priv_dim 8, plus priv_dim 4, no CoM displacement and reversed mass
bounds; SEEDS generator seeds each.  The uniforms the tool's generator drew are recorded from a twin
default_rng(seed) (Generator.uniform(lo, hi) is lo + (hi - lo) * next_double).  The fixture holds arrays only."""
from __future__ import annotations

import itertools
import os
import sys
import types
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_golden import install_stubs  # noqa: E402

from tests import compare_restate as CR  # noqa: E402

SEEDS = (0, 1, 12345)


def load_reference():
    install_stubs()
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = type("SummaryWriter", (), {"__init__": lambda self, *a, **k: None})
    sys.modules["torch.utils.tensorboard"] = tb
    import omniisaacgymenvs.scripts.rlgames_play_loopz_compare as C
    from omniisaacgymenvs.tasks.USV.USV_disturbances import MassDistributionDisturbances
    from omniisaacgymenvs.tasks.USV_Virtual import USVVirtual
    return C, USVVirtual, MassDistributionDisturbances


def stand_in(torch, USVVirtual, MDD, p):
    """The task object the compare tool reads, from a case dict (tests/compare_restate.case_params)."""
    mdd = SimpleNamespace(_num_envs=1, _device="cpu", _min_mass=p["min_mass"], _max_mass=p["max_mass"],
                          _base_mass=p["base_mass"], _base_com=torch.tensor(p["base_com"], dtype=torch.float32),
                          _com_displacement_xyz=list(p["com_disp"]) if p["com_mode"] == 1 else None,
                          _CoM_max_displacement=0.0)
    mdd.get_base_masses = types.MethodType(MDD.get_base_masses, mdd)
    task = SimpleNamespace(
        MDD=mdd, _device="cpu", _mass_obs_mode="relative" if p["mass_relative"] else "raw",
        _com_obs_mode="scaled" if p["com_scaled"] else "raw", _com_obs_scale=tuple(p["com_scale"]),
        _privileged_params_mode=p["priv_mode"], _privileged_params_nominal=p["nominal"],
        _k_drag_min=p["k_drag_min"], _k_drag_max=p["k_drag_max"], _thruster_rand_for_priv=p["thr_rand"],
        _k_iz_min=p["k_iz_min"], _k_iz_max=p["k_iz_max"], _mass_driven_couple_drag=p["couple_drag"],
        _mass_driven_couple_thruster=p["couple_thr"], _mass_driven_couple_yaw_inertia=p["couple_kiz"])
    task._encode_centered_priv_param = types.MethodType(USVVirtual._encode_centered_priv_param, task)
    task._encode_minmax_priv_param = types.MethodType(USVVirtual._encode_minmax_priv_param, task)
    return task


def main():
    C, USVVirtual, MDD = load_reference()
    import torch
    cases = CR.all_cases()
    out = {"case_values": np.stack([CR.case_to_row(p) for p in cases]), "seeds": np.asarray(SEEDS, np.int64)}
    const_tails, wrong_tails, draws = [], [], []
    for p in cases:
        task = stand_in(torch, USVVirtual, MDD, p)
        md = int(p["priv_dim"])
        t = C._compute_base_const_all_tail(task, env_id=0, mass_dim=md)
        assert t is not None and t.shape == (md,) and t.dtype == np.float32
        const_tails.append(np.pad(t, (0, 8 - md)))
        wt, dr = [], []
        for seed in SEEDS:
            tail, _audit = C._compute_wrong_random_tail(task, env_id=0, mass_dim=md, rng=np.random.default_rng(seed))
            assert tail is not None and tail.shape == (md,) and tail.dtype == np.float32
            twin = np.random.default_rng(seed)
            u = [twin.random()] + (list(twin.random(3)) if p["com_mode"] == 1 else [0.0, 0.0, 0.0])
            wt.append(np.pad(tail, (0, 8 - md)))
            dr.append(u)
        wrong_tails.append(np.stack(wt))
        draws.append(np.asarray(dr, np.float64))
    out["const_tail"] = np.stack(const_tails).astype(np.float32)      # [case][8] (priv_dim 4: zero padded)
    out["wrong_tail"] = np.stack(wrong_tails).astype(np.float32)      # [case][seed][8]
    out["wrong_draws"] = np.stack(draws)                              # [case][seed][4] uniforms in [0, 1)
    g = np.random.default_rng(5)
    obs = g.standard_normal((5, 33)).astype(np.float32)
    out["override_obs_in"] = obs.copy()
    out["override_obs_out8"] = C._override_obs_priv_tail(obs.copy(), tail_1d=out["const_tail"][0], mass_dim=8)
    out["override_obs_out4"] = C._override_obs_priv_tail(obs.copy(), tail_1d=out["const_tail"][0][:4], mass_dim=4)
    path = os.path.join(HERE, "compare_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(cases)} cases x {len(SEEDS)} seeds, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
