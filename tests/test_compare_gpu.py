"""The teacher-vs-student comparison on the device: sysid_play (csrc/usv_sysid.hip) against the torch restatement
and the reference's fixture, usv_priv_tail and usv_cmp_fold (csrc/usv_compare.hip) against their host restatements,
and scenario.compare / scripts.compare_policies end to end."""
import csv
import json
import os

import numpy as np
import pytest
import torch

from tests import compare_restate as CR
from tests import errtab
from tests import sysid_restate as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE20 = os.path.join(ROOT, "tests", "golden", "scenario_pre20.npz")
TASK_YAML = os.path.join(ROOT, "omniisaacgymenvs_loop_amd", "cfg", "task", "USV", "IROS2024",
                         "USV_Virtual_CaptureXY_SysID-TEST.yaml")
DEV = "cuda:0"
TOL = 1e-5
KERNELS = ("default", "scalar")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------ sysid_play
def make_agent(teacher_sd, enc_sd, obs_dim=33):
    from tests.test_sysid_gpu import make_agent as mk
    return mk(teacher_sd, enc_sd, obs_dim)


def play(obs, teacher_sd, enc_sd, mode="zeros", kernel="default", zero_latent=False):
    """The student as a policy fed a recorded stream (dones reach the history as in the reference's loop): per-step
    zhat and actions of sysid_play."""
    from omniisaacgymenvs_loop_amd.sysid import HistoryStream
    obs, dones = obs
    S, n, obs_dim = len(dones), obs.shape[1], obs.shape[2]
    agent = make_agent(teacher_sd, enc_sd, obs_dim)
    hs = HistoryStream(n, obs_dim, horizon=1, fill_history_on_reset=mode, device=DEV)
    zhat = torch.full((n, 8), 7.0, device=DEV)
    actions = torch.zeros((n, 2), device=DEV)
    o_dev, d_dev = torch.tensor(obs, device=DEV), torch.tensor(dones, device=DEV)
    out = {"zhat": [], "actions": []}
    hs.reset()
    hs.append(o_dev[0], None)
    for k in range(S):
        agent.play_step(hs, zhat, actions, zero_latent=zero_latent, scalar=kernel == "scalar")
        out["zhat"].append(zhat.cpu().numpy())
        out["actions"].append(actions.cpu().numpy())
        if k + 1 < S:
            hs.append(o_dev[k + 1], d_dev[k])
    return {q: np.stack(v) for q, v in out.items()}


_WANT = {}


def restated(n, obs_dim, steps, mode):
    """R.run's forward of one stream, computed once and shared."""
    key = (n, obs_dim, steps, mode)
    if key not in _WANT:
        obs, dones = R.make_stream(n, steps, obs_dim, seed=100 + n)
        t, e = R.random_teacher(obs_dim - 8, 31), R.random_enc(obs_dim - 8, 32)
        _WANT[key] = ((obs, dones), t, e, R.run(obs, dones, t, e, mode=mode, horizon=10 ** 6))
    return _WANT[key]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,obs_dim", [(1, 33), (70, 33), (70, 36)])
def test_play_vs_restatement(n, obs_dim, kernel):
    """60 steps, so the windows fill and wrap the ring (horizon 1: the ring is 50 frames), both fill modes; 70 envs
    are a multiple of neither 8, 16 nor 32."""
    for mode in ("zeros", "repeat"):
        stream, t, e, want = restated(n, obs_dim, 60, mode)
        got = play(stream, t, e, mode=mode, kernel=kernel)
        for q in ("zhat", "actions"):
            errtab.check(f"sysid_play[{kernel},n={n},obs={obs_dim},{mode}]", q, got[q], want[q], TOL, TOL)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("mode", ["zeros", "repeat"])
def test_play_vs_reference(golden, mode, kernel):
    fx = golden("sysid_golden.npz")
    t = R.unflatten(fx["teacher"], R.TEACHER_KEYS, R.teacher_shapes(25))
    e = R.unflatten(fx["enc0"], R.ENC_KEYS, R.enc_shapes(25))
    H = 16   # the fixture's encoder is updated after 16 steps: its first 16 steps ran enc0
    got = play((fx["obs"][:H + 1], fx["dones"][:H]), t, e, mode=mode, kernel=kernel)
    for q in ("zhat", "actions"):
        errtab.check(f"sysid_play_fixture[{kernel},{mode}]", q, got[q], fx[f"{mode}_{q}"][:H], TOL, TOL)


@pytest.mark.parametrize("kernel", KERNELS)
def test_play_many_tiles(kernel):
    """4,160 envs, 4 steps: more tiles than a capped grid would hold in one wave of workgroups."""
    stream, t, e, want = restated(4160, 33, 4, "repeat")
    got = play(stream, t, e, mode="repeat", kernel=kernel)
    for q in ("zhat", "actions"):
        errtab.check(f"sysid_play_tiles[{kernel}]", q, got[q], want[q], TOL, TOL)


def test_play_zero_latent():
    """zhat == 0 exactly, the actions are the action head of [cur | 0], and the two kernels agree."""
    n, obs_dim = 70, 36
    stream, t, e, _ = restated(n, obs_dim, 60, "zeros")
    obs = stream[0]
    got = {k: play((obs[:5], stream[1][:4]), t, e, kernel=k, zero_latent=True) for k in KERNELS}
    D = obs_dim - 8
    x = torch.tensor(np.nan_to_num(obs[:4, :, :D]))
    x = torch.cat([x, torch.zeros(4, n, 8)], -1)
    lk = torch.nn.functional.leaky_relu
    h = lk(x @ t["architecture.action_mlp.0.weight"].T + t["architecture.action_mlp.0.bias"])
    h = lk(h @ t["architecture.action_mlp.2.weight"].T + t["architecture.action_mlp.2.bias"])
    want = torch.tanh(h @ t["architecture.action_mlp.4.weight"].T + t["architecture.action_mlp.4.bias"]).numpy()
    for k in KERNELS:
        assert not got[k]["zhat"].any()
        errtab.check(f"sysid_play_zero_latent[{k}]", "actions", got[k]["actions"], want, TOL, TOL)
    assert np.array_equal(bits(got["default"]["actions"]), bits(got["scalar"]["actions"]))


def test_play_checks_its_arguments():
    from omniisaacgymenvs_loop_amd import _capi
    from omniisaacgymenvs_loop_amd.sysid import HistoryStream
    stream, t, e, _ = restated(1, 33, 60, "zeros")
    agent = make_agent(t, e, 33)
    hs = HistoryStream(1, 33, horizon=1, device=DEV)
    z, a = torch.zeros((1, 8), device=DEV), torch.zeros((1, 2), device=DEV)
    args = lambda flags, hist=50: (_capi.ptr(agent.enc_flat), _capi.ptr(agent.teacher_flat), 1, 33, hist, 1, 0, 0,  # noqa: E731
                                   flags, _capi.ptr(hs.stream), _capi.ptr(hs.valid_rows), _capi.ptr(z), _capi.ptr(a),
                                   _capi.stream_ptr())
    assert _capi.call_rc("sysid_play", *args(0)) == 0
    assert _capi.call_rc("sysid_play", *args(4)) == 1
    assert _capi.call_rc("sysid_play", *args(0, hist=40)) == 2


# --------------------------------------------------------------------------------------------- usv_priv_tail
def cfg_of_case(p):
    from omniisaacgymenvs_loop_amd.tasks.usv_config import build_usv_cfg, load_yaml
    c = build_usv_cfg(load_yaml(TASK_YAML))
    c.priv_dim, c.priv_mode, c.priv_nominal = p["priv_dim"], CR.PRIV_MODES.index(p["priv_mode"]), p["nominal"]
    c.mass_relative, c.com_scaled, c.com_mode, c.com_legacy_r = p["mass_relative"], p["com_scaled"], p["com_mode"], \
        p["com_legacy_r"]
    for i in range(3):
        c.com_scale[i], c.base_com[i], c.com_disp[i] = p["com_scale"][i], p["base_com"][i], p["com_disp"][i]
    c.mass_min, c.mass_max, c.base_mass = p["min_mass"], p["max_mass"], p["base_mass"]
    c.couple_drag, c.couple_thr, c.couple_kiz = p["couple_drag"], p["couple_thr"], p["couple_kiz"]
    c.kdrag_min, c.kdrag_max, c.kiz_min, c.kiz_max = p["k_drag_min"], p["k_drag_max"], p["k_iz_min"], p["k_iz_max"]
    c.thr_rand = p["thr_rand"]
    c.thr_min = 1.0 - p["thr_rand"]
    c.thr_max = 1.0 if p["couple_thr"] else 1.0 + p["thr_rand"]
    return c


def priv_tail(cfg, mode, obs, const_tail=None, episode=None, seed=0, in_place=False):
    from omniisaacgymenvs_loop_amd import _capi
    n, obs_dim = obs.shape
    out = obs if in_place else torch.full_like(obs, -9.0)
    rc = _capi.call_rc("usv_priv_tail", _capi.byref(cfg), mode, _capi.ptr(obs), _capi.ptr(out), n, obs_dim,
                       _capi.ptr(const_tail), _capi.ptr(episode), seed, _capi.stream_ptr())
    return rc, out


@pytest.mark.parametrize("n", [1, 70])
def test_priv_tail_equals_the_host_restatement(n):
    """Every case of the CPU fixture (each privileged_params_mode, coupling, mass and CoM encoding, priv_dim 4, no CoM
    displacement): the head is bit-unchanged, the tail is the host restatement's bits from the same Philox words,
    out of place and in place; constant within an episode, different in the next."""
    from omniisaacgymenvs_loop_amd.scenario import compare as C
    seed = 0x1234567890ABCDEF
    for ci, p in enumerate(CR.all_cases()):
        cfg = cfg_of_case(p)
        md, obs_dim = p["priv_dim"], 25 + p["priv_dim"]
        g = torch.Generator().manual_seed(ci)
        obs = torch.randn((n, obs_dim), generator=g).to(DEV)
        params = C.tail_params(cfg)
        # base_const_all
        const = C.base_const_tail_host(params)
        rc, out = priv_tail(cfg, C.PT_CONST, obs, const_tail=torch.from_numpy(const).to(DEV))
        assert rc == 0
        o = out.cpu().numpy()
        assert np.array_equal(bits(o[:, :-md]), bits(obs.cpu().numpy()[:, :-md]))
        assert np.array_equal(bits(o[:, -md:]), bits(np.broadcast_to(const, (n, md)))), (ci, p)
        # wrong_random
        ep = (torch.arange(n, dtype=torch.int32) % 3).to(DEV)
        rc, out = priv_tail(cfg, C.PT_WRONG_RANDOM, obs, episode=ep, seed=seed)
        assert rc == 0
        u = C.wrong_random_words(seed, n, ep.cpu().numpy())
        want = C.wrong_random_tail_host(params, u[:, 0], u[:, 1:4])
        o = out.cpu().numpy()
        assert np.array_equal(bits(o[:, :-md]), bits(obs.cpu().numpy()[:, :-md]))
        assert np.array_equal(bits(o[:, -md:]), bits(want)), (ci, p, o[:, -md:], want)
        obs2 = torch.randn((n, obs_dim), generator=g).to(DEV)      # a later step of the same episodes
        keep = obs2.clone()
        rc, out2 = priv_tail(cfg, C.PT_WRONG_RANDOM, obs2, episode=ep, seed=seed, in_place=True)
        assert rc == 0 and out2 is obs2
        assert np.array_equal(bits(obs2.cpu().numpy()[:, -md:]), bits(want))
        assert np.array_equal(bits(obs2.cpu().numpy()[:, :-md]), bits(keep.cpu().numpy()[:, :-md]))
        rc, out3 = priv_tail(cfg, C.PT_WRONG_RANDOM, obs, episode=ep + 1, seed=seed)
        assert rc == 0 and (out3.cpu().numpy()[:, -md] != want[:, 0]).all()
        rc, out4 = priv_tail(cfg, C.PT_WRONG_RANDOM, obs, episode=None, seed=seed)   # NULL = episode 0
        u0 = C.wrong_random_words(seed, n, np.zeros(n, np.int32))
        assert rc == 0 and np.array_equal(bits(out4.cpu().numpy()[:, -md:]),
                                          bits(C.wrong_random_tail_host(params, u0[:, 0], u0[:, 1:4])))


def test_priv_tail_matches_the_task_encodings_and_refuses_the_legacy_mode():
    from omniisaacgymenvs_loop_amd.scenario import compare as C
    p = CR.case_params("centered", True, True, True)
    cfg = cfg_of_case(p)
    obs = torch.zeros((4, 33), device=DEV)
    cfg.com_mode, cfg.com_legacy_r = 2, 0.1
    assert priv_tail(cfg, C.PT_WRONG_RANDOM, obs)[0] == 2
    assert priv_tail(cfg, C.PT_CONST, obs, const_tail=torch.zeros(8, device=DEV))[0] == 0   # needs no draw
    cfg.com_legacy_r = 0.0
    assert priv_tail(cfg, C.PT_WRONG_RANDOM, obs)[0] == 0
    assert priv_tail(cfg, 3, obs)[0] == 1 and priv_tail(cfg, C.PT_CONST, obs)[0] == 1
    cfg.priv_dim = 6
    assert priv_tail(cfg, C.PT_WRONG_RANDOM, obs)[0] == 2


# ---------------------------------------------------------------------------------------------- usv_cmp_fold
def _ev_of(tab, cnt, K):
    from omniisaacgymenvs_loop_amd import _capi
    from omniisaacgymenvs_loop_amd._abi import UsvEval
    t, c = torch.tensor(tab, device=DEV), torch.tensor(cnt, device=DEV)
    ev = UsvEval()
    ev.acc, ev.episodes, ev.ep_count = None, _capi.ptr(t), _capi.ptr(c)
    ev.max_episodes, ev.action_scale, ev.control_dt = K, 1.0, 0.2
    return ev, (t, c)


@pytest.mark.parametrize("S,R,K,n,missing", [(3, 2, 1, 8, ()), (5, 3, 2, 8, (7,))])
def test_cmp_fold_equals_the_numpy_restatement(S, R, K, n, missing):
    from omniisaacgymenvs_loop_amd._abi import DEFINES as D
    from omniisaacgymenvs_loop_amd.scenario import compare as C
    (ta, ca), (tb, cb) = CR.hand_tables(S, R, K, n, missing_in_b=missing)
    thr = 1.2
    want = CR.cmp_fold_host(ta, ca, tb, cb, n, S, R, K, thr)
    (ea, keep_a), (eb, keep_b) = _ev_of(ta, ca, K), _ev_of(tb, cb, K)
    got = C.cmp_fold_device(ea, eb, n, S, R, K, thr, DEV)
    assert got.shape == (D["USV_CMP_ROWS"], S)
    for k in C.CMP_INT_KEYS:
        assert np.array_equal(got[D[C.CMP_KEYS[k]]], want[D[C.CMP_KEYS[k]]]), k
    for k in ("d_steps", "d_return", "d_final_dist", "d_min_margin"):
        np.testing.assert_allclose(got[D[C.CMP_KEYS[k]]], want[D[C.CMP_KEYS[k]]], rtol=1e-12, atol=0, err_msg=k)
    assert want[D["USV_CMP_PAIRS"]].sum() == S * R - len(missing)   # each missing row is the last of its env
    if missing:
        assert (want[D["USV_CMP_PAIRS"]] < R).any()
    again = C.cmp_fold_device(ea, eb, n, S, R, K, thr, DEV)
    assert np.array_equal(bits(again), bits(got))
    from omniisaacgymenvs_loop_amd import _capi
    out = torch.zeros((D["USV_CMP_ROWS"], S), device=DEV, dtype=torch.float64)
    assert _capi.call_rc("usv_cmp_fold", _capi.byref(ea), _capi.byref(eb), n, S, R, K + 1, thr, _capi.ptr(out),
                         _capi.stream_ptr()) == 2
    assert _capi.call_rc("usv_cmp_fold", _capi.byref(ea), None, n, S, R, K, thr, _capi.ptr(out),
                         _capi.stream_ptr()) == 1


# ---------------------------------------------------------------------------------------------- end to end
def _task(n, seed=21, max_len=12):
    from omniisaacgymenvs_loop_amd.tasks.usv_config import load_yaml
    from omniisaacgymenvs_loop_amd.tasks.usv_virtual import USVVirtual
    cfg_d = load_yaml(TASK_YAML)
    cfg_d["env"]["maxEpisodeLength"] = max_len
    return USVVirtual(cfg_d, num_envs=n, device=DEV, seed=seed)


def _actor(obs_dim, seed=3):
    from omniisaacgymenvs_loop_amd.loopz import Actor, MLPEncode_wrap, SquashedGaussianDiagonalCovariance
    arch = MLPEncode_wrap([128, 128], torch.nn.LeakyReLU, obs_dim, 2, torch.nn.Tanh, False, speed_dim=3, mass_dim=8,
                          seed=seed)
    return Actor(arch, SquashedGaussianDiagonalCovariance(2, 0.3, action_scale=[1.0, 1.0]), DEV)


def test_pairing_end_to_end():
    """scenario_pre20, 64 envs, 12-step episodes, R = 3 (K = 1).  The same policy in two arms: no pair differs and
    every difference is exactly 0.  teacher / teacher tails / student_zero_latent complete with PAIRS == R."""
    from omniisaacgymenvs_loop_amd.loopz import LoopzTeacher
    from omniisaacgymenvs_loop_amd.scenario import ScenarioRunner, load_table
    from omniisaacgymenvs_loop_amd.scenario import compare as C
    from omniisaacgymenvs_loop_amd.sysid import StateHistoryEncoder, SysIDStudent, USVSysIDAgent
    table, n, R_ = load_table(PRE20), 64, 3
    actor = _actor(33)

    def factory():
        return ScenarioRunner(_task(n), table, rollouts=R_)

    def teacher(runner):
        return LoopzTeacher(actor, DEV)

    def student(runner, zero_latent):
        enc = StateHistoryEncoder(torch.nn.LeakyReLU, input_size=25, tsteps=50, output_size=8)
        agent = USVSysIDAgent(teacher=actor.architecture, id_encoder=enc, history_len=50, obs_nonpriv_dim=25, device=DEV)
        return SysIDStudent(agent, n, zero_latent=zero_latent)

    res = C.compare(factory, {"teacher": teacher, "teacher_again": teacher})
    assert res["paired_draws"] is True and res["episodes_per_env"] == 1 and res["baseline"] == "teacher"
    cmp = res["pairs"]["teacher_again"]["scenarios"]
    assert (cmp["pairs"] == R_).all() and not cmp["only_a"].any() and not cmp["only_b"].any()
    assert (cmp["collision_a"] == cmp["collision_b"]).all() and (cmp["out_of_bounds_a"] == cmp["out_of_bounds_b"]).all()
    for k in ("d_return", "d_final_dist"):
        assert (cmp[k] == 0.0).all(), k
    for k in ("d_steps", "d_min_margin"):
        assert ((cmp[k] == 0.0) | np.isnan(cmp[k])).all(), k
    assert np.array_equal(np.isnan(cmp["d_steps"]), cmp["both_success"] == 0)
    tot = res["pairs"]["teacher_again"]["totals"]
    assert tot["pairs"] == 20 * R_ and tot["success_diff"]["mean"] == 0.0 and tot["success_diff"]["std"] == 0.0

    arms = C.arm_factories(["teacher", "teacher_base_tail", "teacher_wrong_tail", "student_zero_latent"], teacher,
                           student, seed=5)
    res = C.compare(factory, arms)
    for name in ("teacher_base_tail", "teacher_wrong_tail", "student_zero_latent"):
        c = res["pairs"][name]["scenarios"]
        assert (c["pairs"] == R_).all(), name
        assert ((c["both_success"] + c["only_a"] + c["only_b"] + c["neither"]) == R_).all()
        assert np.isfinite(c["d_return"]).all() and res["arms"][name]["steps"] > 0
    # the override changes what the policy sees, so the arms do not replay the teacher's episodes
    assert (res["pairs"]["teacher_wrong_tail"]["scenarios"]["d_return"] != 0.0).any()
    # the starts are shared: the pairing the differences rest on
    from omniisaacgymenvs_loop_amd._abi import DEFINES as D
    ta = res["arms"]["teacher"]["table"].table.cpu().numpy()
    tz = res["arms"]["student_zero_latent"]["table"].table.cpu().numpy()
    for row in ("START_X", "START_Y", "GOAL_X", "GOAL_Y", "SCENE_IDX"):
        assert np.array_equal(ta[D[f"USV_EV_{row}"]][:n], tz[D[f"USV_EV_{row}"]][:n]), row


def _cfg(num_envs, seed):
    from omniisaacgymenvs_loop_amd.scripts import loopz_train as LT
    cfg = LT.build_config({"num_envs": num_envs, "seed": seed, "train": "USV/USV_MLP"})
    return LT.merge_loopz_overrides(cfg, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(LT.__file__))), "cfg"))


def test_compare_policies_main(tmp_path, monkeypatch):
    """loopz_train for one update at 64 envs, sysid_distill for one update from its checkpoint, then the command
    line on scenario_pre20 with all five arms: the three files and their columns."""
    from omniisaacgymenvs_loop_amd.scripts import compare_policies as CP
    from omniisaacgymenvs_loop_amd.scripts import loopz_train as LT
    from omniisaacgymenvs_loop_amd.scripts import sysid_distill as SD
    monkeypatch.chdir(tmp_path)
    cfg = _cfg(64, 3)
    cfg["environment"]["max_time"] = 0.16
    cfg["environment"]["eval_every_n"] = 1
    LT.train(cfg, max_updates=1, log=lambda *a: None)
    ckpt = str(tmp_path / "runs" / "USV" / "nn" / "full_1.pt")
    cfg = _cfg(64, 3)
    cfg["checkpoint"] = ckpt
    cfg["environment"]["sysid_eval_every_n"] = 1
    _, _, _, _, ckpt_dir = SD.distill(cfg, max_updates=1, run_dir=str(tmp_path / "run"), log=lambda *a: None)
    enc = os.path.join(ckpt_dir, "id_encoder_1.pth")
    assert os.path.exists(enc)
    out_dir = str(tmp_path / "compare")
    res, meta = CP.main(["num_envs=64", "task.env.maxEpisodeLength=12", f"scenario_npz={PRE20}", f"checkpoint={ckpt}",
                         f"id_encoder={enc}", f"out_dir={out_dir}", "compare.n_rollouts=3"])
    arms = CP.ARMS.split(",")
    assert sorted(os.listdir(out_dir)) == ["compare.meta.json", "compare_pairs.csv", "compare_scenarios.csv"]
    scen = list(csv.reader(open(os.path.join(out_dir, "compare_scenarios.csv"))))
    assert scen[0] == CP.SCENARIO_COLUMNS and len(scen) - 1 == 20 * len(arms)
    assert [r[0] for r in scen[1::20]] == arms
    pairs = list(csv.reader(open(os.path.join(out_dir, "compare_pairs.csv"))))
    assert pairs[0] == CP.PAIR_COLUMNS and len(pairs) - 1 == 20 * (len(arms) - 1)
    assert all(r[0] == "teacher" and int(r[4]) == 3 for r in pairs[1:])
    on_disk = json.load(open(os.path.join(out_dir, "compare.meta.json")))
    assert on_disk["paired_draws"] is True and on_disk["arms"] == arms and on_disk["baseline"] == "teacher"
    assert set(on_disk["totals"]) == set(arms[1:]) and set(on_disk["per_arm"]) == set(arms)
    for name in arms[1:]:
        t = on_disk["totals"][name]
        assert t["pairs"] == 60 and {"count", "mean", "std", "ci95_lo", "ci95_hi"} <= set(t["success_diff"])
    assert all(on_disk["per_arm"][a]["wall_s"] > 0 for a in arms)
    assert meta["student_kernel"] in KERNELS
