"""SysID distillation on the GPU (csrc/usv_sysid.hip through omniisaacgymenvs_loop_amd.sysid) against the fixture
the reference's own classes produced (tests/golden/sysid_golden.npz) and, for shapes the fixture cannot hold, the
torch restatement (tests/sysid_restate.py, validated against the fixture by tests/test_sysid_cpu.py)."""
import os

import numpy as np
import pytest
import torch

from tests import errtab
from tests import sysid_restate as R
from tests.test_sysid_cpu import param_check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
D, H = 25, 16


def make_agent(teacher_sd, enc_sd, obs_dim=33):
    from omniisaacgymenvs_loop_amd.loopz import MLPEncode_wrap
    from omniisaacgymenvs_loop_amd.sysid import StateHistoryEncoder, USVSysIDAgent
    teacher = MLPEncode_wrap([128, 128], torch.nn.LeakyReLU, obs_dim, 2, torch.nn.Tanh, False, speed_dim=3, mass_dim=8,
                             mass_latent_dim=8, mass_encoder_shape=(64, 16))
    teacher.load_state_dict(teacher_sd)
    enc = StateHistoryEncoder(torch.nn.LeakyReLU, input_size=obs_dim - 8, tsteps=50, output_size=8)
    enc.load_state_dict(enc_sd)
    return USVSysIDAgent(teacher=teacher, id_encoder=enc, history_len=50, obs_nonpriv_dim=obs_dim - 8, device=DEV)


class ReplayEnv:
    """What USVSysIDTrainer touches of a USVSysIDVecEnv, fed from a recorded stream."""

    def __init__(self, n, obs_dim, mode, horizon=H):
        from omniisaacgymenvs_loop_amd.sysid import HistoryStream
        self.history = HistoryStream(n, obs_dim, horizon=horizon, fill_history_on_reset=mode, device=DEV)

    def _flush(self):
        pass


def replay(obs, dones, teacher_sd, enc_sd, mode="zeros", n_updates=None, update=True, keep=()):
    """The loop of the reference's script on the device: returns per-step zhat / zstar / actions, the windows at the
    steps in `keep`, and per update the minibatch losses, parameters and metrics."""
    from omniisaacgymenvs_loop_amd.sysid import USVSysIDTrainer
    S, n, obs_dim = len(dones), obs.shape[1], obs.shape[2]
    agent = make_agent(teacher_sd, enc_sd, obs_dim)
    env = ReplayEnv(n, obs_dim, mode)
    tr = USVSysIDTrainer(actor=agent, num_envs=n, num_transitions_per_env=H, history_dim=50 * (obs_dim - 8), latent_dim=8,
                         device=DEV, env=env)
    hs = env.history
    out = {"zhat": [], "zstar": [], "actions": [], "hist": {}, "losses": [], "params": [], "metrics": []}
    o_dev, d_dev = torch.tensor(obs, device=DEV), torch.tensor(dones, device=DEV)
    hs.reset()
    hs.append(o_dev[0], None)
    for k in range(S):
        if k in keep:
            out["hist"][k] = hs.window().reshape(n, -1).cpu().numpy()
        out["actions"].append(tr.observe_device().cpu().numpy())
        out["zhat"].append(tr.zhat.cpu().numpy())
        out["zstar"].append(hs.zstar[hs.row].cpu().numpy())
        tr.step()
        if (k + 1) % H == 0 and update:
            out["metrics"].append(tr.update())
            out["losses"].append(tr.losses.cpu().numpy().copy())
            out["params"].append(agent.enc_flat.cpu().numpy().copy())
            if n_updates is not None and len(out["params"]) >= n_updates:
                break
        if k + 1 < S:   # the rows of the last update stay in place
            hs.append(o_dev[k + 1], d_dev[k])
    for q in ("zhat", "zstar", "actions"):
        out[q] = np.stack(out[q])
    out["trainer"] = tr
    return out


@pytest.fixture(scope="module")
def fx(golden):
    return golden("sysid_golden.npz")


@pytest.fixture(scope="module")
def nets(fx):
    return (R.unflatten(fx["teacher"], R.TEACHER_KEYS, R.teacher_shapes(D)),
            R.unflatten(fx["enc0"], R.ENC_KEYS, R.enc_shapes(D)))


@pytest.fixture(scope="module")
def dev_runs(fx, nets):
    keep = set(int(k) for k in fx["hist_steps"])
    return {m: replay(fx["obs"], fx["dones"], *nets, mode=m, keep=keep) for m in ("zeros", "repeat")}


@pytest.mark.parametrize("mode", ["zeros", "repeat"])
def test_history_windows_are_the_references_bit_for_bit(fx, dev_runs, mode):
    """Pure data movement: the window of every recorded step (first frames, after a done, the first full window,
    across update boundaries) equals the reference's history buffer exactly, in both fill modes."""
    for i, k in enumerate(fx["hist_steps"]):
        np.testing.assert_array_equal(dev_runs[mode]["hist"][int(k)], fx[f"{mode}_hist"][i], err_msg=f"step {k}")


@pytest.mark.parametrize("mode", ["zeros", "repeat"])
def test_forward_vs_reference(fx, dev_runs, mode):
    r = dev_runs[mode]
    for q in ("zhat", "zstar", "actions"):
        errtab.check(f"sysid_forward[{mode}]", q, r[q], fx[f"{mode}_{q}"], TOL, TOL)


@pytest.mark.parametrize("n,obs_dim", [(1, 33), (70, 33), (70, 36)])
def test_forward_vs_restatement(n, obs_dim):
    """One env, and 70 envs (no multiple of the 8-row tile or the action head's 16), 60 steps without updates so the
    windows fill and wrap the ring; the widest observation loopz accepts too."""
    obs, dones = R.make_stream(n, 60, obs_dim, seed=100 + n)
    t, e = R.random_teacher(obs_dim - 8, 31), R.random_enc(obs_dim - 8, 32)
    for mode in ("zeros", "repeat"):
        want = R.run(obs, dones, t, e, mode=mode, horizon=10 ** 6)
        got = replay(obs, dones, t, e, mode=mode, update=False)
        for q in ("zhat", "zstar", "actions"):
            errtab.check(f"sysid_forward[n={n},obs={obs_dim}]", q, got[q], want[q], TOL, TOL)


def test_first_minibatch_gradient_vs_reference(fx, nets):
    r = replay(fx["obs"][:17], fx["dones"][:16], *nets, update=False)
    tr = r["trainer"]
    tr.minibatch(0, 24, apply=False)
    g, want = tr.grad.cpu().numpy(), fx["zeros_grad0"]
    print("max |grad| %.3g  max err %.3g" % (np.abs(want).max(), np.abs(g - want).max()))
    np.testing.assert_allclose(g, want, rtol=0, atol=TOL * np.abs(want).max())
    np.testing.assert_allclose(tr.losses[0].item(), fx["zeros_losses"][0], rtol=TOL)
    assert np.array_equal(tr.actor.enc_flat.cpu().numpy(), fx["enc0"])   # apply = 0 leaves the parameters alone


@pytest.mark.parametrize("n,mode", [(6, "zeros"), (7, "repeat")])
def test_teacher_forced_gradients_vs_restatement(fx, nets, n, mode):
    """Every one of the 16 Adam steps of an update: the restatement's parameters before the step are loaded, the
    device gradient of that minibatch must match the restatement's to 1e-5 of its max.  n = 6: 24-row minibatches
    (the fixture's stream); n = 7: 28 rows, no multiple of the 8-row tile, at unaligned row offsets."""
    if n == 6:
        obs, dones, (t, e) = fx["obs"][:17], fx["dones"][:16], nets
    else:
        obs, dones = R.make_stream(n, 16, 33, seed=7, done_rate=0.1)
        t, e = R.random_teacher(D, 41), R.random_enc(D, 42)
    want = R.run(obs, dones, t, e, mode=mode)
    tr = replay(obs, dones, t, e, mode=mode, update=False)["trainer"]
    M = n * H // 4
    for i in range(16):
        tr.actor.enc_flat.copy_(torch.tensor(want["pre"][0][i], device=DEV))
        tr.minibatch((i % 4) * M, M, apply=False, loss_slot=i)
        g, w = tr.grad.cpu().numpy(), want["grads"][0][i]
        np.testing.assert_allclose(g, w, rtol=0, atol=TOL * np.abs(w).max(), err_msg=f"step {i}")
    np.testing.assert_allclose(tr.losses.cpu().numpy(), want["losses"][0], rtol=TOL)


def test_many_tiles_per_workgroup_vs_restatement():
    """1,040 envs: 4,160-row minibatches are 520 tiles on 256 gradient workgroups, and the 16,640 rows of the
    metrics' forward are 2,080 tiles on 2,048 workgroups, so both kernels loop over tiles (accumulators carried
    from tile to tile).  One epoch of the restatement; gradients of the first and last minibatch, metrics."""
    n = 1040
    obs, dones = R.make_stream(n, 16, 33, seed=9)
    t, e = R.random_teacher(D, 51), R.random_enc(D, 52)
    want = R.run(obs, dones, t, e, epochs=1)
    tr = replay(obs, dones, t, e, update=False)["trainer"]
    M = n * H // 4
    for i in (0, 3):
        tr.actor.enc_flat.copy_(torch.tensor(want["pre"][0][i], device=DEV))
        tr.minibatch(i * M, M, apply=False, loss_slot=i)
        g, w = tr.grad.cpu().numpy(), want["grads"][0][i]
        np.testing.assert_allclose(g, w, rtol=0, atol=TOL * np.abs(w).max(), err_msg=f"minibatch {i}")
        np.testing.assert_allclose(tr.losses[i].item(), want["losses"][0][i], rtol=TOL)
    from omniisaacgymenvs_loop_amd import _capi
    from omniisaacgymenvs_loop_amd.sysid import metrics_dict
    tr.actor.enc_flat.copy_(torch.tensor(want["params"][0], device=DEV))
    hs = tr.hs
    _capi.call("sysid_metrics", _capi.ptr(tr.actor.enc_flat), *hs.geometry(), _capi.ptr(hs.stream),
               _capi.ptr(hs.valid_rows), _capi.ptr(hs.zstar), _capi.ptr(tr.losses), 4, 4, _capi.ptr(tr.zhat_all),
               _capi.ptr(tr.metrics_work), _capi.ptr(tr.metrics_dev), _capi.stream_ptr())
    m = metrics_dict(tr.metrics_dev.cpu().numpy())
    for k, v in want["metrics"][0].items():
        if k != "mse":
            np.testing.assert_allclose(m[k], v, rtol=TOL, atol=1e-6 if k.startswith("r2") else 0, err_msg=k)


@pytest.mark.parametrize("mode", ["zeros", "repeat"])
def test_update_vs_reference(fx, nets, dev_runs, mode):
    """Five updates on the fixture's stream: per-minibatch losses, the parameters after updates 1 and 5 (bound
    max(1e-6 + 1e-5 |w|, 4 F) per tensor, F = max |float64 restatement - fixture|), every returned metric."""
    r = dev_runs[mode]
    np.testing.assert_allclose(np.concatenate(r["losses"]), fx[f"{mode}_losses"], rtol=TOL)
    names = list(fx["metric_names"])
    for u in range(5):
        for j, k in enumerate(names):
            np.testing.assert_allclose(r["metrics"][u][k], fx[f"{mode}_metrics"][u, j], rtol=TOL,
                                       atol=1e-6 if k.startswith("r2") else 0, err_msg=f"update {u + 1} {k}")
    r64 = R.run(fx["obs"], fx["dones"], *nets, mode=mode, dtype=torch.float64)
    if mode == "zeros":
        param_check(r["params"][0], fx["zeros_params1"], r64["params"][0] - fx["zeros_params1"], R.enc_shapes(D),
                    "device update 1")
    param_check(r["params"][4], fx[f"{mode}_params5"], r64["params"][4] - fx[f"{mode}_params5"], R.enc_shapes(D),
                f"device {mode} update 5")
    assert r["trainer"].itr == 5 and r["trainer"].adam_step == 80


def test_two_runs_give_the_same_bits(fx, nets, dev_runs):
    again = replay(fx["obs"], fx["dones"], *nets, mode="zeros")
    for u in range(5):
        assert np.array_equal(again["params"][u], dev_runs["zeros"]["params"][u]), u
        assert np.array_equal(again["losses"][u], dev_runs["zeros"]["losses"][u]), u


def _cfg(num_envs, seed):
    from omniisaacgymenvs_loop_amd.scripts import loopz_train as LT
    cfg = LT.build_config({"num_envs": num_envs, "seed": seed, "train": "USV/USV_MLP"})
    return LT.merge_loopz_overrides(cfg, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(LT.__file__))), "cfg"))


def test_wrapper_does_not_disturb_the_env():
    """20 steps with the SysID wrapper attached (history read every step) leave the env state bit-identical to the
    same steps through the plain loopz adapter."""
    from omniisaacgymenvs_loop_amd.envs.vec_env_rlgames import VecEnvRLGames
    from omniisaacgymenvs_loop_amd.loopz import USVRaisimVecEnv
    from omniisaacgymenvs_loop_amd.sysid import USVSysIDVecEnv
    from omniisaacgymenvs_loop_amd.utils.task_util import initialize_task
    g = torch.Generator().manual_seed(0)
    actions = (torch.rand((20, 64, 2), generator=g) * 2 - 1).to(DEV)
    states = []
    for wrapped in (False, True):
        rlg = VecEnvRLGames(headless=True)
        initialize_task(_cfg(64, 5), rlg)
        env = USVSysIDVecEnv(rlg, history_len=50, priv_dim=8, horizon=16) if wrapped else USVRaisimVecEnv(rlg)
        env.reset()
        for k in range(20):
            if wrapped:
                assert env.observe_sysid_obs_device().shape == (64, 51 * D)
            env.step_device(actions[k])
        states.append((rlg._task.state.cpu().numpy().copy(), env.observe_device().cpu().numpy().copy()))
    np.testing.assert_array_equal(states[0][0], states[1][0])
    np.testing.assert_array_equal(states[0][1], states[1][1])


def test_end_to_end_train_distill_export_evaluate(tmp_path, monkeypatch):
    """loopz_train for one update at 64 envs, sysid_distill for two updates from its checkpoint: finite metrics, the
    exported files, the traced encoder on the CPU reproducing the device's z^ of the stored batch, and the student
    as a policy under eval.rollout for one episode per env."""
    from omniisaacgymenvs_loop_amd.eval import EpisodeEvaluator, rollout
    from omniisaacgymenvs_loop_amd.scripts import loopz_train as LT
    from omniisaacgymenvs_loop_amd.scripts import sysid_distill as SD
    from omniisaacgymenvs_loop_amd.sysid import SysIDStudent
    monkeypatch.chdir(tmp_path)
    cfg = _cfg(64, 3)
    cfg["environment"]["max_time"] = 0.16
    cfg["environment"]["eval_every_n"] = 1
    LT.train(cfg, max_updates=1, log=lambda *a: None)
    cfg = _cfg(64, 3)
    cfg["checkpoint"] = str(tmp_path / "runs" / "USV" / "nn" / "full_1.pt")
    cfg["environment"]["sysid_eval_every_n"] = 2
    lines = []
    hist, env, agent, trainer, ckpt_dir = SD.distill(cfg, max_updates=2, run_dir=str(tmp_path / "run"), log=lines.append)
    assert len(hist) == 2 and all(np.isfinite(v) for m in hist for v in m.values())
    assert lines[-1].startswith("[sysid] update=2 mse=") and " r2=" in lines[-1] and " fps=" in lines[-1]
    for f in ("export_meta.yaml", "id_encoder_1.pt", "action_mlp_1.pt", "id_encoder_1.pth", "id_encoder_2.pt",
              "action_mlp_2.pt", "id_encoder_2.pth"):
        assert os.path.exists(os.path.join(ckpt_dir, f)), f
    hs = trainer.hs
    assert hs.full
    agent.encode_rows(hs, 0, 64 * 16, trainer.zhat_all)
    windows = torch.cat([hs.window(s).reshape(64, -1) for s in range(16)]).cpu()
    with torch.no_grad():
        z_cpu = torch.jit.load(os.path.join(ckpt_dir, "id_encoder_2.pt"))(windows).numpy()
    errtab.check("sysid_end_to_end", "traced zhat", trainer.zhat_all.cpu().numpy(), z_cpu, TOL, TOL)
    task = env._task
    student = SysIDStudent(agent, 64)
    steps, complete = rollout(task, student, EpisodeEvaluator(task, 1))
    assert complete and steps > 0
    assert torch.isfinite(student.actions).all() and float(student.actions.abs().max()) <= 1.0
