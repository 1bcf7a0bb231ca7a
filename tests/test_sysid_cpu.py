"""SysID distillation without a GPU: the torch restatement (tests/sysid_restate.py) against the fixture the
reference's own classes produced (tests/golden/sysid_golden.npz, make_sysid_golden.py), the argument checks of the
sysid entry points, the host-side containers, the StepLR closed form and the exported files."""
import ctypes
import os

import numpy as np
import pytest
import torch
import yaml

from tests import errtab
from tests import sysid_restate as R

TOL = 1e-5
D = 25


def param_check(got, want, F, shapes, what):
    """|got - want| <= max(1e-6 + 1e-5 |w|, 4 F) per tensor, F that tensor's max |float64 restatement - fixture|
    (Adam divides by sqrt(v): parameters with near-zero gradients are ill-conditioned, and two float32 summation
    orders differ by about what float32 differs from float64).  Returns the largest error / bound per tensor."""
    p, ratios = 0, []
    for k, s in zip(R.ENC_KEYS, shapes):
        n = int(np.prod(s))
        g, w = got[p:p + n].astype(np.float64), want[p:p + n].astype(np.float64)
        f = float(np.abs(F[p:p + n]).max())
        bound = np.maximum(1e-6 + 1e-5 * np.abs(w), 4 * f)
        ratios.append(float((np.abs(g - w) / bound).max()))
        print(f"{what} {k}: max err {np.abs(g - w).max():.3g}  F {f:.3g}  err/bound {ratios[-1]:.3g}")
        p += n
    assert max(ratios) <= 1.0, (what, ratios)
    return ratios


@pytest.fixture(scope="module")
def fx(golden):
    return golden("sysid_golden.npz")


@pytest.fixture(scope="module")
def runs(fx):
    """The restatement on the fixture's stream: float32 both modes, float64 for the conditioning yardstick."""
    t = R.unflatten(fx["teacher"], R.TEACHER_KEYS, R.teacher_shapes(D))
    e = R.unflatten(fx["enc0"], R.ENC_KEYS, R.enc_shapes(D))
    out = {m: R.run(fx["obs"], fx["dones"], t, e, mode=m, keep_hist=True) for m in ("zeros", "repeat")}
    for m in ("zeros", "repeat"):
        out[m + "64"] = R.run(fx["obs"], fx["dones"], t, e, mode=m, dtype=torch.float64)
    return out


@pytest.mark.parametrize("mode", ["zeros", "repeat"])
def test_restatement_matches_the_reference(fx, runs, mode):
    r, name = runs[mode], f"sysid_restate[{mode}]"
    for i, k in enumerate(fx["hist_steps"]):
        np.testing.assert_array_equal(r["hist"][k], fx[f"{mode}_hist"][i], err_msg=f"window at step {k}")
    for q in ("zhat", "zstar", "actions"):
        errtab.check(name, q, r[q], fx[f"{mode}_{q}"], TOL, TOL)
    np.testing.assert_allclose(np.concatenate(r["losses"]), fx[f"{mode}_losses"], rtol=TOL)
    names = list(fx["metric_names"])
    for u in range(5):
        for j, k in enumerate(names):
            np.testing.assert_allclose(r["metrics"][u][k], fx[f"{mode}_metrics"][u, j], rtol=TOL,
                                       atol=1e-6 if k.startswith("r2") else 0, err_msg=f"update {u + 1} {k}")
    if mode == "zeros":
        g = fx["zeros_grad0"]
        np.testing.assert_allclose(r["grads"][0][0], g, rtol=0, atol=TOL * np.abs(g).max())
        param_check(r["params"][0], fx["zeros_params1"], runs["zeros64"]["params"][0] - fx["zeros_params1"],
                    R.enc_shapes(D), "update 1")
    param_check(r["params"][4], fx[f"{mode}_params5"], runs[mode + "64"]["params"][4] - fx[f"{mode}_params5"],
                R.enc_shapes(D), f"{mode} update 5")


def test_fixture_covers_the_quirks(fx):
    """Windows fill past 50 frames and cross update boundaries; there are dones; in the default mode a done leaves
    the window sliding (the frame before the done is still in it), in "repeat" mode it refills the window."""
    assert fx["obs"].shape == (81, 6, 33) and fx["dones"].sum() > 3 and fx["dones"][3, 1] == 1
    steps = list(fx["hist_steps"])
    z, r = fx["zeros_hist"][steps.index(4)].reshape(6, 50, D), fx["repeat_hist"][steps.index(4)].reshape(6, 50, D)
    np.testing.assert_array_equal(z[1, -2], fx["obs"][3, 1, :D])          # the pre-done frame survives
    np.testing.assert_array_equal(r[1], np.broadcast_to(fx["obs"][4, 1, :D], (50, D)))
    np.testing.assert_array_equal(fx["zeros_hist"][0].reshape(6, 50, D)[:, :-1], 0)
    full = fx["zeros_hist"][steps.index(49)].reshape(6, 50, D)
    np.testing.assert_array_equal(full, np.transpose(fx["obs"][:50, :, :D], (1, 0, 2)))


def test_state_dict_keys_and_shapes_are_the_references(fx):
    from omniisaacgymenvs_loop_amd.sysid import StateHistoryEncoder
    enc = StateHistoryEncoder(torch.nn.LeakyReLU, input_size=D, tsteps=50, output_size=8, seed=1)
    want = [(k, tuple(int(v) for v in s.split(","))) for k, s in zip(fx["enc_keys"], fx["enc_shapes"])]
    assert [(k, tuple(v.shape)) for k, v in enc.state_dict().items()] == want
    assert enc.numel() == 20136 and enc.input_shape == 50 * D and enc.output_shape == 8
    # PyTorch's default init: every tensor within 1 / sqrt(fan_in) of zero, and not degenerate
    for k, v in enc.state_dict().items():
        fan_in = int(np.prod(enc.state_dict()[k.replace("bias", "weight")].shape[1:]))
        assert float(v.abs().max()) <= 1.0 / np.sqrt(fan_in) + 1e-7 and float(v.std()) > 0.2 / np.sqrt(fan_in)
    # the CPU mirror is the restatement's network
    h = torch.randn(3, 50 * D)
    with torch.no_grad():
        np.testing.assert_allclose(enc.torch_mirror()(h).numpy(), R.encoder_forward(enc.state_dict(), h).numpy(),
                                   rtol=1e-6, atol=1e-7)
    for bad in (dict(tsteps=20), dict(output_size=4)):
        with pytest.raises(NotImplementedError):
            StateHistoryEncoder(torch.nn.LeakyReLU, **{**dict(input_size=D, tsteps=50, output_size=8), **bad})


def _lib():
    from omniisaacgymenvs_loop_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libusv_hip.so not built (run __graft_entry__.build())")
    return _capi.lib()


def test_argument_statuses():
    """NULL pointers give status 1, history_len != 50 or an obs_dim outside 33..36 the unsupported-configuration
    status 2, before any device work (there is no device here)."""
    lib = _lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf) % 16)   # host scratch: never dereferenced
    n, H = 6, 16
    assert lib.sysid_nparam(33) == 20136 and lib.sysid_nparam(36) == 20136 + 3 * 32
    assert lib.sysid_nparam(32) <= 0 and lib.sysid_nparam(37) <= 0
    assert lib.sysid_partials_floats(33, 24) >= 3 * 20137 and lib.sysid_partials_floats(40, 24) <= 0

    def append(obs=p, obs_dim=33, T=50):
        return lib.sysid_append(obs, None, p, n, obs_dim, T, H, 0, 0, 0, 1, p, p, p, p, None)

    def encode(enc=p, obs_dim=33, T=50, row0=0, rows=n):
        return lib.sysid_encode(enc, n, obs_dim, T, H, 0, row0, rows, p, p, p, None)

    def step(teacher=p, obs_dim=33, T=50):
        return lib.sysid_student_step(p, teacher, n, obs_dim, T, H, 0, 0, p, p, p, p, None)

    def minibatch(enc=p, obs_dim=33, T=50, rows=24):
        return lib.sysid_minibatch(enc, p, p, n, obs_dim, T, H, 0, 0, rows, ctypes.c_float(5e-4), 1, 1, p, p, p, p, p, p,
                                   None)

    def metrics(out=p, obs_dim=33, T=50):
        return lib.sysid_metrics(p, n, obs_dim, T, H, 0, p, p, p, p, 16, 4, p, p, out, None)

    for fn, null in ((append, dict(obs=None)), (encode, dict(enc=None)), (step, dict(teacher=None)),
                     (minibatch, dict(enc=None)), (metrics, dict(out=None))):
        assert fn(**null) == 1, fn.__name__
        assert fn(T=20) == 2 and fn(T=10) == 2, fn.__name__
        assert fn(obs_dim=29) == 2 and fn(obs_dim=37) == 2, fn.__name__
    assert encode(row0=n * H) == 1 and encode(rows=0) == 1 and minibatch(rows=n * H + 1) == 1


def test_teacher_checkpoint_round_trip(tmp_path):
    """A loopz full_<update>.pt as scripts/loopz_train.save_full writes it gives the teacher back bit for bit."""
    from omniisaacgymenvs_loop_amd.loopz import Actor, Critic, MLPEncode_wrap, SquashedGaussianDiagonalCovariance
    from omniisaacgymenvs_loop_amd.scripts.loopz_train import save_full
    from omniisaacgymenvs_loop_amd.sysid import action_head_mirror, load_teacher
    kw = dict(speed_dim=3, mass_dim=8, mass_latent_dim=8, mass_encoder_shape=(64, 16))
    actor = Actor(MLPEncode_wrap([128, 128], torch.nn.LeakyReLU, 33, 2, torch.nn.Tanh, False, seed=5, **kw),
                  SquashedGaussianDiagonalCovariance(2, 0.3))
    critic = Critic(MLPEncode_wrap([128, 128], torch.nn.LeakyReLU, 33, 1, seed=6, **kw))

    class _NoOptimizer:
        def optimizer_state_dict(self):
            return {}
    path = str(tmp_path / "full_7.pt")
    save_full(path, actor, critic, _NoOptimizer(), 7)
    teacher = load_teacher(path, 33)
    for k, v in actor.architecture.state_dict().items():
        assert torch.equal(teacher.state_dict()[k], v), k
    # the exported action head is the restatement's
    x = torch.randn(4, 33)
    with torch.no_grad():
        np.testing.assert_allclose(action_head_mirror(teacher)(x).numpy(),
                                   R.action_head(teacher.state_dict(), x).numpy(), rtol=1e-6, atol=1e-7)
    torch.save({"model": {}}, str(tmp_path / "other.pt"))
    with pytest.raises(RuntimeError, match="actor_architecture_state_dict"):
        load_teacher(str(tmp_path / "other.pt"), 33)


def test_step_lr_is_torchs():
    from omniisaacgymenvs_loop_amd.sysid import step_lr
    w = torch.zeros(1, requires_grad=True)
    opt = torch.optim.Adam([w], lr=5e-4)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=200, gamma=0.1)
    seen = {}
    for u in range(401):
        seen[u] = opt.param_groups[0]["lr"]
        opt.step()
        sched.step()
    for u in (0, 199, 200, 399, 400):
        assert step_lr(5e-4, u) == pytest.approx(seen[u], rel=1e-12), u
    assert step_lr(5e-4, 199) == 5e-4 and step_lr(5e-4, 200) == pytest.approx(5e-5) \
        and step_lr(5e-4, 400) == pytest.approx(5e-6)


def test_export_meta_and_traced_files(tmp_path):
    from omniisaacgymenvs_loop_amd.loopz import MLPEncode_wrap
    from omniisaacgymenvs_loop_amd.scripts.sysid_distill import export_meta, export_student
    from omniisaacgymenvs_loop_amd.sysid import StateHistoryEncoder
    d = str(tmp_path / "nn")
    export_meta(d, history_len=50, priv_dim=8, speed_dim=3, obs_nonpriv_dim=D, mass_latent_dim=8,
                checkpoint="runs/USV/nn/full_0.pt", device="cuda:0", eval_every_n=100)
    with open(os.path.join(d, "export_meta.yaml")) as f:
        meta = yaml.safe_load(f)
    assert meta == {"history_len": 50, "priv_dim": 8, "mass_dim": 8, "speed_dim": 3, "obs_nonpriv_dim": 25,
                    "history_dim": 1250, "mass_latent_dim": 8, "action_in_dim": 33,
                    "checkpoint": "runs/USV/nn/full_0.pt", "device": "cuda:0", "eval_every_n": 100}
    enc = StateHistoryEncoder(torch.nn.LeakyReLU, input_size=D, tsteps=50, output_size=8, seed=2)
    teacher = MLPEncode_wrap([128, 128], torch.nn.LeakyReLU, 33, 2, torch.nn.Tanh, False, speed_dim=3, mass_dim=8,
                             mass_latent_dim=8, mass_encoder_shape=(64, 16), seed=3)
    id_path, act_path = export_student(d, 1, enc, teacher)
    ts_enc, ts_act = torch.jit.load(id_path), torch.jit.load(act_path)
    h, x = torch.randn(5, 1250), torch.randn(5, 33)
    with torch.no_grad():
        np.testing.assert_allclose(ts_enc(h).numpy(), R.encoder_forward(enc.state_dict(), h).numpy(), rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(ts_act(x).numpy(), R.action_head(teacher.state_dict(), x).numpy(), rtol=1e-6, atol=1e-7)
    sd = torch.load(os.path.join(d, "id_encoder_1.pth"), map_location="cpu", weights_only=True)
    assert list(sd) == R.ENC_KEYS and all(torch.equal(sd[k], v) for k, v in enc.state_dict().items())
