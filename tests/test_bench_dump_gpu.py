"""bench.py's plain run and --dump-outputs on the GPU: the result line of a plain run carries the headline and
none of the --full measurements, --steps sets the number of timed epochs, and two runs with the same arguments
write the same arrays (float32 / float64, inside the byte budget), so two builds can be compared output for output."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY_KEYS = ("roofline", "roofline_ppo", "cpu_baseline", "sustained", "wall_clock_to_reward", "fps_step_inference",
                  "fps_step_env_only")
ENVS, STEPS = 4096, 3          # 65,536 batch rows: the experience arrays are written whole; 8 minibatches per mini-epoch


def _run(bench, capsys, out_dir, envs=ENVS):
    out = bench.main(["--gpus", "1", "--steps", str(STEPS), "--warmup", "2", "--envs", str(envs),
                      "--dump-outputs", str(out_dir)])
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    assert line["value"] == out["value"]
    return line, {f[:-4]: np.load(os.path.join(out_dir, f), allow_pickle=False) for f in sorted(os.listdir(out_dir))}


def test_plain_run_line_and_dump_repeatable(tmp_path, capsys):
    import bench
    line_a, a = _run(bench, capsys, tmp_path / "a")
    line_b, b = _run(bench, capsys, tmp_path / "b")
    for k in HEADLINE_KEYS:
        assert k in line_a, k
    assert not [k for k in FULL_ONLY_KEYS if k in line_a]
    assert not [k for k in line_a["extra"] if k in ("seeds", "c2", "c3", "c4_pose", "c4_track", "device_only")]
    assert line_a["steps"] == STEPS and line_a["n_gpus"] == 1 and line_a["dtype"] == "fp32"
    assert line_a["dump_outputs"]["after_epoch"] == 2 + STEPS      # 2 warmup epochs, then exactly STEPS timed ones
    assert np.isfinite(line_a["value"]) and line_a["value"] > 0
    np.testing.assert_allclose(line_a["value"], ENVS * 16 * 1e3 / line_a["ms_per_step"], rtol=1e-9)
    # the dump: every array float32 / float64, finite, inside the budget, whole at this size
    assert set(a) >= {"params", "adam_m", "adam_v", "obs_rms", "val_rms", "obs", "dones", "env_state", "exp_obs",
                      "exp_act", "exp_ret", "exp_adv", "loss_log"}
    assert "exp_rows" not in a and "env_rows" not in a
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BUDGET_BYTES
    assert a["obs"].shape == (ENVS, 33) and a["env_state"].shape == (ENVS, 8) and a["exp_obs"].shape == (ENVS * 16, 33)
    assert a["obs_rms"].dtype == np.float64
    assert all(np.isfinite(v).all() for v in a.values())
    assert np.abs(a["adam_m"]).max() > 0 and np.abs(a["exp_adv"]).max() > 0      # the epoch ran: not the initial zeros
    # same arguments, same inputs, same outputs
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)

