"""Scenario tables on the host against the reference's recorded outputs (tests/golden/scenario_golden.npz and the
reference-written table scenario_pre20.npz; tests/golden/make_scenario_golden.py): the numpy sampler, the
geometry-only selections, the metrics restatement, the filter's selection, the table IO, and the argument checks
of the four C entry points (no device work)."""
import ctypes
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE20 = os.path.join(ROOT, "tests", "golden", "scenario_pre20.npz")
ARRAYS = ("obstacles_xy", "spawn_root_pos", "spawn_root_rot", "target_pos", "target_rot", "init_root_vel_xy")
METRICS = ("d_spawn", "d_goal", "d_corr", "d_oo", "density_score")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def gold(golden):
    return golden("scenario_golden.npz")


@pytest.fixture(scope="module")
def cands(gold):
    from omniisaacgymenvs_loop_amd.scenario import SamplingParams, build_candidates
    d = json.loads(str(gold["defaults"]))
    params = SamplingParams(**{k: d[k] for k in SamplingParams().meta()})
    return build_candidates(d["n_candidates"], d["seed"], params, sampler="numpy"), d


def same_scenarios(gold, prefix, c, idx=None):
    for k in ARRAYS:
        got = c[k] if idx is None else c[k][idx]
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(gold[f"{prefix}_{k}"])), (prefix, k)
    h = c["obstacles_hash"] if idx is None else c["obstacles_hash"][idx]
    assert [str(x) for x in h] == [str(x) for x in gold[f"{prefix}_obstacles_hash"]]
    for k in METRICS:   # the reference's Python floats, bit for bit
        got = c["metrics"][k] if idx is None else c["metrics"][k][idx]
        assert got.dtype == np.float64 and np.array_equal(bits(got), bits(gold[f"{prefix}_{k}"])), (prefix, k)


def test_numpy_sampler_reproduces_build_candidates(gold, cands):
    c, d = cands
    assert c["obstacles_xy"].shape == (d["n_candidates"], 16, 2)
    same_scenarios(gold, "cand", c)
    assert np.array_equal(gold["cand_scenario_id"], np.arange(d["n_candidates"]))


def test_preselect_and_select_reproduce_the_reference(gold, cands):
    from omniisaacgymenvs_loop_amd.scenario import preselect, select_from_pre
    c, d = cands
    idx, summary = preselect(c["metrics"]["density_score"], d["n_preselect"], tuple(d["ratio"]), seed=d["seed"] + 1)
    assert np.array_equal(idx, gold["pre_source_candidate_id"]) and idx.dtype == np.int64
    assert summary == json.loads(str(gold["pre_summary"]))   # the quantiles included, as floats
    same_scenarios(gold, "pre", c, idx)
    sel, sel_summary = select_from_pre(c["metrics"]["density_score"][idx], d["n_selected"], seed=d["seed"] + 2)
    assert sel_summary == json.loads(str(gold["sel_summary"]))
    same_scenarios(gold, "sel", c, idx[sel])
    assert np.array_equal(gold["sel_scenario_id"], np.arange(d["n_selected"]))


def test_metrics_restatement_equals_the_reference_on_all_67(gold):
    from omniisaacgymenvs_loop_amd.scenario import METRIC_KEYS, metrics_host
    assert METRIC_KEYS == METRICS
    m = metrics_host(gold["m_obstacles_xy"], gold["m_spawn_xy"], gold["m_goal_xy"], 0.5)
    want = gold["m_out"]
    assert want.shape == (5, 67)
    for i, k in enumerate(METRICS):
        assert np.array_equal(bits(m[k]), bits(want[i])), (k, np.nonzero(bits(m[k]) != bits(want[i])))
        assert np.array_equal(bits(m[k].astype(np.float32)), bits(want[i].astype(np.float32)))
    assert np.isinf(want[:, 40]).all() and np.isinf(want[3, 41]) and np.isfinite(want[:3, 41]).all()


@pytest.mark.parametrize("case", ["fold_a", "fold_b"])
def test_select_keep_equals_the_reference(gold, case):
    from omniisaacgymenvs_loop_amd.scenario import select_keep
    p = json.loads(str(gold["fold_params"]))
    rows = json.loads(str(gold[f"{case}_select_rows"]))
    keep, final, summary = select_keep(rows, p["n_keep"], p["n_final"], p["easy_steps_max"], p["easy_margin_min"])
    assert keep.dtype == np.int64 and np.array_equal(keep, gold[f"{case}_keep_idx"])
    assert np.array_equal(final, gold[f"{case}_final_idx"])
    assert summary == json.loads(str(gold[f"{case}_select_summary"]))
    assert select_keep([], 1, 1, 80, 0.8)[2] == {"n": 0}


def test_reference_table_loads_without_pickle(gold):
    from omniisaacgymenvs_loop_amd.scenario import load_table
    with np.load(PRE20, allow_pickle=True) as ref:
        assert ref["obstacles_hash"].dtype == object   # the file is the reference's: this key needs pickle
    t = load_table(PRE20)
    assert [str(h) for h in t["obstacles_hash"]] == [str(h) for h in gold["pre_obstacles_hash"]]
    assert t["obstacles_hash"].dtype.kind == "U"
    for k in ARRAYS:
        assert np.array_equal(bits(t[k]), bits(gold[f"pre_{k}"]))
    for k in METRICS:
        assert t[k].dtype == np.float32 and np.array_equal(bits(t[k]), bits(gold[f"pre_{k}"].astype(np.float32)))
    assert np.array_equal(t["source_candidate_id"], gold["pre_source_candidate_id"])
    assert json.loads(t["meta"])["sampling"]["quant_m"] == 0.05


def test_table_round_trip_and_refusals(tmp_path, cands):
    from omniisaacgymenvs_loop_amd.scenario import SamplingParams, load_table, save_table, table_of
    c, d = cands
    t = table_of(c, np.array([5, 2, 9]), {"sampling": {"quant_m": 0.05}}, extra={"source_candidate_id": np.array([5, 2, 9])})
    path = str(tmp_path / "t.npz")
    save_table(path, t)
    with np.load(path, allow_pickle=False) as raw:   # nothing in our files needs pickle
        assert raw["obstacles_hash"].dtype.kind == "U" and set(raw.files) == set(t)
    with np.load(path, allow_pickle=True) as raw:    # the reference's reader takes it as well
        assert [str(h) for h in raw["obstacles_hash"]] == [str(h) for h in t["obstacles_hash"]]
    back = load_table(path)
    assert set(back) == set(t)
    for k, v in t.items():
        assert np.array_equal(np.asarray(back[k]), np.asarray(v)), k
    assert np.array_equal(back["scenario_id"], [0, 1, 2])
    bad = dict(t, obstacles_xy=t["obstacles_xy"][:, :8])
    with pytest.raises(ValueError, match="big = 16"):
        save_table(path, bad)
    with pytest.raises(ValueError, match="big"):
        SamplingParams(big=8).check()


def test_subset_follows_save_subset_npz(gold):
    from omniisaacgymenvs_loop_amd.scenario import load_table, subset
    t = load_table(PRE20)
    sub = subset(t, gold["sub_keep_idx"], json.loads(str(gold["sub_extra_meta"])))
    keys = {k[4:] for k in gold if k.startswith("sub_")} - {"keep_idx", "extra_meta"}
    assert keys == set(sub)
    for k in keys - {"meta", "obstacles_hash"}:
        want = gold[f"sub_{k}"]
        assert sub[k].dtype == want.dtype and np.array_equal(bits(sub[k]), bits(want)), k
    assert [str(h) for h in sub["obstacles_hash"]] == [str(h) for h in gold["sub_obstacles_hash"]]
    assert json.loads(sub["meta"]) == json.loads(str(gold["sub_meta"]))
    assert np.array_equal(sub["source_preselect_id"], gold["sub_keep_idx"])
    assert np.array_equal(sub["scenario_id"], np.arange(4)) and "teacher_filter" in json.loads(sub["meta"])


def test_to_scene_arrays_feeds_pack_scenes():
    from omniisaacgymenvs_loop_amd._abi import DEFINES as D
    from omniisaacgymenvs_loop_amd.scenario import load_table, to_scene_arrays, to_scene_rows
    from omniisaacgymenvs_loop_amd.tasks.scene_replay import pack_scenes
    t = load_table(PRE20)
    a = to_scene_arrays(t)
    rows = pack_scenes(a)
    assert rows.shape == (20, D["USV_SCENE_STRIDE"]) and rows.dtype == np.float32
    assert np.array_equal(rows, to_scene_rows(t))
    assert np.array_equal(rows[:, D["USV_SC_OBST"]:D["USV_SC_OBST"] + 32], t["obstacles_xy"].reshape(20, 32))
    assert np.array_equal(rows[:, D["USV_SC_START"]:D["USV_SC_START"] + 2], t["spawn_root_pos"][:, :2])
    assert np.array_equal(rows[:, D["USV_SC_GOAL"]:D["USV_SC_GOAL"] + 2], t["target_pos"][:, :2])
    assert np.array_equal(rows[:, D["USV_SC_VEL"]:D["USV_SC_VEL"] + 2], t["init_root_vel_xy"])
    q = t["spawn_root_rot"].astype(np.float64)
    yaw = np.array([np.float32(2.0 * np.arctan2(z, w)) for w, z in zip(q[:, 0], q[:, 3])])
    assert np.array_equal(bits(rows[:, D["USV_SC_YAW"]]), bits(yaw)) and (yaw >= 0).all() and (yaw <= 3.1416).all()
    assert (a["obstacles_count"] == 16).all()
    limbo = t["obstacles_xy"] == 999.0   # limbo entries stay (999, 999) in the rows
    assert np.array_equal(rows[:, :32].reshape(20, 16, 2) == 999.0, limbo)
    assert (rows[:, D["USV_SC_GOAL"] + 2:] == 0).all()


def test_scenario_table_script_writes_the_reference_tables(gold, tmp_path):
    from omniisaacgymenvs_loop_amd.scenario import load_table
    from omniisaacgymenvs_loop_amd.scripts import scenario_table
    out = str(tmp_path / "scenarios")
    files = scenario_table.main(["--n-candidates", "40", "--n-preselect", "20", "--n-selected", "10", "--seed", "0",
                                 "--save-candidates", "--out-dir", out])
    assert files == ["candidates_40_unique.npz", "preselect_20.npz", "selected_10.npz", "scenario_table.meta.json"]
    assert sorted(os.listdir(out)) == sorted(files)
    for name, prefix in (("candidates_40_unique.npz", "cand"), ("preselect_20.npz", "pre"), ("selected_10.npz", "sel")):
        t = load_table(os.path.join(out, name))
        for k in ARRAYS:
            assert np.array_equal(bits(t[k]), bits(gold[f"{prefix}_{k}"])), (name, k)
        for k in METRICS:
            assert np.array_equal(bits(t[k]), bits(gold[f"{prefix}_{k}"].astype(np.float32))), (name, k)
        assert [str(h) for h in t["obstacles_hash"]] == [str(h) for h in gold[f"{prefix}_obstacles_hash"]]
        assert np.array_equal(t["scenario_id"], gold[f"{prefix}_scenario_id"])
    pre = load_table(os.path.join(out, "preselect_20.npz"))
    assert np.array_equal(pre["source_candidate_id"], gold["pre_source_candidate_id"])
    meta = json.load(open(os.path.join(out, "scenario_table.meta.json")))
    assert meta["summary"]["preselect"] == json.loads(str(gold["pre_summary"])) and meta["sampler"] == "numpy"
    assert meta["summary"]["selected"] == json.loads(str(gold["sel_summary"])) and json.loads(pre["meta"]) == meta


def test_philox_host_sampler_obeys_the_law():
    """The host restatement of the device sampler: deterministic, independent of the range it is asked for, every
    obstacle in the box and clear of spawn and target or exactly in limbo."""
    from omniisaacgymenvs_loop_amd._abi import DEFINES as D
    from omniisaacgymenvs_loop_amd.scenario import SamplingParams, philox_host
    p = SamplingParams(max_iterations=1, min_dist_safe=12.0, init_vel_mode="rand")
    rows, quat = philox_host(0, 67, 3, p)
    part, qpart = philox_host(40, 27, 3, p)
    assert np.array_equal(bits(rows[40:]), bits(part)) and np.array_equal(bits(quat[40:]), bits(qpart))
    obs = rows[:, :32].reshape(67, 16, 2)
    s, g = rows[:, None, D["USV_SC_START"]:D["USV_SC_START"] + 2], rows[:, None, D["USV_SC_GOAL"]:D["USV_SC_GOAL"] + 2]
    limbo = (obs == 999.0).all(2)
    assert limbo.any() and not limbo.all() and ((obs == 999.0).any(2) == limbo).all()
    f = np.float32
    for ref in (s, g):
        dx, dy = obs[..., 0] - ref[..., 0], obs[..., 1] - ref[..., 1]
        assert (np.sqrt(dx * dx + dy * dy)[~limbo] >= f(12.0)).all()
    assert (np.abs(obs - g)[~limbo] <= f(15.0) * (1 + 2 ** -23)).all()
    assert (np.abs(rows[:, D["USV_SC_VEL"]:D["USV_SC_VEL"] + 2]) <= 1.5).all() and rows[:, D["USV_SC_VEL"]].std() > 0.1
    r = np.hypot(rows[:, D["USV_SC_START"]], rows[:, D["USV_SC_START"] + 1])
    assert (r >= 0.5 - 1e-6).all() and (r <= 5.0 + 1e-6).all() and (np.abs(rows[:, D["USV_SC_GOAL"]]) <= 5.0).all()
    assert np.allclose(quat[:, 0] ** 2 + quat[:, 3] ** 2, 1.0, atol=1e-6) and (quat[:, 1:3] == 0).all()
    assert np.allclose(2.0 * np.arctan2(quat[:, 3], quat[:, 0]), rows[:, D["USV_SC_YAW"]], atol=1e-6)


def test_entry_points_check_their_arguments_without_a_device():
    """Status 1 for a NULL or out-of-range argument, 2 for an unsupported size: every check precedes device work
    (as test_stale_root_needs_its_rows: there is no GPU here)."""
    from omniisaacgymenvs_loop_amd import _capi
    from omniisaacgymenvs_loop_amd._abi import DEFINES as D
    from omniisaacgymenvs_loop_amd._abi import LzCfg, UsvEval
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libusv_hip.so not built (run __graft_entry__.build())")
    lib = _capi.lib()
    buf = ctypes.create_string_buffer(1 << 12)
    p = ctypes.addressof(buf)   # host scratch: never dereferenced
    gen = lambda count=4, first=0, iters=20, vel=0, rows=p, quat=p: lib.usv_scn_generate(
        7, first, count, 5.0, 0.5, 5.0, 15.0, 2.0, iters, vel, rows, quat, None)
    assert gen(rows=None) == 1 and gen(quat=None) == 1 and gen(count=0) == 1 and gen(first=-1) == 1
    assert gen(count=D["USV_SCN_MAX_COUNT"] + 1) == 2 and gen(iters=-1) == 2
    assert gen(iters=D["USV_SCN_MAX_ITERS"] + 1) == 2 and gen(vel=2) == 2
    met = lambda rows=p, s=4, out=p: lib.usv_scn_metrics(rows, s, 0.5, 100.0, out, None)
    assert met(rows=None) == 1 and met(out=None) == 1 and met(s=0) == 1 and met(s=D["USV_SCN_MAX_COUNT"] + 1) == 2
    ev = UsvEval()
    ev.acc = ev.episodes = ev.ep_count = p
    ev.max_episodes = 3
    fold = lambda e=ev, n=8, s=7, r=3, k=3, out=p: lib.usv_scn_fold(
        _capi.byref(e) if e is not None else None, n, s, r, k, 0.5, 80, 0.8, 200, out, None)
    assert fold(e=None) == 1 and fold(out=None) == 1 and fold(n=0) == 1 and fold(s=0) == 1 and fold(r=0) == 1
    assert fold(k=0) == 1
    empty = UsvEval()
    assert fold(e=empty) == 1
    assert fold(k=2) == 2 and fold(k=4) == 2            # K is ceil(S R / n)
    assert fold(n=4, k=6) == 2                           # past the evaluator's max_episodes
    assert fold(s=D["USV_SCN_MAX_COUNT"] + 1, k=1) == 2
    cfg = LzCfg()
    cfg.n_envs, cfg.horizon, cfg.obs_dim, cfg.mini_batches, cfg.epochs = 70, 1, 33, 1, 1
    play = lambda c=cfg, par=p, obs=p, act=p: lib.lz_play(_capi.byref(c) if c is not None else None, par, obs, act, None)
    assert play(c=None) == 1 and play(par=None) == 1 and play(obs=None) == 1 and play(act=None) == 1
    bad = LzCfg()
    bad.n_envs, bad.horizon, bad.obs_dim, bad.mini_batches, bad.epochs = 70, 1, 40, 1, 1
    assert play(c=bad) == 1
