"""The teacher-vs-student comparison on the host: the restatements of the compare tool's privileged-tail overrides
(omniisaacgymenvs_loop_amd.scenario.compare) against the fixture the reference's own functions produced
(tests/golden/compare_golden.npz), the numpy restatement of the paired fold against a hand-worked table, the totals
and the pairing flag."""
import math

import numpy as np
import pytest

from omniisaacgymenvs_loop_amd._abi import DEFINES as D
from omniisaacgymenvs_loop_amd.scenario import compare as C
from tests import compare_restate as CR


@pytest.fixture(scope="module")
def fx(golden):
    return golden("compare_golden.npz")


def test_fixture_covers_every_mode(fx):
    cases = [CR.row_to_case(r) for r in fx["case_values"]]
    combos = {(p["priv_mode"], p["couple_drag"], p["mass_relative"], p["com_scaled"]) for p in cases
              if p["priv_dim"] == 8 and p["com_mode"] == 1}
    assert len(combos) == 3 * 2 * 2 * 2
    assert any(p["priv_dim"] == 4 for p in cases) and any(p["com_mode"] == 0 for p in cases)
    assert [CR.case_to_row(p).tolist() for p in CR.all_cases()] == fx["case_values"].tolist()


def test_base_const_tail_equals_reference(fx):
    for i, row in enumerate(fx["case_values"]):
        p = CR.row_to_case(row)
        got = C.base_const_tail_host(p)
        assert got.dtype == np.float32 and got.shape == (p["priv_dim"],)
        np.testing.assert_array_equal(got, fx["const_tail"][i][:p["priv_dim"]], err_msg=f"case {i} {p}")


def test_wrong_random_tail_equals_reference(fx):
    for i, row in enumerate(fx["case_values"]):
        p = CR.row_to_case(row)
        u = fx["wrong_draws"][i]                                    # [seed][4]
        got = C.wrong_random_tail_host(p, u[:, 0], u[:, 1:4])
        assert got.dtype == np.float32 and got.shape == (u.shape[0], p["priv_dim"])
        np.testing.assert_array_equal(got, fx["wrong_tail"][i][:, :p["priv_dim"]], err_msg=f"case {i} {p}")


def test_wrong_random_tail_depends_on_the_draws(fx):
    p = CR.row_to_case(fx["case_values"][0])
    a = C.wrong_random_tail_host(p, [0.25], [[0.1, 0.2, 0.3]])
    b = C.wrong_random_tail_host(p, [0.75], [[0.1, 0.2, 0.3]])
    assert a[0, 0] != b[0, 0] and np.array_equal(a[0, 1:4], b[0, 1:4])


def test_legacy_disk_com_is_refused(fx):
    p = CR.row_to_case(fx["case_values"][0])
    p.update(com_mode=2, com_legacy_r=0.1)
    with pytest.raises(NotImplementedError):
        C.wrong_random_tail_host(p, [0.5], [[0.5, 0.5, 0.5]])


def test_override_replaces_only_the_tail(fx):
    obs = fx["override_obs_in"]
    for md in (8, 4):
        want = fx[f"override_obs_out{md}"]
        got = obs.copy()
        got[:, -md:] = fx["const_tail"][0][:md]
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(want[:, :-md], obs[:, :-md])


def test_wrong_random_words_are_a_pure_function_of_seed_env_episode():
    a = C.wrong_random_words(7, 5, np.zeros(5, np.int32))
    b = C.wrong_random_words(7, 5, np.array([0, 1, 0, 0, 0], np.int32))
    assert a.shape == (5, 4) and (a >= 0).all() and (a < 1).all()
    assert np.array_equal(a[[0, 2, 3, 4]], b[[0, 2, 3, 4]]) and not np.array_equal(a[1], b[1])
    assert not np.array_equal(a, C.wrong_random_words(8, 5, np.zeros(5, np.int32)))
    assert len({tuple(r) for r in a}) == 5


def test_paired_fold_against_a_hand_worked_table():
    """S = 2 scenarios, R = 2 rollouts, n = 4, K = 1; worked by hand below."""
    G, CO, OB, OT = CR.GOAL, CR.COLL, CR.OOB, CR.OTHER
    thr = 1.2
    #       reason steps return dist min_obs
    a = {0: (G, 10, 5.0, 0.1, 2.0), 1: (CO, 4, -2.0, 3.0, 1.0), 2: (G, 20, 6.0, 0.2, np.inf), 3: (OT, 50, 1.0, 4.0, 3.0)}
    b = {0: (G, 14, 4.0, 0.3, 1.5), 1: (G, 30, 3.0, 0.1, 2.5), 2: (OB, 9, -1.0, 9.0, 2.0)}   # row 3: no record in b
    (ta, ca), (tb, cb) = CR.make_table(4, 1, a), CR.make_table(4, 1, b)
    out = CR.cmp_fold_host(ta, ca, tb, cb, 4, 2, 2, 1, thr)
    row = lambda k: out[D[f"USV_CMP_{k}"]].tolist()   # noqa: E731
    assert row("PAIRS") == [2, 1] and row("BOTH_SUCC") == [1, 0] and row("ONLY_A") == [0, 1]
    assert row("ONLY_B") == [1, 0] and row("NEITHER") == [0, 0]
    assert row("COLL_A") == [1, 0] and row("COLL_B") == [0, 0] and row("OOB_A") == [0, 0] and row("OOB_B") == [0, 1]
    assert out[D["USV_CMP_D_STEPS"], 0] == 4.0 and math.isnan(out[D["USV_CMP_D_STEPS"], 1])
    assert row("D_RETURN") == [((4.0 - 5.0) + (3.0 - -2.0)) / 2, -7.0]
    assert row("D_FINAL_DIST") == [((0.3 - 0.1) + (0.1 - 3.0)) / 2, 9.0 - 0.2]
    assert out[D["USV_CMP_D_MIN_MARGIN"], 0] == (((1.5 - thr) - (2.0 - thr)) + ((2.5 - thr) - (1.0 - thr))) / 2
    assert math.isnan(out[D["USV_CMP_D_MIN_MARGIN"], 1])   # a's min_obs is infinite in the only pair
    t = C.cmp_totals(C.cmp_to_dict(out))
    assert (t["pairs"], t["only_a"], t["only_b"], t["both_success"]) == (3, 1, 1, 1)
    sd = t["success_diff"]
    assert sd["mean"] == 0.0 and sd["std"] == pytest.approx(math.sqrt(2 / 3))
    assert sd["ci95_hi"] == pytest.approx(1.96 * math.sqrt(2 / 3) / math.sqrt(3)) and sd["ci95_lo"] == -sd["ci95_hi"]
    assert t["d_steps"] == 4.0 and t["d_return"] == pytest.approx((2 * 2.0 + 1 * -7.0) / 3)


def test_totals_interval_from_the_counts():
    cmp = {k: np.zeros(2, np.int64) for k in C.CMP_INT_KEYS}
    cmp.update(pairs=np.array([60, 40]), only_a=np.array([3, 2]), only_b=np.array([10, 5]),
               both_success=np.array([40, 30]), d_steps=np.array([2.0, np.nan]), d_return=np.array([1.0, 3.0]),
               d_final_dist=np.array([0.0, 0.0]), d_min_margin=np.array([np.nan, np.nan]))
    t = C.cmp_totals(cmp)
    mean = (15 - 5) / 100
    std = math.sqrt(20 / 100 - mean * mean)
    assert t["success_diff"]["mean"] == pytest.approx(mean) and t["success_diff"]["std"] == pytest.approx(std)
    assert t["success_diff"]["ci95_lo"] == pytest.approx(mean - 1.96 * std / 10)
    assert t["d_steps"] == 2.0 and t["d_return"] == pytest.approx(1.8) and math.isnan(t["d_min_margin"])
    empty = C.cmp_totals({k: np.zeros(1) for k in C.CMP_KEYS})
    assert empty["pairs"] == 0 and math.isnan(empty["success_diff"]["mean"])


def test_more_than_one_episode_per_env_clears_paired_draws():
    assert C.pairing_info(64, 20, 3) == {"episodes_per_env": 1, "paired_draws": True}
    assert C.pairing_info(64, 64, 1)["paired_draws"] is True
    two = C.pairing_info(64, 20, 4)
    assert two["episodes_per_env"] == 2 and two["paired_draws"] is False


def test_arm_names_are_checked():
    with pytest.raises(ValueError):
        C.arm_factories(["teacher", "nobody"], lambda r: None, None)
    with pytest.raises(ValueError):
        C.arm_factories(["student"], lambda r: None, None)
    assert list(C.arm_factories(["teacher", "teacher_wrong_tail"], lambda r: None, None)) == ["teacher", "teacher_wrong_tail"]
