"""What the comparison tests share: the cases of tests/golden/compare_golden.npz as parameter dicts for the host
restatements of the privileged-tail overrides (omniisaacgymenvs_loop_amd.scenario.compare), and a numpy restatement
of the paired per-scenario fold (usv_cmp_fold, include/usv_hip.h) with hand-built evaluator tables."""
from __future__ import annotations

import itertools

import numpy as np

from omniisaacgymenvs_loop_amd._abi import DEFINES

D = DEFINES
PRIV_MODES = ("raw", "centered", "minmax")
SCALARS = ("priv_dim", "priv_mode", "nominal", "mass_relative", "com_scaled", "com_mode", "com_legacy_r", "min_mass",
           "max_mass", "base_mass", "couple_drag", "couple_thr", "couple_kiz", "k_drag_min", "k_drag_max", "thr_rand",
           "k_iz_min", "k_iz_max")
VECTORS = ("com_scale", "base_com", "com_disp")
BOOLS = ("mass_relative", "com_scaled", "couple_drag", "couple_thr", "couple_kiz")


def case_params(priv_mode="raw", coupled=False, mass_relative=False, com_scaled=False, priv_dim=8, com_mode=1,
                reversed_mass=False):
    """Values that float32 does not hold exactly, so a restatement in the wrong precision shows."""
    lo, hi = (30.1, 42.7) if not reversed_mass else (42.7, 30.1)
    return {"priv_dim": priv_dim, "priv_mode": priv_mode, "nominal": 1.0, "mass_relative": mass_relative,
            "com_scaled": com_scaled, "com_scale": [1.35, 0.98, 1.0], "com_mode": com_mode, "com_legacy_r": 0.0,
            "base_com": [0.01, -0.02, 0.1], "com_disp": [0.05, 0.03, 0.02], "min_mass": lo, "max_mass": hi,
            "base_mass": 35.3, "couple_drag": coupled, "couple_thr": coupled, "couple_kiz": coupled,
            "k_drag_min": 0.8, "k_drag_max": 1.4, "thr_rand": 0.3, "k_iz_min": 0.9, "k_iz_max": 1.3}


def all_cases():
    cases = [case_params(pm, cp, mr, cs) for pm, cp, mr, cs in
             itertools.product(PRIV_MODES, (False, True), (False, True), (False, True))]
    cases.append(case_params("centered", True, True, True, priv_dim=4))
    cases.append(case_params("minmax", True, False, True, com_mode=0))
    cases.append(case_params("centered", True, True, False, reversed_mass=True))
    return cases


def case_to_row(p) -> np.ndarray:
    vals = [float(PRIV_MODES.index(p[k])) if k == "priv_mode" else float(p[k]) for k in SCALARS]
    for k in VECTORS:
        vals += [float(v) for v in p[k]]
    return np.asarray(vals, np.float64)


def row_to_case(row) -> dict:
    p = {k: float(row[i]) for i, k in enumerate(SCALARS)}
    for j, k in enumerate(VECTORS):
        p[k] = [float(v) for v in row[len(SCALARS) + 3 * j:len(SCALARS) + 3 * j + 3]]
    for k in ("priv_dim", "com_mode"):
        p[k] = int(p[k])
    p["priv_mode"] = PRIV_MODES[int(p["priv_mode"])]
    for k in BOOLS:
        p[k] = bool(p[k])
    return p


# ------------------------------------------------------------------ the paired fold
GOAL, COLL, OOB, OTHER = (D["USV_EV_REASON_GOAL"], D["USV_EV_REASON_COLLISION"], D["USV_EV_REASON_OOB"],
                          D["USV_EV_REASON_OTHER"])


def make_table(n, K, records):
    """An evaluator table ([USV_EV_ROWS][K n] doubles, ep_count [n]) from {playlist row p: (reason, steps, return,
    final_dist, min_obs)}; env p // K gets its records in order (a missing record ends the env's list)."""
    tab = np.zeros((D["USV_EV_ROWS"], K * n), np.float64)
    cnt = np.zeros(n, np.int32)
    for p in sorted(records):
        e, k = p // K, p % K
        assert cnt[e] == k, "records of an env are filled in episode order"
        col = k * n + e
        reason, steps, ret, dist, mo = records[p]
        tab[D["USV_EV_REASON"], col], tab[D["USV_EV_LEN_STEPS"], col] = reason, steps
        tab[D["USV_EV_RETURN"], col], tab[D["USV_EV_DIST_TO_GOAL"], col] = ret, dist
        tab[D["USV_EV_MIN_OBS_EP"], col] = mo
        tab[D["USV_EV_SUCCESS"], col] = float(reason == GOAL)
        cnt[e] = k + 1
    return tab, cnt


def cmp_fold_host(tab_a, cnt_a, tab_b, cnt_b, n, S, R, K, thr) -> np.ndarray:
    """usv_cmp_fold in numpy: [USV_CMP_ROWS][S] doubles, sums in rollout order."""
    out = np.zeros((D["USV_CMP_ROWS"], S), np.float64)

    def rec(tab, cnt, p):
        e, k = p // K, p % K
        if k >= min(int(cnt[e]), K):
            return None
        col = k * n + e
        return tuple(tab[D[f"USV_EV_{r}"], col] for r in ("REASON", "LEN_STEPS", "RETURN", "DIST_TO_GOAL", "MIN_OBS_EP"))

    for s in range(S):
        c = {k: 0.0 for k in ("pairs", "both", "oa", "ob", "nei", "ca", "cb", "xa", "xb", "ns", "ds", "dr", "dd", "nm",
                              "dm")}
        for r in range(R):
            a, b = rec(tab_a, cnt_a, s * R + r), rec(tab_b, cnt_b, s * R + r)
            if a is None or b is None:
                continue
            sa, sb = a[0] == GOAL, b[0] == GOAL
            c["pairs"] += 1
            c["both"] += sa and sb
            c["oa"] += sa and not sb
            c["ob"] += sb and not sa
            c["nei"] += (not sa) and (not sb)
            c["ca"] += a[0] == COLL
            c["cb"] += b[0] == COLL
            c["xa"] += a[0] == OOB
            c["xb"] += b[0] == OOB
            if sa and sb:
                c["ns"] += 1
                c["ds"] += b[1] - a[1]
            c["dr"] += b[2] - a[2]
            c["dd"] += b[3] - a[3]
            if np.isfinite(a[4]) and np.isfinite(b[4]):
                c["nm"] += 1
                c["dm"] += (b[4] - thr) - (a[4] - thr)
        with np.errstate(invalid="ignore", divide="ignore"):
            vals = {"PAIRS": c["pairs"], "BOTH_SUCC": c["both"], "ONLY_A": c["oa"], "ONLY_B": c["ob"],
                    "NEITHER": c["nei"], "COLL_A": c["ca"], "COLL_B": c["cb"], "OOB_A": c["xa"], "OOB_B": c["xb"],
                    "D_STEPS": np.float64(c["ds"]) / np.float64(c["ns"]),
                    "D_RETURN": np.float64(c["dr"]) / np.float64(c["pairs"]),
                    "D_FINAL_DIST": np.float64(c["dd"]) / np.float64(c["pairs"]),
                    "D_MIN_MARGIN": np.float64(c["dm"]) / np.float64(c["nm"])}
        for k, v in vals.items():
            out[D[f"USV_CMP_{k}"], s] = v
    return out


def hand_tables(S, R, K, n, missing_in_b=()):
    """Two deterministic hand-built tables of a playlist with S R rows: every reason occurs, arm b differs from
    arm a in a known pattern; rows in missing_in_b have no record in b (and none after them in that env)."""
    ra, rb = {}, {}
    reasons = (GOAL, COLL, OOB, OTHER, GOAL, GOAL)
    for p in range(S * R):
        a_reason, b_reason = reasons[p % 6], reasons[(p * 5 + 1) % 6]
        ra[p] = (a_reason, 10.0 + p, 1.5 * p - 3.0, 0.25 + 0.125 * p, np.inf if p % 7 == 3 else 1.0 + 0.0625 * p)
        rb[p] = (b_reason, 12.0 + 2 * p, 1.25 * p - 1.0, 0.5 + 0.0625 * p, 1.5 + 0.03125 * p)
    dead = set()
    for p in missing_in_b:
        dead.update(q for q in range(p, (p // K) * K + K))
    for q in dead:
        rb.pop(q, None)
    return make_table(n, K, ra), make_table(n, K, rb)
