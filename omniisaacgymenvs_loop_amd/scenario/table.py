"""Scenario tables: the NPZ format of the reference's scripts/build_usv_scenario_table.py (_save_npz :518-550)
and the subset tables of scripts/teacher_filter_scenario_table.py (_save_subset_npz :205-242).

A table is a dict of numpy arrays with S scenarios on the first axis (PER_SCENARIO + the optional source ids)
and `meta`, a JSON string.  Files are read with allow_pickle=False.  The reference stores `obstacles_hash` as an
object array, which needs pickle: that key is never touched in such a file, the hashes are recomputed from the
obstacles instead (obstacles_hash :115-121; quant_m from the meta).  Tables written here hold it as a
fixed-width unicode array, which the reference's np.load(allow_pickle=True) reads as well."""
from __future__ import annotations

import hashlib
import json
import os
from typing import Any, Dict, Optional

import numpy as np

from .._abi import DEFINES

BIG = DEFINES["USV_NOBST"]
LIMBO = 999.0
DEFAULT_QUANT_M = 0.05
F32_KEYS = ("obstacles_xy", "spawn_root_pos", "spawn_root_rot", "target_pos", "target_rot", "init_root_vel_xy",
            "d_spawn", "d_goal", "d_corr", "d_oo", "density_score")
PER_SCENARIO = ("scenario_id",) + F32_KEYS[:6] + ("obstacles_hash",) + F32_KEYS[6:]
OPTIONAL_IDS = ("source_candidate_id", "source_preselect_id")
SHAPES = {"obstacles_xy": (BIG, 2), "spawn_root_pos": (3,), "spawn_root_rot": (4,), "target_pos": (3,),
          "target_rot": (4,), "init_root_vel_xy": (2,)}


def obstacles_hash(obstacles_xy: np.ndarray, quant_m: float) -> str:
    """sha1 of the rounded int32 quantisation plus the shape / quant suffix (_obstacles_hash :115-121)."""
    q = np.round(obstacles_xy / float(quant_m)).astype(np.int32)
    return hashlib.sha1(q.tobytes() + (f"|shape={q.shape}|quant={quant_m}").encode("utf-8")).hexdigest()


def hashes_of(obstacles_xy: np.ndarray, quant_m: float) -> np.ndarray:
    obs = np.asarray(obstacles_xy, np.float32)
    return np.array([obstacles_hash(o, quant_m) for o in obs], dtype="U40")


def meta_of(table: Dict[str, Any]) -> Dict[str, Any]:
    try:
        return dict(json.loads(str(table.get("meta", "") or "{}")))
    except Exception:
        return {}


def quant_of(meta: Dict[str, Any]) -> float:
    try:
        return float(meta["sampling"]["quant_m"])
    except Exception:
        return DEFAULT_QUANT_M


def check_table(table: Dict[str, Any]) -> int:
    """Shapes and dtypes of a table; returns S.  A table whose obstacle lists are not 16 long is refused."""
    missing = [k for k in PER_SCENARIO if k not in table]
    if missing:
        raise KeyError(f"scenario table missing keys={missing}; found={sorted(table)}")
    s = int(np.asarray(table["scenario_id"]).shape[0])
    obs = np.asarray(table["obstacles_xy"])
    if obs.ndim != 3 or obs.shape[1] != BIG or obs.shape[2] != 2:
        raise ValueError(f"obstacles_xy must be [S][{BIG}][2] (big = {BIG} only), got {obs.shape}")
    for k in PER_SCENARIO + tuple(i for i in OPTIONAL_IDS if i in table):
        a = np.asarray(table[k])
        if a.shape != (s,) + SHAPES.get(k, ()):
            raise ValueError(f"{k} must be {(s,) + SHAPES.get(k, ())}, got {a.shape}")
    return s


def make_table(scenario_id, obstacles_xy, spawn_root_pos, spawn_root_rot, target_pos, target_rot, init_root_vel_xy,
               metrics: Dict[str, np.ndarray], meta: Dict[str, Any], hashes: Optional[np.ndarray] = None,
               extra: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, Any]:
    """A table from its arrays (_save_npz's payload :527-545); metrics: the five d_* / density_score arrays."""
    t: Dict[str, Any] = {
        "scenario_id": np.asarray(scenario_id, np.int64),
        "obstacles_xy": np.asarray(obstacles_xy, np.float32), "spawn_root_pos": np.asarray(spawn_root_pos, np.float32),
        "spawn_root_rot": np.asarray(spawn_root_rot, np.float32), "target_pos": np.asarray(target_pos, np.float32),
        "target_rot": np.asarray(target_rot, np.float32), "init_root_vel_xy": np.asarray(init_root_vel_xy, np.float32)}
    t["obstacles_hash"] = (np.asarray(hashes, dtype="U40") if hashes is not None
                           else hashes_of(t["obstacles_xy"], quant_of(meta)))
    for k in ("d_spawn", "d_goal", "d_corr", "d_oo", "density_score"):
        t[k] = np.asarray(metrics[k], np.float32)
    for k, v in (extra or {}).items():
        t[str(k)] = np.asarray(v)
    t["meta"] = json.dumps(meta, ensure_ascii=False)
    check_table(t)
    return t


def _npy_dtype(npz, key: str) -> np.dtype:
    """The dtype of one member of an open npz from its header alone (the data is not read)."""
    fmt = np.lib.format
    with npz.zip.open(key + ".npy") as f:
        version = fmt.read_magic(f)
        header = fmt.read_array_header_1_0(f) if version == (1, 0) else fmt.read_array_header_2_0(f)
    return header[2]


def load_table(path: str) -> Dict[str, Any]:
    """Read a table without pickle; an object-dtype obstacles_hash (a reference-written file) is recomputed."""
    if not os.path.exists(path):
        raise FileNotFoundError(f"scenario table not found: {path}")
    t: Dict[str, Any] = {}
    with np.load(path, allow_pickle=False) as npz:
        files = list(npz.files)
        for k in files:
            if k == "obstacles_hash":
                continue
            t[k] = np.array(npz[k])
        t["meta"] = str(t["meta"].tolist()) if "meta" in t else "{}"
        stored = None
        if "obstacles_hash" in files and _npy_dtype(npz, "obstacles_hash").kind == "U":
            stored = np.array(npz["obstacles_hash"])
    if "obstacles_xy" not in t:
        raise KeyError(f"scenario table missing obstacles_xy; found={files}")
    t["obstacles_hash"] = (stored.astype("U40") if stored is not None and stored.dtype.kind == "U"
                           else hashes_of(t["obstacles_xy"], quant_of(meta_of(t))))
    for k in F32_KEYS:
        if k in t:
            t[k] = np.asarray(t[k], np.float32)
    check_table(t)
    return t


def save_table(path: str, table: Dict[str, Any]) -> None:
    check_table(table)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    payload = {k: v for k, v in table.items() if k != "meta"}
    payload["obstacles_hash"] = np.asarray(table["obstacles_hash"], dtype="U40")
    np.savez_compressed(path, **payload, meta=str(table.get("meta", "{}")))


def subset(table: Dict[str, Any], keep_idx, extra_meta: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
    """_save_subset_npz (:205-242): every per-scenario array sliced, source_preselect_id = keep_idx, scenario_id
    re-indexed, meta["teacher_filter"] = extra_meta."""
    keep = np.asarray(keep_idx, np.int64).reshape(-1)
    s = int(np.asarray(table["scenario_id"]).shape[0])
    out: Dict[str, Any] = {}
    for k, v in table.items():
        if k == "meta":
            continue
        out[k] = v[keep] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == s else v
    out["source_preselect_id"] = keep.astype(np.int64)
    out["scenario_id"] = np.arange(keep.size, dtype=np.int64)
    meta = meta_of(table)
    meta["teacher_filter"] = dict(extra_meta or {})
    out["meta"] = json.dumps(meta, ensure_ascii=False)
    return out


def to_scene_arrays(table: Dict[str, Any]) -> Dict[str, np.ndarray]:
    """The six arrays tasks.scene_replay.pack_scenes takes.  The yaw is that of the yaw-only quaternion
    (w, 0, 0, z), 2 atan2(z, w) in double, rounded once; limbo obstacles stay (999, 999) with a count of 16, which
    is what the reference's ScenarioReplayer (:245-332) hands to the field."""
    s = check_table(table)
    rot = np.asarray(table["spawn_root_rot"], np.float64)
    return {"obstacles_xy": np.asarray(table["obstacles_xy"], np.float32),
            "obstacles_count": np.full((s,), BIG, np.int32),
            "start_pos": np.asarray(table["spawn_root_pos"], np.float32)[:, :2],
            "start_yaw": (2.0 * np.arctan2(rot[:, 3], rot[:, 0])).astype(np.float32),
            "start_vel": np.asarray(table["init_root_vel_xy"], np.float32),
            "goal_pos": np.asarray(table["target_pos"], np.float32)[:, :2]}


def to_scene_rows(table: Dict[str, Any]) -> np.ndarray:
    """[S][USV_SCENE_STRIDE] float32 rows (USV_SC_* layout) of a table."""
    from ..tasks.scene_replay import pack_scenes
    return pack_scenes(to_scene_arrays(table))
