"""The potential field's statistics split on the device: cost-only statistics and far flags from the sweep kernels'
registers, near-cell statistics over the obstacles' windows (k_field_near), the two-row fold (k_field_batch).

Every scene of tests/field_split_scenes.py, in batches of 1, 5 and 17 slots in shuffled slot order (partial rows
are indexed by slot, not by env), through each sweep kernel and launch function: usv_potential_field with
USV_FIELD_PACK = 0 / 1 and usv_field_stage(2) with USV_FIELD_HALF = 0 / 1.  The materialised field is the oracle's
bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle as O
from omniisaacgymenvs_loop_amd.tasks.usv_config import load_yaml
from tests import field_split_scenes as S
from tests.test_oracle_golden import TEST_YAML

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROUTES = {"field_plain": ("0", "0", False), "field_pack": ("1", "0", False),
          "stage_pack": ("0", "0", True), "stage_half": ("0", "1", True)}
BATCHES = (1, 5, 17)


@pytest.fixture(scope="module")
def task():
    from omniisaacgymenvs_loop_amd.tasks.usv_virtual import USVVirtual
    return USVVirtual(load_yaml(TEST_YAML), num_envs=64, device=DEV, seed=7)


_REF = {}


def _reference(cfg, name, k):
    """The batch and the oracle's field of it, computed once and shared by the four routes."""
    if (name, k) not in _REF:
        obst, tgt, ids = S.batch(name, k, seed=100 * S.NAMES.index(name) + k)
        ref, cost = O.potential_field(cfg, obst, tgt, want_cost=True)
        for a in (obst, tgt, ids, ref, cost):
            a.setflags(write=False)
        _REF[(name, k)] = (obst, tgt, ids, ref, cost)
    return _REF[(name, k)]


def _run_field(task, ids, obst, tgt, stage):
    """The fields of the reset envs `ids` (obstacles / targets given) by usv_potential_field, or with stage=True
    by usv_field_stage(2) (test_env_gpu.py's helper)."""
    from omniisaacgymenvs_loop_amd import _capi
    k = len(ids)
    ids_t = torch.tensor(ids, device=DEV, dtype=torch.int32)
    task.reset_ids[:k] = ids_t
    task.ctl.zero_()
    task.ctl[0] = k
    task.fscratch.zero_()
    task.slot_stats.fill_(float("nan"))          # no statistic may come from an earlier batch's rows
    task.obst[:, ids_t.long()] = torch.tensor(obst.reshape(k, 32).T.copy(), device=DEV)
    task.field_old_tgt[:, ids_t.long()] = torch.tensor(tgt.T.copy(), device=DEV)
    if stage:
        _capi.call("usv_field_stage", _capi.byref(task.cfg), _capi.byref(task._bufs), 2, _capi.stream_ptr())
    else:
        _capi.call("usv_potential_field", _capi.byref(task.cfg), _capi.byref(task._bufs), _capi.stream_ptr())
    torch.cuda.synchronize()
    return task.field_rowmajor(ids_t.long()).cpu().numpy()


@pytest.mark.parametrize("name", S.NAMES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_split_field_matches_oracle(task, route, name, monkeypatch):
    from omniisaacgymenvs_loop_amd._abi import DEFINES
    pack, half, stage = ROUTES[route]
    monkeypatch.setenv("USV_FIELD_PACK", pack)
    monkeypatch.setenv("USV_FIELD_HALF", half)
    for k in BATCHES:
        obst, tgt, ids, ref, cost = _reference(task.cfg, name, k)
        f = _run_field(task, ids, obst, tgt, stage)
        np.testing.assert_array_equal(f, ref, err_msg=f"{name} k={k} {route}")
        # the envs that took the reference's 225 literal sweeps: those with a finite cost above the certificate's
        n_exact = int(sum(c[np.isfinite(c)].max(initial=0.0) > 224.0 for c in cost))
        assert int(task.ctl[DEFINES["USV_CTL_FIELD_EXACT"]].item()) == n_exact
        if name == "detour":
            assert n_exact == 1
