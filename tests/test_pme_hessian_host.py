"""AIMNet2Calculator.set_pme_hessian against the recording fake engine of tests/fake_engine.py, and the host side of the arming
(capacity policy, the symbols): with "analytic" the calculator sends ONE engine.hvp call with coulomb="pme", pme_tangent=True and
the accuracy, and no displaced copies; None (the default) and hvp_method = "fd" take differences of forces as before.  CPU only."""
from __future__ import annotations

import warnings

import numpy as np
import pytest
import torch

from aimnetcentral_amd import _lib, capacity
from fake_engine import FakeEngine, fake_calculator


class RecordingHvpEngine(FakeEngine):
    def hvp(self, coord, numbers, mol_idx, charge, vectors, **kw):
        self.hvp_calls.append(dict(kw, K=int(vectors.shape[0]), n=int(coord.shape[0])))
        return {"hv": torch.zeros_like(vectors)}


@pytest.fixture()
def calc(monkeypatch):
    return fake_calculator(monkeypatch, RecordingHvpEngine)


CELL = dict(coord=[[0.0, 0.0, 0.1173], [0.0, 0.7572, -0.4692], [0.0, -0.7572, -0.4692]], numbers=[8, 1, 1], charge=0.0,
            cell=np.eye(3, dtype=np.float32) * 9.0)
V = np.arange(18, dtype=np.float32).reshape(2, 3, 3)


def _set(calc, method, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        calc.set_lrcoulomb_method(method, **kw)


def test_armed_pme_takes_one_call_of_the_sweep(calc):
    _set(calc, "pme", ewald_accuracy=3e-7)
    calc.set_pme_hessian("analytic")
    n_eval = len(calc.engine.calls)
    hv = calc.hessian_vector_product(CELL, V)
    assert hv.shape == (2, 3, 3)
    assert len(calc.engine.calls) == n_eval  # no displaced copies
    (call,) = calc.engine.hvp_calls
    assert call["coulomb"] == "pme" and call["pme_tangent"] is True and call["ewald_accuracy"] == pytest.approx(3e-7)
    assert call["K"] == 2 and call["n"] == 3 and tuple(call["cell"].shape) == (3, 3)
    out = calc(CELL, hessian=True)  # the dense Hessian: its 9 unit directions in one more call of the sweep
    assert out["hessian"].shape == (3, 3, 3, 3)
    assert [c["K"] for c in calc.engine.hvp_calls] == [2, 9] and calc.engine.hvp_calls[-1]["pme_tangent"] is True


def test_unarmed_and_fd_take_differences_of_forces(calc):
    _set(calc, "pme", ewald_accuracy=3e-7)
    assert calc._pme_hessian is None  # the default
    calc.hessian_vector_product(CELL, V)
    assert not calc.engine.hvp_calls
    last = calc.engine.calls[-1]  # ONE batched evaluation of the 4 x 2 displaced copies, with the mesh method
    assert last["n_mol"] == 8 and last["n"] == 24 and last["coulomb"] == "pme"
    calc.set_pme_hessian("analytic")
    calc.hvp_method = "fd"
    calc.hessian_vector_product(CELL, V)
    assert not calc.engine.hvp_calls and calc.engine.calls[-1]["n_mol"] == 8
    calc.hvp_method = "analytic"
    calc.set_pme_hessian(None)  # disarmed again
    calc.hessian_vector_product(CELL, V)
    assert not calc.engine.hvp_calls


def test_the_flag_goes_with_pme_only(calc):
    """Armed, the other methods' calls do not carry the keyword (engines that do not know it keep working)."""
    calc.set_pme_hessian("analytic")
    _set(calc, "ewald", ewald_accuracy=3e-7)
    calc.hessian_vector_product(CELL, V)
    (call,) = calc.engine.hvp_calls
    assert call["coulomb"] == "ewald" and "pme_tangent" not in call


def test_a_bad_mode_raises(calc):
    for bad in ("fd", "Analytic", True, 1):
        with pytest.raises(ValueError, match="set_pme_hessian"):
            calc.set_pme_hessian(bad)
    assert calc._pme_hessian is None


def test_embedding_with_pme_raises(calc):
    _set(calc, "pme")
    calc.set_pme_hessian("analytic")
    calc.set_embedding_hessian("fixed_sites")
    data = dict(CELL, ext_potential=np.zeros(3, np.float32), ext_potential_grad=np.zeros((3, 3), np.float32),
                ext_potential_hess=np.zeros((3, 6), np.float32))
    with pytest.raises(NotImplementedError, match="embedding"):
        calc(data, hessian=True)
    assert not calc.engine.hvp_calls


def test_capacity_policy_of_the_armed_sweep():
    """hvp with the mesh method: the list cutoff is the capped r_c, the options carry the mesh capacity and the Ewald list's row
    capacity; status[7] and status[3] grow them and ask for a repeat."""
    cap = capacity.Capacities(5.0)
    vol, n = 214.0, 12
    rc_ewald = capacity.ewald_list_cutoff([vol], [n], 1e-8)
    assert rc_ewald < capacity.PME_RC_MAX  # (cell A of the GPU tests: below the cap)
    assert capacity.ewald_list_cutoff([340.0], [16], 1e-8) > capacity.PME_RC_MAX  # (cell B: capped)
    rq = capacity.Request("hvp", n, 1, True, _lib.COULOMB_PME, rc_ewald, 0.2, 1e-8)
    opt = cap.fill_options(rq)
    assert opt.coulomb == _lib.COULOMB_PME and opt.pme_max_mesh == capacity.PME_START_MESH and opt.max_nb_lr > 0
    assert opt.ewald_accuracy == pytest.approx(1e-8) and opt.dsf_rc == pytest.approx(rc_ewald)
    st = np.zeros(8, dtype=np.int32)
    st[7] = 20000
    assert cap.grow(st, opt, rq) and cap._pme_max_mesh >= 20000
    opt = cap.fill_options(rq)
    st[:] = 0
    st[7], st[3], st[1] = 20000, 1, opt.max_nb_lr + 100
    assert cap.grow(st, opt, rq) and cap._ewald_nb_lr >= opt.max_nb_lr + 100
    st[3] = 0
    assert not cap.grow(st, cap.fill_options(rq), rq)


def test_symbols():
    assert {"aimnet_engine_set_pme_tangent", "aimnet_debug_pme_tangent"} <= set(_lib.EXPORTED_SYMBOLS)
    lib = _lib.load()
    assert lib.aimnet_engine_set_pme_tangent(None, 1) == _lib.E_INVALID
    assert lib.aimnet_debug_pme_tangent(None, None, None, None, None, None, 0.0, 0, 0, 1e-6, 0, None, None, None, None, None) == _lib.E_INVALID
