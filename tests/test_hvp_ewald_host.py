"""Which second-derivative operator the calculator takes for the Ewald methods, with the recording fake engine of
tests/test_host_logic.py: "ewald" goes to the engine's analytic sweep (one call, with the method and its accuracy), "pme" and
`hvp_method = "fd"` to differences of the forces of displaced copies.  CPU only."""
from __future__ import annotations

import warnings

import numpy as np
import pytest
import torch

from fake_engine import FakeEngine, fake_calculator


class RecordingHvpEngine(FakeEngine):
    def hvp(self, coord, numbers, mol_idx, charge, vectors, **kw):
        self.hvp_calls = getattr(self, "hvp_calls", [])
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


def test_ewald_takes_the_analytic_sweep(calc):
    _set(calc, "ewald", ewald_accuracy=3e-7)
    n_eval = len(calc.engine.calls)
    hv = calc.hessian_vector_product(CELL, V)
    assert hv.shape == (2, 3, 3)
    assert len(calc.engine.calls) == n_eval  # no displaced copies
    (call,) = calc.engine.hvp_calls
    assert call["coulomb"] == "ewald" and call["ewald_accuracy"] == pytest.approx(3e-7) and call["K"] == 2 and call["n"] == 3
    assert tuple(call["cell"].shape) == (3, 3)
    out = calc(CELL, hessian=True)  # the dense Hessian: its 9 unit directions in one more call of the sweep
    assert out["hessian"].shape == (3, 3, 3, 3)
    assert [c["K"] for c in calc.engine.hvp_calls] == [2, 9] and calc.engine.hvp_calls[-1]["coulomb"] == "ewald"


def test_pme_and_fd_take_differences_of_forces(calc):
    _set(calc, "pme", ewald_accuracy=3e-7)
    calc.hessian_vector_product(CELL, V)
    assert not getattr(calc.engine, "hvp_calls", [])
    last = calc.engine.calls[-1]  # ONE batched evaluation of the 4 x 2 displaced copies, with the mesh method
    assert last["n_mol"] == 8 and last["n"] == 24 and last["coulomb"] == "pme" and last["ewald_accuracy"] == pytest.approx(3e-7)
    _set(calc, "ewald", ewald_accuracy=3e-7)
    calc.hvp_method = "fd"
    calc.hessian_vector_product(CELL, V)
    assert not getattr(calc.engine, "hvp_calls", [])
    assert calc.engine.calls[-1]["n_mol"] == 8 and calc.engine.calls[-1]["coulomb"] == "ewald"
