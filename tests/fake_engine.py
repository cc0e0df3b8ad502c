"""The recording stand-in for HipEngine shared by the CPU tests of the calculator (the reference tests its calculator the same
way, with TinyLegacyModel / RecordingExternalCoulomb fakes, tests/test_calculator.py:15-196), and the helper that builds an
AIMNet2Calculator on top of it."""
from __future__ import annotations

import torch

from aimnetcentral_amd import calculator as calc_mod
from aimnetcentral_amd import loader

WATER = dict(coord=[[0.0, 0.0, 0.1173], [0.0, 0.7572, -0.4692], [0.0, -0.7572, -0.4692]], numbers=[8, 1, 1], charge=0.0)


class FakeEngine:
    """Records eval() / hvp() / charge_response() calls and returns recognisable tensors; stands in for HipEngine."""

    def __init__(self, spec, device):
        self.spec, self.device, self.calls, self.d3_tables = spec, torch.device("cpu"), [], None
        self.hvp_calls, self.charge_response_calls = [], []
        self.nq = int(getattr(spec, "num_charge_channels", 1))

    def set_dftd3_tables(self, tables):
        self.d3_tables = tables

    def eval(self, coord, numbers, mol_idx, charge, cell=None, pbc=(True, True, True), forces=False, stress=False,
             coulomb="simple", dsf_rc=15.0, dsf_alpha=0.2, ewald_accuracy=1e-6, sync=True, dftd3=None, host_out=False, **lists):
        self.calls.append(dict(lists=lists, host_out=host_out, n=coord.shape[0], n_mol=charge.shape[0], coulomb=coulomb, dsf_rc=dsf_rc, dsf_alpha=dsf_alpha, dftd3=dftd3,
                               ewald_accuracy=ewald_accuracy,
                               pbc=pbc, cell=None if cell is None else tuple(cell.shape), mol_idx=mol_idx.clone(),
                               numbers=numbers.clone(), charge=charge.clone()))
        n = coord.shape[0]
        out = {"energy": torch.arange(charge.shape[0], dtype=torch.float64), "charges": torch.arange(n, dtype=torch.float32) + 1}
        if self.nq == 2:
            assert charge.ndim == 2 and charge.shape[1] == 2
            out["spin_charges"] = -(torch.arange(n, dtype=torch.float32) + 1)
        if forces:
            out["forces"] = torch.ones(n, 3) * (torch.arange(n, dtype=torch.float32) + 1).unsqueeze(-1)
        if stress:
            out["stress"] = torch.zeros(3, 3) if cell is not None and cell.ndim == 2 else torch.zeros(charge.shape[0], 3, 3)
        return out

    def hvp(self, coord, numbers, mol_idx, charge, vectors, cell=None, pbc=(True, True, True), coulomb="simple", dsf_rc=15.0,
            dsf_alpha=0.2, want_forces=False, dftd3=None, ewald_accuracy=1e-6):
        self.hvp_calls.append(dict(K=int(vectors.shape[0]), n=coord.shape[0], coulomb=coulomb, dsf_rc=dsf_rc, dsf_alpha=dsf_alpha, dftd3=dftd3,
                                   ewald_accuracy=ewald_accuracy, pbc=pbc, cell=None if cell is None else tuple(cell.shape)))
        return {"hv": torch.zeros_like(vectors)}

    def charge_response(self, coord, numbers, mol_idx, charge, vectors, cell=None, pbc=(True, True, True), want_dipole=None):
        K, n = int(vectors.shape[0]), coord.shape[0]
        self.charge_response_calls.append(dict(K=K, n=n, pbc=pbc, cell=None if cell is None else tuple(cell.shape)))
        out = {"charges": torch.arange(n, dtype=torch.float32) + 1, "dq": torch.zeros(K, n)}
        if cell is None:
            out["dmu"] = torch.zeros(K, 1, 3)
        return out


def _as_tensor_cpu(orig):
    def f(data, dtype=None, device=None):
        return orig(data, dtype=dtype, device="cpu")

    return f


def fake_calculator(monkeypatch, engine=FakeEngine, spec=None, **kw):
    """An AIMNet2Calculator whose engine is `engine` and whose tensors stay on the CPU."""
    monkeypatch.setattr(calc_mod, "HipEngine", engine)
    monkeypatch.setattr(torch, "as_tensor", _as_tensor_cpu(torch.as_tensor))
    c = calc_mod.AIMNet2Calculator(loader.synthetic_spec(0) if spec is None else spec, device="cuda", **kw)
    c.device = "cpu"
    return c
