"""Host side of the periodic embedding (no GPU): the fp64 yardstick of tests/test_gpu_embedding_periodic.py pinned to the
reference's in-tree Ewald matrix and held to its own properties and to the accuracy rule; the calculator's wiring of
`set_embedding_periodic` against the recording fake engine of tests/fake_engine.py; and eval_validate's refusals, walked by the
stand-alone program tests/embedding_periodic_plan_main.cpp."""
from __future__ import annotations

import math
import os
import subprocess

import numpy as np
import pytest
import torch

import embedding_periodic_yardstick as Y
from conftest import ROOT, golden
from fake_engine import WATER, FakeEngine, fake_calculator
from test_chain_prefetch_plan import _host_compiler


# ---- 1. the reference's data ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acc,key", [(1e-6, "1e-06"), (1e-8, "1e-08")])
def test_field_against_the_references_ewald_matrix(acc, key):
    """The ions of tests/golden/ewald_matrix.npz split into atoms (even) and sites (odd): `field` minus J[I, A] q[A] is one
    constant over the atoms, -pi Q_ext / (V alpha^2) - the in-tree matrix omits the background.  Gate 5e-6 max|J q|, the gate of
    tests/test_oracle_ewald.py for these potentials.  Measured: spread 1e-7, constant -0.105969."""
    from oracle import aimnet2_oracle as O

    g = golden("ewald_matrix")
    I, A = np.arange(0, 12, 2), np.arange(1, 12, 2)
    vol = abs(np.linalg.det(g["cell"]))
    al, rc, kc = O.ewald_parameters(12, vol, acc)
    phi, _, _ = Y.field(g["coord"][I], g["coord"][A], g["q"][A], g["cell"], al, rc, kc, ke=1.0)
    ref = g["J_" + key].astype(np.float64)[np.ix_(I, A)] @ g["q"][A]
    diff = phi - ref
    want = -math.pi * g["q"][A].sum() / (vol * al * al)
    gate = 5e-6 * np.abs(ref).max()
    print(f"[embedding periodic] accuracy {acc:g}: field - J q = {diff.mean():.6f} (background {want:.6f}), spread "
          f"{np.ptp(diff):.2e}, gate {gate:.2e}")
    assert np.ptp(diff) <= gate and np.abs(diff - want).max() <= gate


# ---- 2. the yardstick's own properties -----------------------------------------------------------------------------------------
def _triclinic():
    rng = np.random.default_rng(4)
    cell = np.array([[11.0, 0.0, 0.0], [1.3, 9.0, 0.0], [-0.8, 1.1, 8.0]])
    x = rng.uniform(0, 1, (24, 3)) @ cell
    q = rng.uniform(-0.4, 0.4, 24)
    X, Q, _ = Y.sites(x, cell, 64, 7)
    return cell, x, q, X, Q


def test_yardstick_properties():
    cell, x, q, X, Q = _triclinic()
    assert abs(Q.sum()) > 0.1  # a net charge: the background is exercised
    al, rc, kc = Y.params(cell, 24 + 64, 1e-10)
    phi, g, _ = Y.field(x, X, Q, cell, al, rc, kc)
    # independent of alpha (rc ~ 1 / alpha, kc ~ alpha keep the accuracy)
    for s in (0.7, 1.4):
        p2, g2, _ = Y.field(x, X, Q, cell, al * s, rc / s, kc * s)
        dp, dg = np.abs(p2 - phi).max() / Y.KE, np.abs(g2 - g).max() / Y.KE
        print(f"[embedding periodic] alpha x {s}: max|d phi| {dp:.2e}, max|d g| {dg:.2e} (gate 1e-9)")
        assert dp <= 1e-9 and dg <= 1e-9
    # g is the gradient of phi
    h, fd = 1e-4, np.zeros_like(g)
    for c in range(3):
        e = np.zeros(3)
        e[c] = h
        fd[:, c] = (Y.field(x + e, X, Q, cell, al, rc, kc)[0] - Y.field(x - e, X, Q, cell, al, rc, kc)[0]) / (2 * h)
    r = np.abs(fd - g).max() / np.abs(g).max()
    print(f"[embedding periodic] g against central differences of phi: {r:.2e} of max|g| (gate 1e-8)")
    assert r <= 1e-8
    # reciprocity and Newton's third law between the two particle sets
    psi, f_site, _ = Y.site_terms(x, q, X, Q, cell, al, rc, kc)
    e1, e2 = (q * phi).sum(), (Q * psi).sum()
    net = (q[:, None] * g).sum(0) - f_site.sum(0)
    print(f"[embedding periodic] sum q phi - sum Q psi = {abs(e1 - e2) / Y.KE:.2e}, |sum q g + sum Q grad psi| = "
          f"{np.abs(net).max() / Y.KE:.2e} (gates 1e-12)")
    assert abs(e1 - e2) / Y.KE <= 1e-12 and np.abs(net).max() / Y.KE <= 1e-12


# ---- 3. the accuracy rule --------------------------------------------------------------------------------------------------------
def test_accuracy_rule_on_the_glucose_cell():
    """rms error of g <= accuracy x rms g (the project's PME calibration rule) and max error of phi <= accuracy x rms phi, against
    the sums at 1e-12.  The ratios are printed (0.41 / 0.39 / 0.36 of the gate for g, 0.44 / 0.32 / 0.24 for phi)."""
    gl = golden("pbc96_dsf15")
    x, cell = gl["coord"].astype(np.float64), gl["cell"].astype(np.float64)
    X, Q, draws = Y.sites(x, cell, 64, 5)
    print(f"[embedding periodic] 64 sites in {draws} draws, Q_ext = {Q.sum():.3f}")
    ref_phi, ref_g, _ = Y.field(x, X, Q, cell, *Y.params(cell, 160, 1e-12))
    rms = lambda v: float(np.sqrt((v * v).mean()))  # noqa: E731
    for acc in (1e-4, 1e-6, 1e-8):
        phi, g, _ = Y.field(x, X, Q, cell, *Y.params(cell, 160, acc))
        rg, rp = rms(g - ref_g) / (acc * rms(ref_g)), np.abs(phi - ref_phi).max() / (acc * rms(ref_phi))
        print(f"[embedding periodic] accuracy {acc:g}: rms error of g at {rg:.2f} of the gate, max error of phi at {rp:.2f}")
        assert rg <= 1.0 and rp <= 1.0


# ---- 4. the calculator against the recording fake engine ----------------------------------------------------------------------
class _Engine(FakeEngine):
    """tests/fake_engine.py's engine, plus the outputs an embedded evaluation returns."""

    def eval(self, coord, numbers, mol_idx, charge, **kw):
        out = super().eval(coord, numbers, mol_idx, charge, **kw)
        emb = kw.get("embedding")
        if emb is not None:
            out["embedding_energy"] = torch.full((charge.shape[0],), 7.0, dtype=torch.float64)
            if emb.get("want_ext_forces"):
                out["ext_forces"] = torch.arange(emb["ext_coord"].shape[0] * 3, dtype=torch.float32).view(-1, 3)
        return out


@pytest.fixture()
def calc(monkeypatch):
    return fake_calculator(monkeypatch, engine=_Engine)


SITES = dict(ext_coord=[[3.0, 0.0, 0.0], [0.0, 4.0, 0.0]], ext_charge=[0.4, -0.4])
CELL = np.eye(3, dtype=np.float32) * 12.0
BOX = dict(WATER, cell=CELL, **SITES)


def _calls(calc):
    e = calc.engine
    return len(e.calls) + len(e.hvp_calls) + len(e.charge_response_calls)


@pytest.mark.filterwarnings("ignore:Switching to DSF")
def test_unarmed_sites_with_a_cell_are_refused_as_before(calc):
    assert calc._embedding_periodic_mode is None
    calc.set_embedding_hessian("fixed_sites")  # (without it the second derivatives refuse every embedding)
    n0 = _calls(calc)
    with pytest.raises(ValueError, match="non-periodic"):
        calc(BOX, forces=True)
    with pytest.raises(ValueError, match="non-periodic"):
        calc.hessian_vector_product(BOX, np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError, match="non-periodic"):
        calc(BOX, forces=True, hessian=True)
    calc.set_embedding_periodic("ewald")
    calc.set_embedding_periodic(None)  # switched off again: the same refusal
    with pytest.raises(ValueError, match="non-periodic"):
        calc(BOX, forces=True)
    assert _calls(calc) == n0  # the engine was never touched


@pytest.mark.filterwarnings("ignore:Switching to DSF")
def test_armed_sites_with_a_cell_pass_the_accuracy(calc):
    with pytest.raises(ValueError, match="mode"):
        calc.set_embedding_periodic("bogus")
    with pytest.raises(ValueError, match="accuracy"):
        calc.set_embedding_periodic("ewald", accuracy=1.5)
    calc.set_embedding_periodic("ewald", accuracy=1e-5)
    out = calc(BOX, forces=True)
    call = calc.engine.calls[-1]
    emb = call["lists"]["embedding"]
    assert emb["ewald_accuracy"] == 1e-5 and call["cell"] == (3, 3) and call["pbc"] == (True, True, True)
    assert set(emb) == {"ext_coord", "ext_charge", "want_ext_forces", "ewald_accuracy"} and tuple(emb["ext_coord"].shape) == (2, 3)
    assert set(out) == {"energy", "charges", "forces", "embedding_energy", "ext_forces"}
    # without a cell nothing changes: no accuracy key
    calc(dict(WATER, **SITES), forces=True)
    assert "ewald_accuracy" not in calc.engine.calls[-1]["lists"]["embedding"]
    # a per-atom potential with a cell carries no key either
    calc(dict(WATER, cell=CELL, ext_potential=[0.1, 0.2, 0.3], ext_potential_grad=np.zeros((3, 3))), forces=True)
    assert set(calc.engine.calls[-1]["lists"]["embedding"]) == {"potential", "potential_grad"}


@pytest.mark.filterwarnings("ignore:Switching to DSF")
def test_armed_refusals(calc):
    calc.set_embedding_periodic("ewald")
    calc.set_embedding_hessian("fixed_sites")
    n0 = _calls(calc)
    for pbc in ([True, True, False], [False, False, False]):
        with pytest.raises(ValueError, match="periodic along all three axes"):
            calc(dict(BOX, pbc=pbc), forces=True)
    with pytest.raises(NotImplementedError, match="periodic embedding sites"):
        calc(BOX, forces=True, stress=True)
    with pytest.raises(NotImplementedError, match="periodic embedding sites"):
        calc(BOX, forces=True, hessian=True)
    with pytest.raises(NotImplementedError, match="periodic embedding sites"):
        calc.hessian_vector_product(BOX, np.zeros((3, 3), np.float32))
    calc._dd = object()  # (domain decomposition on: refused before the decomposed engine is looked at)
    with pytest.raises(NotImplementedError, match="periodic embedding sites"):
        calc(BOX, forces=True)
    calc._dd = None
    assert _calls(calc) == n0


@pytest.mark.filterwarnings("ignore:Switching to DSF")
def test_batched_layout_with_per_system_cells(calc):
    calc.set_embedding_periodic("ewald")
    coord = np.stack([WATER["coord"], np.asarray(WATER["coord"]) + 0.1]).astype(np.float32)
    cells = np.stack([CELL, CELL * 1.1])
    d = dict(coord=coord, numbers=[[8, 1, 1]] * 2, charge=[0.0, 0.0], cell=cells,
             ext_coord=np.stack([SITES["ext_coord"]] * 2).astype(np.float32), ext_charge=[[0.4, -0.4], [0.1, 0.0]])
    out = calc(d, forces=True)
    call = calc.engine.calls[-1]
    emb = call["lists"]["embedding"]
    assert call["cell"] == (2, 3, 3) and call["n_mol"] == 2
    assert emb["ext_mol_idx"].tolist() == [0, 0, 1, 1] and tuple(emb["ext_coord"].shape) == (4, 3) and emb["ewald_accuracy"] == 1e-6
    assert tuple(out["ext_forces"].shape) == (2, 2, 3) and tuple(out["embedding_energy"].shape) == (2,)


class _Atoms:
    """The Atoms stand-in of tests/test_host_logic.py: what AIMNet2ASE reads."""

    def __init__(self, numbers, positions, cell=None, pbc=(False, False, False), info=None):
        self.numbers, self.positions = np.asarray(numbers), np.asarray(positions, dtype=float)
        self.cell, self.pbc, self.info = cell, np.asarray(pbc), dict(info or {})

    def copy(self):
        return _Atoms(self.numbers.copy(), self.positions.copy(), None if self.cell is None else np.array(self.cell), self.pbc.copy(), self.info)

    def __len__(self):
        return len(self.numbers)


@pytest.mark.filterwarnings("ignore:Switching to DSF")
def test_ase_adapter_embeds_periodic_atoms(calc):
    """AIMNet2ASE needs no code of its own: with the calculator armed, embed() on periodic atoms passes cell, pbc and the sites."""
    from aimnetcentral_amd.aimnet2ase import AIMNet2ASE

    ase_calc = AIMNet2ASE(calc, charge=0)
    pc = ase_calc.embed(charges=np.asarray(SITES["ext_charge"]), positions=np.asarray(SITES["ext_coord"]))
    atoms = _Atoms(WATER["numbers"], WATER["coord"], cell=np.eye(3) * 12.0, pbc=(True, True, True))
    n0 = _calls(calc)
    with pytest.raises(ValueError, match="non-periodic"):  # unarmed: as before
        ase_calc.calculate(atoms, properties=["energy", "forces"])
    assert _calls(calc) == n0
    calc.set_embedding_periodic("ewald")
    ase_calc.reset()
    ase_calc.calculate(atoms, properties=["energy", "forces"])
    call = calc.engine.calls[-1]
    emb = call["lists"]["embedding"]
    assert call["cell"] == (3, 3) and call["pbc"] == (True, True, True) and emb["ewald_accuracy"] == 1e-6
    assert np.allclose(emb["ext_coord"].numpy(), SITES["ext_coord"]) and np.allclose(emb["ext_charge"].numpy(), SITES["ext_charge"])
    assert pc.get_forces(ase_calc).shape == (2, 3) and ase_calc.results["embedding_energy"] == 7.0


def test_engine_keys():
    from aimnetcentral_amd import capacity
    from aimnetcentral_amd.engine import HipEngine

    assert "ewald_accuracy" in HipEngine.EMBEDDING_KEYS
    assert capacity.Capacities(5.0)._emb_max_k == 8192


# ---- 5. the plan --------------------------------------------------------------------------------------------------------------
def test_eval_validate_walk(tmp_path):
    exe = str(tmp_path / "embedding_periodic_plan")
    base = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
            "-I", os.path.join(ROOT, "aimnetcentral_amd", "csrc"), os.path.join(ROOT, "tests", "embedding_periodic_plan_main.cpp"), "-o", exe]
    cxx = _host_compiler()
    r = subprocess.run([cxx, "-static-libasan", "-static-libubsan", *base], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run([cxx, *base], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "embedding periodic plan ok" in r.stdout
