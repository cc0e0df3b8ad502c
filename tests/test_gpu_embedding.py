"""Electrostatic embedding (csrc/embed.hip, aimnet_engine_set_embedding) on the GPU against the fp64 yardstick of
tests/embedding_yardstick.py (tests/test_embedding_host.py holds it to differences of sum q phi): oracle charges, forces and
energies, the Jacobian of the charges from the fp64 tangent sweep, phi and grad phi from numpy.  Every comparison prints its ratio
to the gate before it asserts."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import embedding_yardstick as Y
from conftest import CHARGE_ATOL, ENERGY_ATOL, FORCE_ATOL, FORCE_RTOL, assert_forces_close, energy_tol, golden

pytestmark = pytest.mark.gpu

U = 2.0**-24  # one fp32 rounding
ROUND = 8.0 * U  # eight of them per pair term, none in the double accumulation


def _t(a, dt=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dt).cuda()


def _np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _args(eng, coord, numbers, charge, mol, mult=None):
    q = np.atleast_1d(np.asarray(charge, dtype=np.float32))
    if eng.nq == 2:
        mt = np.ones_like(q) if mult is None else np.atleast_1d(np.asarray(mult, dtype=np.float32))
        q = np.stack([0.5 * q + 0.5 * (mt - 1), 0.5 * q - 0.5 * (mt - 1)], -1)
    return _t(coord), _t(numbers, torch.int32), _t(mol, torch.int32), _t(q)


def _ratio(what, err, gate):
    err, gate = np.asarray(err, np.float64), np.asarray(gate, np.float64)
    r = float((err / gate).max())
    print(f"[embedding] {what}: max|d| = {float(err.max()):.3e}, gate {float(gate.min()):.3e}, ratio {r:.3f}")
    assert (err <= gate).all(), f"{what}: ratio {r:.3f}"


def _force_gate(ref):
    return FORCE_ATOL + FORCE_RTOL * np.abs(ref).max()


def _single(name):
    g = golden(name)
    n = len(g["numbers"])
    X, Q = Y.sites(g["coord"])
    return g, n, np.zeros(n, np.int64), X, Q


# ---- 1. single molecule -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cold24", "hvp40"])
def test_single_molecule(hip_engine, oracle64, name):
    g, n, mol, X, Q = _single(name)
    ref = Y.model_reference(oracle64, name, g["coord"], g["numbers"], 0.0, mol)
    emb = Y.embedded_reference(ref, g["coord"], X, Q)
    args = _args(hip_engine, g["coord"], g["numbers"], [0.0], mol)
    res = hip_engine.eval(*args, forces=True, coulomb="simple",
                          embedding=dict(ext_coord=_t(X), ext_charge=_t(Q), want_ext_forces=True, want_ext_potential=True))
    bare = hip_engine.eval(*args, forces=True, coulomb="simple")
    assert set(res) == set(bare) | {"embedding_energy", "ext_forces", "ext_potential"}
    f = _np64(res["forces"])
    print(f"[embedding] {name}: max|F - F_ref| = {np.abs(f - emb['forces']).max():.3e} (gate {_force_gate(emb['forces']):.3e}); without the "
          f"charge response it would be {np.abs(ref['forces'] - ref['charges'][:, None] * emb['g'] - emb['forces']).max():.3e}")
    assert_forces_close(f, emb["forces"], name)
    _ratio(name + " charges", np.abs(_np64(res["charges"]) - ref["charges"]), CHARGE_ATOL)
    assert torch.equal(res["charges"], bare["charges"])  # the charges do not see the field
    _ratio(name + " ext_forces", np.abs(_np64(res["ext_forces"]) - emb["f_site"]), _force_gate(emb["f_site"]))
    de = _np64(res["energy"]) - _np64(bare["energy"])
    gate = ENERGY_ATOL + CHARGE_ATOL * np.abs(emb["phi"]).sum()
    _ratio(name + " E(with) - E(without)", np.abs(de - emb["e_emb"]), gate)
    _ratio(name + " embedding_energy", np.abs(_np64(res["embedding_energy"]) - emb["e_emb"]), gate)


# ---- 2. the sums alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 63, 3 * 1024 + 5, 66 * 1024 + 3])
def test_sums_against_numpy_with_the_engines_charges(hip_engine, M):
    """fp32 pair terms summed in double: eight roundings per term, 8 * 2^-24 * sum |term| per output.  M = 1, 63: one partial chunk;
    3 * EMBED_CHUNK + 5: four slots of one chunk each; 66 * EMBED_CHUNK + 3: more chunks than the 64 slots (a slot sums two)."""
    from aimnetcentral_amd import _lib

    assert _lib.EMBED_CHUNK == 1024
    g = golden("cold24")
    n = 24
    X, Q = Y.sites(g["coord"], M)
    args = _args(hip_engine, g["coord"], g["numbers"], [0.0], np.zeros(n, np.int64))
    res = hip_engine.eval(*args, forces=True, coulomb="simple",
                          embedding=dict(ext_coord=_t(X), ext_charge=_t(Q), want_ext_forces=True, want_ext_potential=True))
    q = _np64(res["charges"])
    x = g["coord"].astype(np.float32)
    phi, _, abs_phi, _ = Y.field(x, X, Q)
    _ratio(f"M={M} embedding_energy", np.abs(_np64(res["embedding_energy"])[0] - (q * phi).sum()), ROUND * (np.abs(q) * abs_phi).sum())
    pot, f_site, abs_pot, abs_f = Y.site_terms(x, q, X, Q)
    _ratio(f"M={M} ext_potential", np.abs(_np64(res["ext_potential"]) - pot), ROUND * abs_pot)
    _ratio(f"M={M} ext_forces", np.abs(_np64(res["ext_forces"]) - f_site).max(-1), ROUND * abs_f)


def test_sums_of_a_skewed_batch(hip_engine):
    """Two copies of cold24 as two molecules, 3 * EMBED_CHUNK + 5 sites on the first and one on the second: the slots follow the
    average (two), so a slot of the first molecule sums two chunks, and the site blocks straddle the molecule boundary."""
    g = golden("cold24")
    c = g["coord"].astype(np.float32)
    coord = np.concatenate([c, c + np.array([60.0, 0.0, 0.0], np.float32)])
    mol = np.repeat(np.arange(2), 24)
    X0, Q0 = Y.sites(c, 3 * 1024 + 5)
    X1, Q1 = Y.sites(coord[24:], 1, 9)
    X, Q, em = np.concatenate([X0, X1]), np.concatenate([Q0, Q1]), np.concatenate([np.zeros(len(Q0), np.int64), [1]])
    res = hip_engine.eval(*_args(hip_engine, coord, np.concatenate([g["numbers"]] * 2), [0.0, 0.0], mol), forces=True, coulomb="simple",
                          embedding=dict(ext_coord=_t(X), ext_charge=_t(Q), ext_mol_idx=_t(em, torch.int32), want_ext_forces=True,
                                         want_ext_potential=True))
    q = _np64(res["charges"])
    phi, _, abs_phi, _ = Y.field(coord, X, Q, mol, em)
    _ratio("skewed batch embedding_energy", np.abs(_np64(res["embedding_energy"]) - np.bincount(mol, weights=q * phi)),
           ROUND * np.bincount(mol, weights=np.abs(q) * abs_phi))
    pot, f_site, abs_pot, abs_f = Y.site_terms(coord, q, X, Q, mol, em)
    _ratio("skewed batch ext_potential", np.abs(_np64(res["ext_potential"]) - pot), ROUND * abs_pot)
    _ratio("skewed batch ext_forces", np.abs(_np64(res["ext_forces"]) - f_site).max(-1), ROUND * abs_f)


# ---- 3. batch ------------------------------------------------------------------------------------------------------------
def _batch_sites(g):
    """Sites per molecule of batch5: the M = 64 construction for molecules 0 and 3 (seeds 5, 6), one site for molecule 1, none for
    molecules 2 and 4."""
    mol = g["mol_idx"]
    Xs, Qs, ms = [], [], []
    for m, (M, seed) in {0: (64, 5), 1: (1, 7), 3: (64, 6)}.items():
        X, Q = Y.sites(g["coord"][mol == m], M, seed)
        Xs.append(X), Qs.append(Q), ms.append(np.full(M, m, np.int64))
    return np.concatenate(Xs), np.concatenate(Qs), np.concatenate(ms)


def test_batch_with_ext_mol_idx(hip_engine, oracle64, oracle32):
    from oracle import aimnet2_oracle as O

    g = golden("batch5")
    mol = g["mol_idx"]
    X, Q, em = _batch_sites(g)
    ref = Y.model_reference(oracle64, "batch5", g["coord"], g["numbers"], g["charge"], mol, jac_mols=(0, 1, 3))
    emb = Y.embedded_reference(ref, g["coord"], X, Q, mol, em)
    args = _args(hip_engine, g["coord"], g["numbers"], g["charge"], mol)
    e = dict(ext_coord=_t(X), ext_charge=_t(Q), ext_mol_idx=_t(em, torch.int32), want_ext_forces=True)
    res = hip_engine.eval(*args, forces=True, coulomb="simple", embedding=e)
    bare = hip_engine.eval(*args, forces=True, coulomb="simple")
    assert_forces_close(_np64(res["forces"]), emb["forces"], "batch5")
    _ratio("batch5 charges", np.abs(_np64(res["charges"]) - ref["charges"]), CHARGE_ATOL)
    _ratio("batch5 ext_forces", np.abs(_np64(res["ext_forces"]) - emb["f_site"]), _force_gate(emb["f_site"]))
    # the hot fixture's energies: widened by the fp32 oracle's own distance from the fp64 one (tests/test_gpu_parity.py::compare)
    e32 = O.evaluate(oracle32, g["coord"], g["numbers"], g["charge"], mol, forces=False)["energy"]
    gate = energy_tol(np.bincount(mol)) + np.abs(np.asarray(e32, np.float64) - ref["energy"]) + \
        CHARGE_ATOL * np.bincount(mol, weights=np.abs(emb["phi"]), minlength=5)
    _ratio("batch5 E(with) - E(without)", np.abs(_np64(res["energy"]) - _np64(bare["energy"]) - emb["e_emb"]), gate)
    _ratio("batch5 embedding_energy", np.abs(_np64(res["embedding_energy"]) - emb["e_emb"]), gate)
    assert _np64(res["embedding_energy"])[2] == 0.0 and _np64(res["embedding_energy"])[4] == 0.0  # molecules without sites
    bad = em.copy()
    bad[[3, 70]] = bad[[70, 3]]
    with pytest.raises(ValueError, match="ext_mol_idx"):
        hip_engine.eval(*args, forces=True, coulomb="simple", embedding=dict(e, ext_mol_idx=_t(bad, torch.int32)))
    assert int(hip_engine.last_status[6]) & 128
    again = hip_engine.eval(*args, forces=True, coulomb="simple", embedding=e)  # the engine is usable afterwards
    assert torch.equal(again["forces"], res["forces"])


# ---- 4. two charge channels --------------------------------------------------------------------------------------------
def test_two_channel_model(hip_engine_nse, oracle64_nse):
    g = golden("nse")
    coord, numbers, charge, mol, mult = (g["b5_" + k] for k in ("coord", "numbers", "charge", "mol_idx", "mult"))
    X, Q, em = [], [], []
    for m in (1, 3):  # two of the five molecules carry sites
        Xm, Qm = Y.sites(coord[mol == m], 16, 5 + m)
        X.append(Xm), Q.append(Qm), em.append(np.full(16, m, np.int64))
    X, Q, em = np.concatenate(X), np.concatenate(Q), np.concatenate(em)
    ref = Y.model_reference(oracle64_nse, "nse_b5", coord, numbers, charge, mol, mult, jac_mols=(1, 3))
    emb = Y.embedded_reference(ref, coord, X, Q, mol, em)
    res = hip_engine_nse.eval(*_args(hip_engine_nse, coord, numbers, charge, mol, mult), forces=True, coulomb="simple",
                              embedding=dict(ext_coord=_t(X), ext_charge=_t(Q), ext_mol_idx=_t(em, torch.int32)))
    assert_forces_close(_np64(res["forces"]), emb["forces"], "nse b5")
    _ratio("nse b5 charges", np.abs(_np64(res["charges"]) - ref["charges"]), CHARGE_ATOL)
    _ratio("nse b5 spin_charges", np.abs(_np64(res["spin_charges"]) - ref["spin_charges"]), CHARGE_ATOL)


# ---- 5. per-atom mode ---------------------------------------------------------------------------------------------------
def test_per_atom_potential_equals_the_point_charges(hip_engine):
    g, n, mol, X, Q = _single("hvp40")
    args = _args(hip_engine, g["coord"], g["numbers"], [0.0], mol)
    pc = hip_engine.eval(*args, forces=True, coulomb="simple", embedding=dict(ext_coord=_t(X), ext_charge=_t(Q)))
    phi, grad, _, abs_g = Y.field(g["coord"].astype(np.float32), X, Q)
    pa = hip_engine.eval(*args, forces=True, coulomb="simple", embedding=dict(potential=_t(phi), potential_grad=_t(grad)))
    qmax = float(pc["charges"].abs().max())
    gate = ROUND * abs_g.max() * qmax + _force_gate(_np64(pc["forces"]))
    _ratio("hvp40 per-atom against point-charge mode", np.abs(_np64(pa["forces"]) - _np64(pc["forces"])), gate)


def test_uniform_field_against_the_polar_tensor(hip_engine):
    """phi = -E.x, grad phi = -E: E_emb = -E.mu, and the force change is sum_a E_a d mu_a / d x_ic - the backward seed against the
    forward tangent sweep.  Gate: the force gate plus |E|_1 times the charge-response gate (1e-5 + 3e-5 max|dq|) per atom, summed
    over the atoms."""
    g, n, mol, _, _ = _single("hvp40")
    args = _args(hip_engine, g["coord"], g["numbers"], [0.0], mol)
    E = np.array([0.05, -0.02, 0.03])
    x = g["coord"].astype(np.float32).astype(np.float64)
    eye = np.eye(3 * n, dtype=np.float32).reshape(3 * n, n, 3)
    cr = hip_engine.charge_response(*args, _t(eye))
    P = _np64(cr["dmu"])[:, 0]  # [(i, c), a]
    res = hip_engine.eval(*args, forces=True, coulomb="simple",
                          embedding=dict(potential=_t(-(x @ E)), potential_grad=_t(np.tile(-E, (n, 1)))))
    bare = hip_engine.eval(*args, forces=True, coulomb="simple")
    q = _np64(res["charges"])
    mu = (q[:, None] * x).sum(0)
    _ratio("uniform field embedding_energy", np.abs(_np64(res["embedding_energy"])[0] + E @ mu),
           ENERGY_ATOL + ROUND * np.abs(q[:, None] * x * E).sum())
    dF = _np64(res["forces"]) - _np64(bare["forces"])
    want = (P @ E).reshape(n, 3)
    gate = _force_gate(_np64(res["forces"])) + np.abs(E).sum() * n * (1e-5 + 3e-5 * float(cr["dq"].abs().max()))
    _ratio("uniform field force change against the polar tensor", np.abs(dF - want), gate)


def test_periodic_cell_with_a_per_atom_potential(hip_engine):
    g = golden("pbc96_dsf8_wrapped")
    n = 96
    kw = dict(cell=_t(g["cell"]), coulomb="dsf", dsf_rc=float(g["dsf_rc"]), dsf_alpha=float(g["dsf_alpha"]))
    args = _args(hip_engine, g["coord"], g["numbers"], [0.0], np.zeros(n, np.int64))
    rng = np.random.default_rng(8)
    phi, grad = rng.uniform(-0.3, 0.3, n).astype(np.float32), rng.uniform(-0.05, 0.05, (n, 3)).astype(np.float32)
    e = dict(potential=_t(phi), potential_grad=_t(grad))
    res = hip_engine.eval(*args, forces=True, embedding=e, **kw)
    bare = hip_engine.eval(*args, forces=True, **kw)
    eye = np.eye(3 * n, dtype=np.float32).reshape(3 * n, n, 3)
    cr = hip_engine.charge_response(*args, _t(eye), cell=kw["cell"])
    q, J = _np64(res["charges"]), _np64(cr["dq"])  # J [(i, c), j]
    want = -(q[:, None] * grad.astype(np.float64) + (J @ phi.astype(np.float64)).reshape(n, 3))
    gate = _force_gate(_np64(res["forces"])) + np.abs(phi).sum() * (1e-5 + 3e-5 * np.abs(J).max())
    _ratio("pbc96 force change against -(q g + J phi)", np.abs(_np64(res["forces"]) - _np64(bare["forces"]) - want), gate)
    _ratio("pbc96 embedding_energy", np.abs(_np64(res["embedding_energy"])[0] - (q * phi).sum()), ENERGY_ATOL + ROUND * np.abs(q * phi).sum())
    with pytest.raises(ValueError, match="stress"):
        hip_engine.eval(*args, forces=True, stress=True, embedding=e, **kw)
    with pytest.raises(ValueError, match="non-periodic"):
        hip_engine.eval(*args, forces=True, embedding=dict(ext_coord=_t(np.zeros((1, 3))), ext_charge=_t([0.1])), **kw)


# ---- 6. contract ------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_contract(hip_engine):
    from aimnetcentral_amd import _lib, loader
    from aimnetcentral_amd.engine import HipEngine

    g, n, mol, _, _ = _single("cold24")
    X, Q = Y.sites(g["coord"], 3 * 1024 + 5)
    args = _args(hip_engine, g["coord"], g["numbers"], [0.0], mol)
    e = dict(ext_coord=_t(X), ext_charge=_t(Q), want_ext_forces=True, want_ext_potential=True)
    a = hip_engine.eval(*args, forces=True, coulomb="simple", embedding=e)
    assert _same_bits(a, hip_engine.eval(*args, forces=True, coulomb="simple", embedding=e))
    hip_engine._ws.fill_(0xFF)
    hip_engine._emb_scratch.fill_(0xFF)
    assert _same_bits(a, hip_engine.eval(*args, forces=True, coulomb="simple", embedding=e))
    # energy only: the same energies, bit for bit
    eo = hip_engine.eval(*args, coulomb="simple", embedding=e)
    assert torch.equal(eo["energy"], a["energy"]) and torch.equal(eo["embedding_energy"], a["embedding_energy"])
    assert torch.equal(eo["ext_forces"], a["ext_forces"]) and "forces" not in eo
    # switched off again: what a fresh engine computes
    after = hip_engine.eval(*args, forces=True, coulomb="simple")
    fresh = HipEngine(loader.synthetic_spec(0), "cuda:0").eval(*args, forces=True, coulomb="simple")
    assert _same_bits(after, fresh) and "embedding_energy" not in after
    # the tangent sweep does not carry the term: refused while an embedding is set
    s = _lib.Embedding(n_ext=0, scratch=hip_engine._emb_scratch.data_ptr(), scratch_bytes=hip_engine._emb_scratch.numel())
    import ctypes as C

    assert hip_engine.lib.aimnet_engine_set_embedding(hip_engine._h, C.byref(s)) == 0
    try:
        with pytest.raises(_lib.HipLibraryError, match="embedding"):
            hip_engine.hvp(*args, torch.zeros(1, n, 3, device="cuda"))
    finally:
        assert hip_engine.lib.aimnet_engine_set_embedding(hip_engine._h, None) == 0
    assert hip_engine.hvp(*args, torch.zeros(1, n, 3, device="cuda"))["hv"].abs().max().item() == 0.0


def test_through_the_calculator(hip_engine):
    from aimnetcentral_amd import AIMNet2Calculator, loader

    g, n, mol, X, Q = _single("cold24")
    calc = AIMNet2Calculator(loader.synthetic_spec(0), device="cuda:0")
    out = calc({"coord": g["coord"], "numbers": g["numbers"], "charge": 0.0, "ext_coord": X, "ext_charge": Q}, forces=True)
    want = hip_engine.eval(*_args(hip_engine, g["coord"], g["numbers"], [0.0], mol), forces=True, coulomb=calc.coulomb_method or "none",
                           embedding=dict(ext_coord=_t(X), ext_charge=_t(Q), want_ext_forces=True))
    for k in ("energy", "forces", "charges", "embedding_energy", "ext_forces"):
        assert torch.equal(out[k], want[k]), k
    with pytest.raises(NotImplementedError):
        calc.hessian_vector_product({"coord": g["coord"], "numbers": g["numbers"], "charge": 0.0, "ext_coord": X, "ext_charge": Q},
                                    np.zeros((n, 3), np.float32))
