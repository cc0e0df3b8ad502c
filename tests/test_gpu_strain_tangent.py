"""Strain directions in the tangent sweep (csrc/hvp.hip armed by aimnet_engine_set_strain_tangent; HipEngine.hvp(..., strain=),
AIMNet2Calculator.strain_response / elastic_constants) against the fp64 reference of tests/strain_cases.py, on the smallest
shapes on which these kernels can go wrong (tests/tangent_cases.py): 18 atoms in 3 systems with their own triclinic 3 - 4.5 A
cells, lattice shifts of 2 and 3, atoms outside their box, short-range rows up to 90 (more than one 64-entry chunk) and long-range
rows up to 362 (more than 64 lanes); the same without a Coulomb term; an open axis; per-system flags; two channels, charged.

Gates (none is new): hv - tangent_cases.hv_gate (1e-5 + 3e-5 max|ref|); dvirial - the tangent_gate form 1e-5 + 3e-5 max|ref| per
system; the forces of the sweep - conftest.assert_forces_close; virial / V - STRESS_ATOL.  The two identities on the engine's own
numbers take those gates propagated through the identity (written where they are used).  Every comparison prints max|d|, its gate
and their ratio before it asserts."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import strain_cases as SC
import tangent_cases as T
from aimnetcentral_amd import _lib, capacity, elasticity
from conftest import FORCE_ATOL, FORCE_RTOL, STRESS_ATOL, assert_forces_close

pytestmark = pytest.mark.gpu


def _ratio(what, err, gate):
    err, gate = np.asarray(err, np.float64), np.asarray(gate, np.float64)
    r = float((err / gate).max()) if err.size else 0.0
    print(f"[strain-tangent] {what}: max|d| = {float(err.max()):.3e}, gate {float(gate.min()):.3e}, ratio {r:.3f}")
    assert (err <= gate).all(), f"{what}: ratio {r:.3f}"


def _engines(c, hip_engine, hip_engine_nse, oracle64, oracle64_nse):
    return (hip_engine_nse, oracle64_nse) if c.nse else (hip_engine, oracle64)


def _run(eng, c, V, EPS, **kw):
    out = eng.hvp(*T.engine_args(eng, c), T._t(V), want_forces=True, strain=None if EPS is None else T._t(EPS), **c.coul,
                  **T.cell_kwargs(c), **kw)
    return {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}


def _hv_gate(hv_ref) -> float:
    return T.hv_gate({"hv": hv_ref, "hv_d3": None})


def _dvirial_gate(dS_ref):
    """[n_mol]: the tangent_gate form per system, over the directions given."""
    return np.array([T.tangent_gate(dS_ref[:, m]) for m in range(dS_ref.shape[1])])


def _check_against_reference(tag, out, ref):
    r = ref["ref"]
    assert out["hv"].shape == ref["hv"].shape and out["dvirial"].shape == ref["dvirial"].shape
    assert out["virial"].shape == (r.n_mol, 3, 3)
    _ratio(f"{tag} hv", np.abs(out["hv"] - ref["hv"]).max(), _hv_gate(ref["hv"]))
    _ratio(f"{tag} dvirial", np.abs(out["dvirial"] - ref["dvirial"]).max(axis=(0, 2, 3)), _dvirial_gate(ref["dvirial"]))
    f_top = np.abs(ref["G"]).max()
    _ratio(f"{tag} forces of the sweep", np.abs(out["forces"] + ref["G"]).max(), FORCE_ATOL + FORCE_RTOL * f_top)
    assert_forces_close(out["forces"], -ref["G"], f"{tag} (forces of the sweep)")
    vol = r.volume[:, None, None]
    _ratio(f"{tag} virial / V", np.abs(out["virial"] - ref["S"]).max(axis=(1, 2)) / r.volume, STRESS_ATOL)
    assert np.abs(out["virial"] / vol - ref["S"] / vol).max() <= STRESS_ATOL


def _check_identities(tag, out, ref):
    """The engine's own numbers in the two exact identities.  Every quantity in them is within its own gate of the exact one, so the
    residual is within the sum of those gates times the factors they are multiplied by:
      rotation   dG - G w:              gate_hv + max_b sum_a |w_ab| gate_F
                 dS - (S w + w^T S):    gate_dS + 2 max_b sum_a |w_ab| V STRESS_ATOL
      mixed      eps : dS(v) - sum v . dG(eps) - sum (v eps) . G  per system:
                                        sum|eps| gate_dS + sum_i |v_i|_1 gate_hv + sum_i |(v eps)_i|_1 gate_F"""
    r, V, E = ref["ref"], ref["V"], ref["EPS"]
    G, S = -out["forces"], out["virial"]
    g_hv, g_dS = _hv_gate(ref["hv"]), _dvirial_gate(ref["dvirial"])
    g_F = FORCE_ATOL + FORCE_RTOL * np.abs(ref["G"]).max()
    g_S = r.volume * STRESS_ATOL
    w = E[8]
    wn = np.abs(w).sum(0).max()
    _ratio(f"{tag} rotation, dG - G w", np.abs(out["hv"][8] - G @ w).max(), g_hv + wn * g_F)
    _ratio(f"{tag} rotation, dS - (S w + w^T S)", np.abs(out["dvirial"][8] - (S @ w + w.T @ S)).max(axis=(1, 2)), g_dS + 2 * wn * g_S)
    mol = r.case.mol
    for k in range(6):  # displacement direction 7 against the Voigt strains (v = 0)
        res = SC.mixed_residual(mol, r.n_mol, G, V[7], E[k], out["dvirial"][7], out["hv"][k])
        gate = np.abs(E[k]).sum() * g_dS + r.per_system(np.abs(V[7]).sum(-1)) * g_hv + r.per_system(np.abs(V[7] @ E[k]).sum(-1)) * g_F
        _ratio(f"{tag} mixed derivative, strain {k}", np.abs(res), gate)


@pytest.mark.parametrize("name", SC.CASES)
def test_strain_directions(name, hip_engine, hip_engine_nse, oracle64, oracle64_nse):
    c = SC.case(name)
    eng, om = _engines(c, hip_engine, hip_engine_nse, oracle64, oracle64_nse)
    ref = SC.reference(name, om)
    out = _run(eng, c, ref["V"], ref["EPS"])
    if name == "tiny2-flags":  # small enough for the exact-fp32 GEMMs
        assert len(c.numbers) * (1 + len(ref["V"])) <= T.SPLIT_GEMM_ROWS
    _check_against_reference(name, out, ref)
    _check_identities(name, out, ref)
    # the same bits again, and unarmed the pure displacement is what hvp always returned
    again = _run(eng, c, ref["V"], ref["EPS"])
    assert all(np.array_equal(out[k], again[k]) for k in out)
    plain = _run(eng, c, ref["V"][7:8], None)
    assert set(plain) == {"hv", "forces"}
    _ratio(f"{name} unarmed hvp of the displacement", np.abs(plain["hv"][0] - ref["hv"][7]).max(), _hv_gate(ref["hv"][7:8]))


def _with_unit_displacements(oracle64):
    """tiny3-dsf8: its 54 unit displacements (reference: the fp64 tangent sweep, tangent_cases.reference) in front of the nine
    directions of strain_cases - 18 + 63 x 18 = 1 152 stacked rows, the split GEMMs."""
    c = SC.case("tiny3-dsf8")
    ref = SC.reference("tiny3-dsf8", oracle64)
    n = len(c.numbers)
    assert c.V.shape == (3 * n, n, 3)
    V = np.concatenate([c.V.astype(np.float64), ref["V"]])
    E = np.concatenate([np.zeros((3 * n, 3, 3)), ref["EPS"]])
    assert n * (1 + len(V)) > T.SPLIT_GEMM_ROWS
    return c, ref, V, E, T.reference(c, oracle64)["hv"]


@pytest.mark.parametrize("mode", [0, 2])
def test_many_directions_in_both_gemm_modes(mode, hip_engine, oracle64):
    """The exact-fp32 GEMMs everywhere (0) and the split GEMMs at every size (2): the same gates."""
    c, ref, V, E, hess = _with_unit_displacements(oracle64)
    n = len(c.numbers)
    before = hip_engine.get_option("gemm_bf3")
    hip_engine.set_option("gemm_bf3", mode)
    try:
        out = _run(hip_engine, c, V, E)
    finally:
        hip_engine.set_option("gemm_bf3", before)
    tag = f"tiny3-dsf8 + 54 unit displacements, gemm_bf3={mode}"
    _ratio(f"{tag} hv of the displacements", np.abs(out["hv"][: 3 * n] - hess).max(), _hv_gate(hess))
    tail = {k: (v[3 * n :] if k in ("hv", "dvirial") else v) for k, v in out.items()}
    _check_against_reference(tag, tail, ref)
    _check_identities(tag, tail, ref)


def test_split_sweeps_carry_their_slices(hip_engine, oracle64, monkeypatch):
    """HVP_BYTES_BUDGET lowered to 21 directions per sweep: the 63 directions go in three sweeps, each armed with its slice of the
    strains and of dvirial, each above 256 stacked rows like the single sweep (18 + 21 x 18 = 396: the same GEMM family) - the
    same values.  The size query sees the armed state."""
    c, ref, V, E, _ = _with_unit_displacements(oracle64)
    n, n_mol, K = len(c.numbers), len(c.charge), len(V)
    single = _run(hip_engine, c, V, E)
    rq = capacity.Request("hvp", n, n_mol, True, _lib.COULOMB_DSF, float(c.coul["dsf_rc"]), float(c.coul["dsf_alpha"]))
    opt = hip_engine.fill_options(rq)
    ws = lambda k: int(hip_engine.lib.aimnet_engine_hvp_workspace_bytes(hip_engine._h, n, n_mol, k, C.byref(opt)))  # noqa: E731
    unarmed, unarmed_one = ws(2) - ws(1), ws(1)
    _lib.check(hip_engine.lib.aimnet_engine_set_strain_tangent(hip_engine._h, C.byref(_lib.StrainTangent())), "arm")
    try:
        armed, armed_one = ws(2) - ws(1), ws(1)
    finally:
        hip_engine.lib.aimnet_engine_set_strain_tangent(hip_engine._h, None)
    # 36 bytes per direction and atom, 36 per atom (each of the two buffers rounded up to 256 bytes)
    assert abs(armed - unarmed - 36 * n) < 256 and ws(1) == unarmed_one
    assert 0 <= armed_one - unarmed_one - capacity.strain_tangent_bytes(n, 1) < 256
    per_sweep = 21
    assert -(-K // per_sweep) >= 3 and n * (1 + per_sweep) > T.SPLIT_GEMM_ROWS
    monkeypatch.setattr(hip_engine, "HVP_BYTES_BUDGET", armed * per_sweep + armed // 2)
    split = _run(hip_engine, c, V, E)
    monkeypatch.undo()
    for k in single:
        d = np.abs(single[k] - split[k]).max()
        print(f"[strain-tangent] three sweeps against one, {k}: max|d| = {d:.3e}")
        assert np.array_equal(single[k], split[k]), f"{k} changes with the split into sweeps"


def _refused(eng, c, match, **kw):
    V, E = SC.directions("tiny3-dsf8")
    with pytest.raises(_lib.HipLibraryError, match=match):
        eng.hvp(*T.engine_args(eng, c), T._t(V[:2]), strain=T._t(E[:2]), **kw)
    # no state leaks: a normal call right after works and is what it was
    d = SC.case("tiny3-dsf8")
    plain = eng.hvp(*T.engine_args(eng, d), T._t(V[7:8]), **d.coul, **T.cell_kwargs(d))
    assert set(plain) == {"hv"} and bool(torch.isfinite(plain["hv"]).all())
    return plain["hv"]


def test_refusals_leave_no_state(hip_engine, oracle64):
    eng = hip_engine
    c = SC.case("tiny3-dsf8")
    n = len(c.numbers)
    V, E = SC.directions("tiny3-dsf8")
    base = eng.hvp(*T.engine_args(eng, c), T._t(V[7:8]), **c.coul, **T.cell_kwargs(c))["hv"]
    cellkw = T.cell_kwargs(c)
    # no cell (the same atoms as one open cluster per system)
    assert torch.equal(base, _refused(eng, c, "strain tangent: a strain direction needs a cell", coulomb="none"))
    # Ewald and (with the mesh armed) PME
    assert torch.equal(base, _refused(eng, c, "strain tangent: Ewald summation is not carried", coulomb="ewald", **cellkw))
    assert torch.equal(base, _refused(eng, c, "strain tangent: particle-mesh Ewald is not carried", coulomb="pme", pme_tangent=True,
                                      **cellkw))
    # DFT-D3, finite-difference and analytic block
    eng.set_dftd3_tables(T.d3_tables())
    for armed in (False, True):
        assert torch.equal(base, _refused(eng, c, "strain tangent: the DFT-D3 block is not carried", dftd3=T._d3(9.0), d3_tangent=armed,
                                          **c.coul, **cellkw))
    # an embedding (a per-atom potential: the form a periodic input takes)
    emb = dict(potential=torch.zeros(n), potential_grad=torch.zeros(n, 3), potential_hess=torch.zeros(n, 6))
    assert torch.equal(base, _refused(eng, c, "strain tangent: the embedding term is not carried", embedding=emb, **c.coul, **cellkw))
    # armed by hand without arrays, and the charge response of an armed engine
    args = T.engine_args(eng, c)
    _lib.check(eng.lib.aimnet_engine_set_strain_tangent(eng._h, C.byref(_lib.StrainTangent())), "arm")
    try:
        with pytest.raises(_lib.HipLibraryError, match="strain tangent: strain and dvirial are required"):
            eng.hvp(*args, T._t(V[7:8]), **c.coul, **cellkw)
        with pytest.raises(_lib.HipLibraryError, match="charge_response: a strain tangent is armed"):
            eng.charge_response(*args, T._t(V[7:8]), **cellkw)
    finally:
        eng.lib.aimnet_engine_set_strain_tangent(eng._h, None)
    assert torch.equal(base, eng.hvp(*args, T._t(V[7:8]), **c.coul, **cellkw)["hv"])
    assert "dq" in eng.charge_response(*args, T._t(V[7:8]), **cellkw)
    with pytest.raises(ValueError, match="strain must have shape"):
        eng.hvp(*args, T._t(V[:2]), strain=T._t(E[:3]), **c.coul, **cellkw)


def test_calculator_strain_response_and_elastic_constants(oracle64):
    """The one-system tiny cell (tiny1-TTF: an open axis) through the calculator, DSF at the case's cutoff."""
    from aimnetcentral_amd import loader
    from aimnetcentral_amd.calculator import AIMNet2Calculator

    name = "tiny1-TTF"
    c = SC.case(name)
    ref = SC.reference(name, oracle64)
    r, n = ref["ref"], len(c.numbers)
    vol = float(r.volume[0])
    calc = AIMNet2Calculator(loader.synthetic_spec(0), device="cuda:0")
    calc.set_lrcoulomb_method("dsf", cutoff=c.coul["dsf_rc"], dsf_alpha=c.coul["dsf_alpha"])
    data = dict(coord=c.coord, numbers=c.numbers, charge=float(c.charge[0]), cell=c.cell, pbc=c.pbc)
    out = calc.strain_response(data, ref["EPS"].astype(np.float32), vectors=ref["V"].astype(np.float32))
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}
    _ratio(f"{name} strain_response force_derivative", np.abs(got["force_derivative"] + ref["hv"]).max(), _hv_gate(ref["hv"]))
    S, dS = ref["S"][0], ref["dvirial"][:, 0]
    tr = np.trace(ref["EPS"], axis1=1, axis2=2)
    want = (dS - S[None] * tr[:, None, None]) / vol
    # (dS within its gate, S / V within STRESS_ATOL, and the float32 of the result)
    gate = _dvirial_gate(ref["dvirial"])[0] / vol + np.abs(tr).max() * STRESS_ATOL + 2.0**-23 * np.abs(want).max()
    _ratio(f"{name} strain_response stress_derivative", np.abs(got["stress_derivative"] - want).max(), gate)
    _ratio(f"{name} strain_response stress", np.abs(got["stress"] - S / vol).max(), STRESS_ATOL)
    assert_forces_close(got["forces"], -ref["G"], f"{name} strain_response")

    ec = calc.elastic_constants(data)
    hess = T.reference(T.case(name), oracle64)["hv"].reshape(3 * n, 3 * n)  # (the case's own directions are the 3N unit vectors)
    want_ec = elasticity.elastic_tensors(hess, ref["hv"][:6], dS[:6], S, vol)
    g_hv_L, g_hv_H, g_dS = _hv_gate(ref["hv"][:6]), _hv_gate(hess), T.tangent_gate(dS[:6])
    # born_IJ = (1/V) e_I : (dS_J - e_J^T S): sum|e_I| = 1 and sum_c |e_J|_ca <= 1
    g_born = (g_dS + vol * STRESS_ATOL) / vol
    _ratio(f"{name} elastic_constants born", np.abs(ec["born"] - want_ec["born"]).max(), g_born)
    _ratio(f"{name} elastic_constants internal_strain", np.abs(ec["internal_strain"] - want_ec["internal_strain"]).max(), g_hv_L)
    _ratio(f"{name} elastic_constants hessian", np.abs(ec["hessian"] - want_ec["hessian"]).max(), g_hv_H)
    # relaxed = born - L^T H^+ L / V; to first order d(L^T H^+ L)_IJ = dL_I . u_J + u_I . dL_J - u_I^T dH u_J with u = H^+ L, so
    # elementwise errors within the gates give |.| <= g_L (|u_I|_1 + |u_J|_1) + g_H |u_I|_1 |u_J|_1
    Q = elasticity.translation_complement(n)
    L = want_ec["internal_strain"].reshape(3 * n, 6)
    u1 = np.abs(Q @ np.linalg.solve(Q.T @ want_ec["hessian"].reshape(3 * n, 3 * n) @ Q, Q.T @ L)).sum(0)
    g_rel = g_born + (g_hv_L * (u1[:, None] + u1[None, :]) + g_hv_H * u1[:, None] * u1[None, :]) / vol
    _ratio(f"{name} elastic_constants relaxed", np.abs(ec["relaxed"] - want_ec["relaxed"]), g_rel)
    assert ec["volume"] == pytest.approx(vol, rel=1e-6)
