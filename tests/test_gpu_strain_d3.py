"""The DFT-D3 block under strain (csrc/d3.hip: the STRAIN instantiations of d3_tcn / d3_tpair / d3_tcnforce; armed by
aimnet_engine_set_strain_terms beside the strain tangent and the analytic block - HipEngine.hvp(..., strain=, dftd3=, d3_tangent=True,
strain_terms=("dftd3",)), AIMNet2Calculator.strain_response / elastic_constants after set_dftd3_hessian("analytic")).

Directions as tests/strain_cases.py: six Voigt strains, one non-symmetric strain with a random v, one displacement, one rotation -
K = 9 is two full groups of four directions and a partial one.
  1. the block ALONE (aimnet_debug_dftd3_tangent) on het27 / par12, par9, par10 and het27x2 / par12 of tests/d3_cases.py (27 and 54 atoms,
     rows 640 wide, lattice shifts +-2, two cells with their own virial, N % 4 = 3): hv and dvirial against
     tests/d3_strain_yardstick.py at GATE_HV / GATE_DS, the forces and virial / V against d3_cases.d3_reference at FORCE_GATE /
     STRESS_GATE; the same call twice and K = 9 as 9, 4 + 5 and 9 x 1 are bit for bit equal (the block has no GEMM);
  2. the whole sweep on tiny3-dsf8-d3 (18 atoms, three triclinic 3 - 4.5 A cells, D3 rows 354 wide, shifts up to +-3) against
     strain_cases.reference("tiny3-dsf8") + the yardstick, the two identities on the engine's own numbers, and an unarmed call afterwards;
  3. refusals, state and workspace;
  4. the calculator on tiny1-TTF with the term at 9 A.
Every comparison prints max|d|, its gate and their ratio before it asserts."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import d3_cases as D
import d3_strain_yardstick as SY
import strain_cases as SC
import tangent_cases as T
from aimnetcentral_amd import _lib, capacity, elasticity
from conftest import FORCE_ATOL, FORCE_RTOL, STRESS_ATOL, assert_forces_close

pytestmark = pytest.mark.gpu

TERMS = ("dftd3",)
DEVICE_ERRORS = ("HIP error", "hipError", "illegal memory", "kernel launch failed", "code -2")


def _ratio(what, err, gate):
    err, gate = np.asarray(err, np.float64), np.asarray(gate, np.float64)
    r = float((err / gate).max()) if err.size else 0.0
    print(f"[strain-d3] {what}: max|d| = {float(err.max()):.3e}, gate {float(gate.min()):.3e}, ratio {r:.3f}")
    assert (err <= gate).all(), f"{what}: ratio {r:.3f}"


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _guard(call, what):
    try:
        return call()
    except RuntimeError as exc:  # nothing more is started on a GPU that has faulted
        if any(s in str(exc) for s in DEVICE_ERRORS):
            pytest.exit(f"device error in {what}: {exc}", returncode=3)
        raise


def block(eng, c, par, V, EPS):
    """The armed block alone under strain: hv, forces (float32), dvirial, virial (float64) as numpy arrays."""
    dev = eng.device
    eng.set_dftd3_tables(D.tables())
    args = (torch.from_numpy(c.coord).to(dev), torch.from_numpy(c.numbers.astype(np.int32)).to(dev),
            torch.from_numpy(c.mol.astype(np.int32)).to(dev), torch.from_numpy(c.charge).to(dev))
    out = _guard(lambda: eng.hvp(*args, torch.from_numpy(np.ascontiguousarray(V, np.float32)).to(dev), coulomb="none", dftd3=D.get_par(par),
                                 want_forces=True, d3_tangent=True, _d3_block_only=True, cell=torch.from_numpy(c.cell).to(dev),
                                 strain=torch.from_numpy(np.ascontiguousarray(EPS, np.float32)).to(dev), strain_terms=TERMS),
                 f"the D3 block under strain of {c.name}")
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- 1. the block alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,par", SY.HELD[:4])
def test_block_alone_meets_the_yardstick(hip_engine_cold, name, par):
    c, p = SY.held(name, par)
    V, E = SY.directions(c)
    ref = SY.yardstick(c, p, V, E)
    out = block(hip_engine_cold, c, par, V, E)
    n_mol = len(c.charge)
    assert out["hv"].shape == ref["hv"].shape and out["dvirial"].shape == (9, n_mol, 3, 3) and out["virial"].shape == (n_mol, 3, 3)
    assert out["dvirial"].dtype == np.float64 and out["virial"].dtype == np.float64
    _ratio(f"block {name}/{par} hv", np.abs(out["hv"].astype(np.float64) - ref["hv"]).max(), SY.GATE_HV * np.abs(ref["hv"]).max())
    _ratio(f"block {name}/{par} dvirial", np.abs(out["dvirial"] - ref["dS"]).max(axis=(0, 2, 3)), SY.GATE_DS * np.abs(ref["dS"]).max(axis=(0, 2, 3)))
    f = D.d3_reference(c, torch.float64, par=par)
    _ratio(f"block {name}/{par} forces", np.abs(out["forces"].astype(np.float64) - f["forces"]).max(), D.FORCE_GATE)
    vol = np.abs(np.linalg.det(np.asarray(c.cell, np.float64).reshape(-1, 3, 3)))
    _ratio(f"block {name}/{par} virial / V", np.abs(out["virial"] / vol[:, None, None] - f["stress"]).max(axis=(1, 2)), D.STRESS_GATE)
    again = block(hip_engine_cold, c, par, V, E)
    assert all(bits_equal(out[k], again[k]) for k in out), "the same call twice differs"


@pytest.mark.parametrize("name,par", [("het27", "par12"), ("het27x2", "par12")])
def test_grouping_changes_no_bit(hip_engine_cold, name, par):
    """K = 9 as one call, as 4 + 5 and as nine single calls."""
    c, p = SY.held(name, par)
    V, E = SY.directions(c)
    whole = block(hip_engine_cold, c, par, V, E)
    parts = {"4 + 5": [slice(0, 4), slice(4, 9)], "9 x 1": [slice(k, k + 1) for k in range(9)]}
    for what, slices in parts.items():
        outs = [block(hip_engine_cold, c, par, V[s], E[s]) for s in slices]
        for key in ("hv", "dvirial"):
            other = np.concatenate([o[key] for o in outs])
            d = np.abs(whole[key].astype(np.float64) - other).max()
            print(f"[strain-d3] bits {name} K = 9 against {what}, {key}: max|d| {d:.2e}")
            assert bits_equal(whole[key], other), f"{name}: {key} of K = 9 against {what} differs by {d:.3e}"
        assert all(bits_equal(o["virial"], whole["virial"]) and bits_equal(o["forces"], whole["forces"]) for o in outs)


# ---- 2. the whole sweep ---------------------------------------------------------------------------------------------------------------
def _sweep(eng, c, V, EPS, **kw):
    out = _guard(lambda: eng.hvp(*T.engine_args(eng, c), T._t(V), want_forces=True, strain=None if EPS is None else T._t(EPS), **c.coul,
                                 **T.cell_kwargs(c), **kw), f"the sweep of {c.name}")
    return {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}


def test_whole_sweep_with_the_term(hip_engine, oracle64):
    eng = hip_engine
    c, plain_case = T.case("tiny3-dsf8-d3"), SC.case("tiny3-dsf8")
    assert np.array_equal(c.coord, plain_case.coord) and np.array_equal(c.numbers, plain_case.numbers)
    assert np.array_equal(c.cell, plain_case.cell) and np.array_equal(c.mol, plain_case.mol) and c.coul == plain_case.coul
    base = SC.reference("tiny3-dsf8", oracle64)
    V, E = base["V"], base["EPS"]
    Vy, Ey = SY.directions(c)
    assert np.array_equal(V, Vy) and np.array_equal(E, Ey)
    d3 = SY.yardstick(c, c.d3, V, E)
    r = base["ref"]
    ref = {"hv": base["hv"] + d3["hv"], "dS": base["dvirial"] + d3["dS"], "G": base["G"] + d3["G"], "S": base["S"] + d3["S"]}
    eng.set_dftd3_tables(T.d3_tables())
    before = _sweep(eng, plain_case, V[7:8], None)
    out = _sweep(eng, c, V, E, dftd3=c.d3, d3_tangent=True, strain_terms=TERMS)
    g_hv = 1e-5 + 3e-5 * np.abs(ref["hv"]).max() + SY.GATE_HV * np.abs(d3["hv"]).max()
    g_dS = np.array([T.tangent_gate(ref["dS"][:, m]) + SY.GATE_DS * np.abs(d3["dS"][:, m]).max() for m in range(r.n_mol)])
    g_F = FORCE_ATOL + FORCE_RTOL * np.abs(ref["G"]).max()
    g_S = r.volume * STRESS_ATOL
    tag = "tiny3-dsf8-d3"
    _ratio(f"{tag} hv", np.abs(out["hv"] - ref["hv"]).max(), g_hv)
    _ratio(f"{tag} dvirial", np.abs(out["dvirial"] - ref["dS"]).max(axis=(0, 2, 3)), g_dS)
    _ratio(f"{tag} forces of the sweep", np.abs(out["forces"] + ref["G"]).max(), g_F)
    assert_forces_close(out["forces"], -ref["G"], f"{tag} (forces of the sweep)")
    _ratio(f"{tag} virial / V", np.abs(out["virial"] - ref["S"]).max(axis=(1, 2)) / r.volume, STRESS_ATOL)
    # the block's own share: the sweep without the term shares every other launch
    without = _sweep(eng, plain_case, V, E)
    _ratio(f"{tag} hv share of the block", np.abs((out["hv"] - without["hv"]) - d3["hv"]).max(),
           SY.GATE_HV * np.abs(d3["hv"]).max() + 2.0**-22 * np.abs(ref["hv"]).max())
    _ratio(f"{tag} dvirial share of the block", np.abs((out["dvirial"] - without["dvirial"]) - d3["dS"]).max(axis=(0, 2, 3)),
           SY.GATE_DS * np.abs(d3["dS"]).max(axis=(0, 2, 3)) + 2.0**-22 * np.abs(ref["dS"]).max(axis=(0, 2, 3)))
    # the two identities on the engine's own numbers, the gates propagated as in tests/test_gpu_strain_tangent.py
    G, S = -out["forces"], out["virial"]
    w = E[8]
    wn = np.abs(w).sum(0).max()
    _ratio(f"{tag} rotation, dG - G w", np.abs(out["hv"][8] - G @ w).max(), g_hv + wn * g_F)
    _ratio(f"{tag} rotation, dS - (S w + w^T S)", np.abs(out["dvirial"][8] - (S @ w + w.T @ S)).max(axis=(1, 2)), g_dS + 2 * wn * g_S)
    for k in range(6):
        res = SC.mixed_residual(r.case.mol, r.n_mol, G, V[7], E[k], out["dvirial"][7], out["hv"][k])
        gate = np.abs(E[k]).sum() * g_dS + r.per_system(np.abs(V[7]).sum(-1)) * g_hv + r.per_system(np.abs(V[7] @ E[k]).sum(-1)) * g_F
        _ratio(f"{tag} mixed derivative, strain {k}", np.abs(res), gate)
    again = _sweep(eng, c, V, E, dftd3=c.d3, d3_tangent=True, strain_terms=TERMS)
    assert all(np.array_equal(out[k], again[k]) for k in out)
    after = _sweep(eng, plain_case, V[7:8], None)
    assert set(after) == {"hv", "forces"} and all(np.array_equal(before[k], after[k]) for k in before), "an unarmed call changed"


# ---- 3. refusals, state, workspace ----------------------------------------------------------------------------------------------------
def test_refusals_and_state(hip_engine):
    eng = hip_engine
    c, plain_case = T.case("tiny3-dsf8-d3"), SC.case("tiny3-dsf8")
    V, E = SC.directions("tiny3-dsf8")
    eng.set_dftd3_tables(T.d3_tables())
    args, cellkw = T.engine_args(eng, c), T.cell_kwargs(c)
    plain = lambda: eng.hvp(*args, T._t(V[7:8]), **plain_case.coul, **cellkw)["hv"]  # noqa: E731
    base = plain()
    with pytest.raises(_lib.HipLibraryError, match="carried under strain by its analytic tangent only"):
        eng.hvp(*args, T._t(V[:2]), strain=T._t(E[:2]), dftd3=c.d3, d3_tangent=False, strain_terms=TERMS, **c.coul, **cellkw)
    assert torch.equal(base, plain())
    for armed in (False, True):
        with pytest.raises(_lib.HipLibraryError, match="strain tangent: the DFT-D3 block is not carried"):
            eng.hvp(*args, T._t(V[:2]), strain=T._t(E[:2]), dftd3=c.d3, d3_tangent=armed, **c.coul, **cellkw)
        assert torch.equal(base, plain())
    with pytest.raises(ValueError, match="unknown strain term"):
        eng.hvp(*args, T._t(V[:2]), strain=T._t(E[:2]), dftd3=c.d3, d3_tangent=True, strain_terms=("ewald",), **c.coul, **cellkw)
    with pytest.raises(ValueError, match="needs strain"):
        eng.hvp(*args, T._t(V[:2]), dftd3=c.d3, d3_tangent=True, strain_terms=TERMS, **c.coul, **cellkw)
    assert torch.equal(base, plain())
    # the mask: unknown bits are refused, NULL clears it, a struct leaves it
    lib, h = eng.lib, eng._h
    assert lib.aimnet_engine_set_strain_terms(h, 2) == _lib.E_INVALID and lib.aimnet_engine_set_strain_terms(h, 1) == 0
    try:
        _lib.check(lib.aimnet_engine_set_strain_tangent(h, C.byref(_lib.StrainTangent())), "arm")
        _lib.check(lib.aimnet_engine_set_dftd3_tangent(h, 1), "arm the block")
        # (armed without arrays and with the term named: the D3 check is passed, the arrays are what is missing)
        with pytest.raises(_lib.HipLibraryError, match="strain tangent: strain and dvirial are required"):
            eng.hvp(*args, T._t(V[7:8]), dftd3=c.d3, **c.coul, **cellkw)
    finally:
        lib.aimnet_engine_set_dftd3_tangent(h, 0)
        lib.aimnet_engine_set_strain_tangent(h, None)
    _lib.check(lib.aimnet_engine_set_strain_tangent(h, C.byref(_lib.StrainTangent())), "arm")
    try:  # NULL above cleared the mask: armed again, the old refusal is back
        with pytest.raises(_lib.HipLibraryError, match="strain tangent: the DFT-D3 block is not carried"):
            eng.hvp(*args, T._t(V[7:8]), dftd3=c.d3, **c.coul, **cellkw)
    finally:
        lib.aimnet_engine_set_strain_tangent(h, None)
    assert torch.equal(base, plain())


def test_no_workspace_of_its_own(hip_engine):
    eng = hip_engine
    c = T.case("tiny3-dsf8-d3")
    n, n_mol, K = len(c.numbers), len(c.charge), 9
    eng.set_dftd3_tables(T.d3_tables())
    V, E = SC.directions("tiny3-dsf8")
    _sweep(eng, c, V, E, dftd3=c.d3, d3_tangent=True, strain_terms=TERMS)  # settles the row capacities
    lib, h = eng.lib, eng._h
    sizes = {}
    try:
        for d3 in (False, True):
            rq = capacity.Request("hvp", n, n_mol, True, _lib.COULOMB_DSF, float(c.coul["dsf_rc"]), float(c.coul["dsf_alpha"]), 1e-6,
                                  c.d3 if d3 else None)
            opt = eng.fill_options(rq)
            _lib.check(lib.aimnet_engine_set_dftd3_tangent(h, int(d3)), "aimnet_engine_set_dftd3_tangent")
            for strain in (False, True):
                if strain:
                    _lib.check(lib.aimnet_engine_set_strain_tangent(h, C.byref(_lib.StrainTangent())), "arm")
                    _lib.check(lib.aimnet_engine_set_strain_terms(h, int(d3)), "terms")
                sizes[d3, strain] = int(lib.aimnet_engine_hvp_workspace_bytes(h, n, n_mol, K, C.byref(opt)))
                lib.aimnet_engine_set_strain_tangent(h, None)
    finally:
        lib.aimnet_engine_set_strain_tangent(h, None)
        lib.aimnet_engine_set_dftd3_tangent(h, 0)
    with_d3, without = sizes[True, True] - sizes[True, False], sizes[False, True] - sizes[False, False]
    print(f"[strain-d3] workspace: {sizes} | strain adds {with_d3} with the armed block, {without} without the term")
    assert without > 0 and abs(with_d3 - without) < 256
    assert 0 <= without - capacity.strain_tangent_bytes(n, K) < 512


# ---- 4. the calculator ----------------------------------------------------------------------------------------------------------------
def test_calculator_with_the_external_term(oracle64):
    from aimnetcentral_amd import loader
    from aimnetcentral_amd.calculator import AIMNet2Calculator

    name = "tiny1-TTF"
    c = SC.case(name)
    p = T._d3(9.0)
    base = SC.reference(name, oracle64)
    V, E = base["V"], base["EPS"]
    d3 = SY.yardstick(c, p, V, E)
    n = len(c.numbers)
    vol = float(base["ref"].volume[0])
    hv_ref, dS_ref = base["hv"] + d3["hv"], (base["dvirial"] + d3["dS"])[:, 0]
    G_ref, S_ref = base["G"] + d3["G"], (base["S"] + d3["S"])[0]
    spec = loader.synthetic_spec(0)
    spec.metadata = dict(spec.metadata, needs_dispersion=True, d3_params={k: p[k] for k in ("s6", "s8", "a1", "a2")})
    calc = AIMNet2Calculator(spec, device="cuda:0", dftd3_data=T.d3_tables())
    calc.set_dftd3_cutoff(p["cutoff"], p["smoothing_fraction"])
    calc.set_lrcoulomb_method("dsf", cutoff=c.coul["dsf_rc"], dsf_alpha=c.coul["dsf_alpha"])
    data = dict(coord=c.coord, numbers=c.numbers, charge=float(c.charge[0]), cell=c.cell, pbc=c.pbc)
    with pytest.raises(NotImplementedError, match="set_dftd3_hessian"):
        calc.strain_response(data, E.astype(np.float32))
    calc.set_dftd3_hessian("analytic")
    out = _guard(lambda: calc.strain_response(data, E.astype(np.float32), vectors=V.astype(np.float32)), "strain_response")
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}
    g_hv = 1e-5 + 3e-5 * np.abs(hv_ref).max() + SY.GATE_HV * np.abs(d3["hv"]).max()
    g_dS = T.tangent_gate(dS_ref) + SY.GATE_DS * np.abs(d3["dS"]).max()
    _ratio(f"{name} strain_response force_derivative", np.abs(got["force_derivative"] + hv_ref).max(), g_hv)
    tr = np.trace(E, axis1=1, axis2=2)
    want = (dS_ref - S_ref[None] * tr[:, None, None]) / vol
    gate = g_dS / vol + np.abs(tr).max() * STRESS_ATOL + 2.0**-23 * np.abs(want).max()
    _ratio(f"{name} strain_response stress_derivative", np.abs(got["stress_derivative"] - want).max(), gate)
    _ratio(f"{name} strain_response stress", np.abs(got["stress"] - S_ref / vol).max(), STRESS_ATOL)
    assert_forces_close(got["forces"], -G_ref, f"{name} strain_response")

    ec = _guard(lambda: calc.elastic_constants(data), "elastic_constants")
    units = np.eye(3 * n).reshape(3 * n, n, 3)
    h_d3 = SY.yardstick(c, p, units, np.zeros((3 * n, 3, 3)))["hv"].reshape(3 * n, 3 * n)
    hess = T.reference(T.case(name), oracle64)["hv"].reshape(3 * n, 3 * n) + h_d3
    want_ec = elasticity.elastic_tensors(hess, hv_ref[:6], dS_ref[:6], S_ref, vol)
    g_hv_L = 1e-5 + 3e-5 * np.abs(hv_ref[:6]).max() + SY.GATE_HV * np.abs(d3["hv"][:6]).max()
    g_hv_H = 1e-5 + 3e-5 * np.abs(hess).max() + SY.GATE_HV * np.abs(h_d3).max()
    g_dS6 = T.tangent_gate(dS_ref[:6]) + SY.GATE_DS * np.abs(d3["dS"][:6]).max()
    g_born = (g_dS6 + vol * STRESS_ATOL) / vol
    _ratio(f"{name} elastic_constants born", np.abs(ec["born"] - want_ec["born"]).max(), g_born)
    _ratio(f"{name} elastic_constants internal_strain", np.abs(ec["internal_strain"] - want_ec["internal_strain"]).max(), g_hv_L)
    _ratio(f"{name} elastic_constants hessian", np.abs(ec["hessian"] - want_ec["hessian"]).max(), g_hv_H)
    Q = elasticity.translation_complement(n)
    L = want_ec["internal_strain"].reshape(3 * n, 6)
    u1 = np.abs(Q @ np.linalg.solve(Q.T @ want_ec["hessian"].reshape(3 * n, 3 * n) @ Q, Q.T @ L)).sum(0)
    g_rel = g_born + (g_hv_L * (u1[:, None] + u1[None, :]) + g_hv_H * u1[:, None] * u1[None, :]) / vol
    _ratio(f"{name} elastic_constants relaxed", np.abs(ec["relaxed"] - want_ec["relaxed"]), g_rel)
    assert ec["volume"] == pytest.approx(vol, rel=1e-6)
