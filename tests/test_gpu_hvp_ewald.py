"""Ewald summation in the analytic Hessian-vector sweep (csrc/hvp.hip: the real-space term over the long-range list;
csrc/ewald.hip: tangent structure factors and the per-atom tangent pass) against the dense Hessian the fp64 oracle gets by double
backward through its own Ewald sum (oracle.aimnet2_oracle.evaluate(..., coulomb="ewald", hessian=True)).

Fixtures: triclinic cells of 12 and 16 atoms, 6 and 7 A wide (`small_cell`).  At accuracy 1e-6 their real-space cutoffs (8.29 and
9.22 A) exceed every cell edge - the list holds several images of the same neighbour and shifted self pairs -, their k boxes (140
and 196 entries, 66 and 75 of them inside the half sphere) are no multiple of the 8 entries a structure-factor block takes and
hold more than the 64 entries a wave covers in one trip.  The Ewald block is 5.7 of 11.2 eV/A^2 (A) and 13.8 of 22.3 eV/A^2 (B) of
the largest Hessian element; the real-space term alone (DSF at the same alpha, r_c) is 0.86 / 7.7 eV/A^2 away from the full one.

Gate: the sweep's own, `_close` of tests/test_gpu_hvp.py - max|d| <= 1e-5 + 3e-5 max|ref| (3.5e-4 and 6.8e-4 eV/A^2 here); the fp32
oracle sits at 0.04 and 0.06 of it.  Every comparison prints its ratio to the gate before it asserts (profiles/r7_hvp_ewald.md)."""
from __future__ import annotations

import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

from conftest import assert_forces_close, golden

pytestmark = pytest.mark.gpu

ACC = 1e-6


def small_cell(seed, n, L, dmin=0.95):
    rng = np.random.default_rng(seed)
    cell = np.diag([L, 1.1 * L, 0.9 * L]); cell[1, 0] = 0.8; cell[2, 0] = -0.6; cell[2, 1] = 0.5
    inv, pts = np.linalg.inv(cell), []
    while len(pts) < n:
        x = rng.random(3) @ cell
        if all(np.linalg.norm(((x - p) @ inv - np.rint((x - p) @ inv)) @ cell) >= dmin for p in pts):
            pts.append(x)
    z = rng.choice([1, 6, 7, 8], size=n, p=[0.5, 0.3, 0.1, 0.1])
    return np.array(pts, np.float32), z.astype(np.int64), cell.astype(np.float32)


@functools.lru_cache(maxsize=None)
def cell_a():
    return small_cell(5, 12, 6.0)


@functools.lru_cache(maxsize=None)
def cell_b():
    return small_cell(5, 16, 7.0)


_REF: dict = {}


def oracle_ref(model, key, coord, numbers, charge, cell, **kw):
    """One oracle evaluation with the dense Hessian per (fixture, charge, options): computed once, shared, never modified."""
    from oracle import aimnet2_oracle as O

    if key not in _REF:
        r = O.evaluate(model, coord, numbers, np.atleast_1d(np.float32(charge)), cell=cell, hessian=True, **dict(dict(coulomb="ewald", ewald_accuracy=ACC), **kw))
        n = len(numbers)
        h = r["hessian"].reshape(3 * n, 3 * n)
        h.setflags(write=False)
        _REF[key] = (h, r["forces"])
    return _REF[key]


def _t(a, dt=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dt).cuda()


def _close(hv, ref, what):
    """`_close` of tests/test_gpu_hvp.py, with the ratio to the gate printed first"""
    err, top = np.abs(hv - ref).max(), np.abs(ref).max()
    gate = 1e-5 + 3e-5 * top
    print(f"[hvp-ewald] {what}: max|d| = {err:.3e} on max|ref| = {top:.3e}, gate {gate:.3e}, ratio {err / gate:.3f}")
    assert err <= gate, f"{what}: max|d(Hv)| = {err:.3e} on max|Hv| = {top:.3e}"


def _hvp(eng, coord, numbers, charge, cell, V, mol=None, **kw):
    n = len(numbers)
    mol = np.zeros(n, dtype=np.int64) if mol is None else mol
    return eng.hvp(_t(coord), _t(numbers, torch.int32), _t(mol, torch.int32), _t(charge), _t(V), cell=_t(cell), coulomb="ewald",
                   ewald_accuracy=ACC, **kw)


def _np64(t):
    return t.cpu().numpy().astype(np.float64)


def test_dense_hessian_of_a_small_cell(hip_engine, oracle64):
    """All 36 unit directions of cell A: the Hessian and the forces of the same sweep against the oracle; and the result is NOT the
    real-space term alone (the oracle's DSF Hessian at the same alpha, r_c is 0.86 eV/A^2 away: a dropped reciprocal part shows)."""
    from oracle import aimnet2_oracle as O

    c, z, cell = cell_a()
    H64, f64 = oracle_ref(oracle64, "A0", c, z, 0.0, cell)
    out = _hvp(hip_engine, c, z, [0.0], cell, np.eye(36, dtype=np.float32).reshape(36, 12, 3), want_forces=True)
    H = _np64(out["hv"]).reshape(36, 36)
    _close(H, H64, "case 1: dense Hessian of A")
    assert_forces_close(out["forces"].cpu().numpy(), f64, "A (forces of the sweep)")
    assert 140 <= int(hip_engine.last_status[7]) <= 144 and int(hip_engine.last_status[1]) > 12  # the k box; images in the list
    alpha, rc, _ = O.ewald_parameters(12, abs(np.linalg.det(cell.astype(np.float64))), ACC)
    Hdsf, _ = oracle_ref(oracle64, "A0dsf", c, z, 0.0, cell, coulomb="dsf", dsf_rc=rc, dsf_alpha=alpha)
    assert np.abs(H - Hdsf).max() > 1e-5 + 3e-5 * np.abs(Hdsf).max(), np.abs(H - Hdsf).max()  # outside the gate of the DSF Hessian


def test_charged_cell(hip_engine, oracle64):
    """B with charge +1 (neutralising background: a constant of the evaluation, no tangent)."""
    c, z, cell = cell_b()
    H64, f64 = oracle_ref(oracle64, "B+1", c, z, 1.0, cell)
    V = np.random.default_rng(11).standard_normal((3, 16, 3)).astype(np.float32)
    out = _hvp(hip_engine, c, z, [1.0], cell, V, want_forces=True)
    _close(_np64(out["hv"]).reshape(3, 48), V.reshape(3, 48).astype(np.float64) @ H64, "case 2: B, charge +1")
    assert_forces_close(out["forces"].cpu().numpy(), f64, "B +1 (forces of the sweep)")


def test_two_systems_with_their_own_parameters(hip_engine, oracle64):
    """A and B in one call, charges (0, -1): per-system (alpha, r_c, k box); the second system's k slice starts at entry 144."""
    ca, za, cella = cell_a()
    cb, zb, cellb = cell_b()
    Ha, fa = oracle_ref(oracle64, "A0", ca, za, 0.0, cella)
    Hb, fb = oracle_ref(oracle64, "B-1", cb, zb, -1.0, cellb)
    mol = np.concatenate([np.zeros(12, np.int64), np.ones(16, np.int64)])
    V = np.random.default_rng(11).standard_normal((3, 28, 3)).astype(np.float32)
    out = _hvp(hip_engine, np.concatenate([ca, cb]), np.concatenate([za, zb]), [0.0, -1.0], np.stack([cella, cellb]), V, mol=mol,
               want_forces=True)
    hv = _np64(out["hv"])
    _close(hv[:, :12].reshape(3, 36), V[:, :12].reshape(3, 36).astype(np.float64) @ Ha, "case 3: A of (A, B)")
    _close(hv[:, 12:].reshape(3, 48), V[:, 12:].reshape(3, 48).astype(np.float64) @ Hb, "case 3: B of (A, B), charge -1")
    f = out["forces"].cpu().numpy()
    assert_forces_close(f[:12], fa, "A of (A, B)")
    assert_forces_close(f[12:], fb, "B of (A, B)")
    assert int(hip_engine.last_status[7]) == 144 + 200


def test_two_charge_channels(hip_engine_nse, oracle64_nse):
    """Open-shell NSE model: the Coulomb term sees alpha + beta, both channels get the seed."""
    from oracle import aimnet2_oracle as O

    c, z, cell = small_cell(7, 12, 6.0)
    r = O.evaluate(oracle64_nse, c, z, np.array([1.0], np.float32), cell=cell, coulomb="ewald", ewald_accuracy=ACC, hessian=True,
                   mult=np.array([2.0], np.float32))
    H64 = r["hessian"].reshape(36, 36)
    V = np.random.default_rng(11).standard_normal((3, 12, 3)).astype(np.float32)
    out = _hvp(hip_engine_nse, c, z, [[1.0, 0.0]], cell, V, want_forces=True)  # (alpha, beta) of charge +1, multiplicity 2
    _close(_np64(out["hv"]).reshape(3, 36), V.reshape(3, 36).astype(np.float64) @ H64, "case 4: two channels, charge +1, doublet")
    assert_forces_close(out["forces"].cpu().numpy(), r["forces"], "NSE cell (forces of the sweep)")


def test_operator_properties(hip_engine):
    """Symmetry, translation invariance, bitwise repeatability, independence of how the directions are split into sweeps and of the
    capacities the sweep started from (k arrays and neighbour rows grow and the sweep repeats)."""
    c, z, cell = cell_a()
    args = (hip_engine, c, z, [0.0], cell)
    H = _hvp(*args, np.eye(36, dtype=np.float32).reshape(36, 12, 3))["hv"].view(36, 36)
    assert (H - H.T).abs().max().item() < 1e-5
    shift = np.zeros((3, 12, 3), np.float32)
    for a in range(3):
        shift[a, :, a] = 1.0
    assert _hvp(*args, shift)["hv"].abs().max().item() < 2e-4
    V = np.random.default_rng(2).standard_normal((5, 12, 3)).astype(np.float32)  # 5: one full group of 4 directions + a partial one
    hv = _hvp(*args, V)["hv"]
    assert torch.equal(hv, _hvp(*args, V)["hv"])
    assert (hv.view(5, 36) - _t(V).view(5, 36) @ H).abs().max().item() < 2e-4
    budget = hip_engine.HVP_BYTES_BUDGET
    try:  # one direction per sweep: identical numbers (a direction never sees another one)
        hip_engine.HVP_BYTES_BUDGET = 1
        assert torch.equal(hv, _hvp(*args, V)["hv"])
    finally:
        hip_engine.HVP_BYTES_BUDGET = budget
    old_k, old_nb = hip_engine._ewald_max_k, hip_engine.max_nb
    try:
        hip_engine._ewald_max_k = 64
        got = _hvp(*args, V)["hv"]
        assert hip_engine._ewald_max_k >= int(hip_engine.last_status[7]) > 64 and torch.equal(got, hv)
        hip_engine.max_nb = 16
        got = _hvp(*args, V)["hv"]
        assert hip_engine.max_nb > 16 and torch.equal(got, hv)
    finally:
        hip_engine._ewald_max_k = max(old_k, hip_engine._ewald_max_k)
        hip_engine.max_nb = max(old_nb, hip_engine.max_nb)


def _calculator(dftd3=None):
    from aimnetcentral_amd import AIMNet2Calculator, loader

    spec = loader.synthetic_spec(0)
    kw = {}
    if dftd3 is not None:
        par, tables = dftd3
        spec.metadata = dict(spec.metadata, needs_dispersion=True, d3_params={k: par[k] for k in ("s6", "s8", "a1", "a2")})
        kw["dftd3_data"] = tables
    calc = AIMNet2Calculator(spec, device="cuda:0", **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        calc.set_lrcoulomb_method("ewald", ewald_accuracy=ACC)
    return calc


def test_more_atoms_than_one_block_stride():
    """A (3, 3, 3) supercell of A, 324 atoms: the 256-thread atom loop of the structure-factor kernels takes a second trip.  The
    analytic operator against the calculator's own finite-difference one at the gate the project holds that pair to (structure
    only; the precision is pinned by the dense cases)."""
    c, z, cell = cell_a()
    reps = np.array([(i, j, k) for i in range(3) for j in range(3) for k in range(3)], dtype=np.float64)
    coord = (c[None].astype(np.float64) + (reps @ cell.astype(np.float64))[:, None]).reshape(-1, 3)
    coord = (coord + np.random.default_rng(3).normal(0.0, 0.02, coord.shape)).astype(np.float32)
    data = dict(coord=coord, numbers=np.tile(z, 27), charge=0.0, cell=(3.0 * cell).astype(np.float32))
    assert len(data["numbers"]) == 324
    calc = _calculator()
    v = np.random.default_rng(4).standard_normal((1, 324, 3)).astype(np.float32)
    hv = calc.hessian_vector_product(data, v).cpu().numpy()
    calc.hvp_method = "fd"
    fd = calc.hessian_vector_product(data, v).cpu().numpy()
    err, gate = np.abs(hv - fd).max(), 2e-3 * max(1.0, np.abs(fd).max())
    print(f"[hvp-ewald] case 6: 324 atoms, analytic vs fd: max|d| = {err:.3e}, gate {gate:.3e}, ratio {err / gate:.3f}")
    assert err < gate


def test_through_the_calculator(oracle64, monkeypatch):
    """set_lrcoulomb_method("ewald"): hessian_vector_product is the engine's sweep (bitwise), eval(hessian=True) the oracle's
    Hessian; "pme" still takes differences of forces (engine.hvp is not called)."""
    c, z, cell = cell_a()
    H64, _ = oracle_ref(oracle64, "A0", c, z, 0.0, cell)
    calc = _calculator()
    data = dict(coord=c, numbers=z, charge=0.0, cell=cell)
    V = np.random.default_rng(11).standard_normal((3, 12, 3)).astype(np.float32)
    hv = calc.hessian_vector_product(data, V)
    want = _hvp(calc.engine, c, z, [0.0], cell, V)["hv"]
    assert torch.equal(hv, want)
    out = calc(data, forces=True, hessian=True)
    _close(_np64(out["hessian"]).reshape(36, 36), H64, "case 7: calculator eval(hessian=True) on A")
    calls = []
    real = calc.engine.hvp
    monkeypatch.setattr(calc.engine, "hvp", lambda *a, **k: calls.append(k.get("coulomb")) or real(*a, **k))
    calc.hessian_vector_product(data, V[:1])
    assert calls == ["ewald"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        calc.set_lrcoulomb_method("pme", ewald_accuracy=ACC)
    fd = calc.hessian_vector_product(data, V[:1]).cpu().numpy()
    assert calls == ["ewald"]  # the mesh method did not reach the sweep
    assert np.abs(fd - hv[:1].cpu().numpy()).max() < 2e-3 * max(1.0, np.abs(fd).max())


def test_through_the_calculator_with_external_dftd3(oracle64):
    """The dispersion block stays the in-sweep difference of the D3 gradient whatever the Coulomb method: cell A with the external
    DFT-D3 term against the oracle's Hessian with the same term, at the gate of test_hvp_with_external_dftd3."""
    gd, t = golden("dftd3"), golden("dftd3_subset")
    par = dict(s6=float(gd["s6"]), s8=float(gd["s8"]), a1=float(gd["a1"]), a2=float(gd["a2"]), cutoff=15.0, smoothing_fraction=0.2)
    tables = {k: t[k] for k in ("c6ab", "cn_ref", "rcov", "r4r2")}
    c, z, cell = cell_a()
    H64, _ = oracle_ref(oracle64, "A0d3", c, z, 0.0, cell, dftd3=dict(par, **tables))
    H64_no, _ = oracle_ref(oracle64, "A0", c, z, 0.0, cell)
    assert np.abs(H64 - H64_no).max() > 1e-2  # the term is there
    calc = _calculator((par, tables))
    out = calc(dict(coord=c, numbers=z, charge=0.0, cell=cell), forces=True, hessian=True)
    H = _np64(out["hessian"]).reshape(36, 36)
    err = np.abs(H - H64).max()
    print(f"[hvp-ewald] case 7 (D3): max|d| = {err:.3e} on max|H| = {np.abs(H64).max():.3e}, gate 2e-4, ratio {err / 2e-4:.3f}")
    assert np.allclose(H, H64, rtol=1e-3, atol=1e-3) and err <= 2e-4, err


def test_rejections(hip_engine):
    from aimnetcentral_amd import _lib
    from aimnetcentral_amd._lib import HipLibraryError
    from aimnetcentral_amd.engine import describe_input_flags
    from oracle import aimnet2_oracle as O

    c, z, cell = cell_a()
    args = (_t(c), _t(z, torch.int32), torch.zeros(12, dtype=torch.int32, device="cuda"), _t([0.0]), torch.zeros(1, 12, 3, device="cuda"))
    with pytest.raises(ValueError, match="particle-mesh"):
        hip_engine.hvp(*args, cell=_t(cell), coulomb="pme")
    with pytest.raises(ValueError, match="periodic cell"):
        hip_engine.hvp(*args, coulomb="ewald")
    with pytest.raises(HipLibraryError, match="periodic along all three axes"):
        hip_engine.hvp(*args, cell=_t(cell), pbc=(True, True, False), coulomb="ewald")
    # a list cutoff below the system's real-space cutoff, straight through the C interface: status[6] bit 6
    _, rc, _ = O.ewald_parameters(12, abs(np.linalg.det(cell.astype(np.float64))), ACC)
    coord, numbers, mol, charge, v = args
    cell_t, hv, status = _t(cell), torch.empty_like(v), torch.empty(8, dtype=torch.int32, device="cuda")
    inp = _lib.Inputs()
    inp.n_atoms, inp.n_mol = 12, 1
    inp.coord, inp.numbers, inp.mol_idx, inp.charge = coord.data_ptr(), numbers.data_ptr(), mol.data_ptr(), charge.data_ptr()
    inp.cell, inp.n_cell, inp.pbc_sys = cell_t.data_ptr(), 1, None
    for k in range(3):
        inp.pbc[k] = 1
    for list_rc, flagged in ((0.9 * rc, True), (1.001 * rc, False)):
        opt = _lib.EvalOptions()
        opt.coulomb, opt.dsf_rc, opt.dsf_alpha = _lib.COULOMB_EWALD, float(list_rc), 0.2
        opt.max_nb, opt.max_nb_lr = 128, 1024
        opt.ewald_accuracy, opt.ewald_max_k = ACC, 256
        need = int(hip_engine.lib.aimnet_engine_hvp_workspace_bytes(hip_engine._h, 12, 1, 1, C.byref(opt)))
        ws = torch.empty(need + 4096, dtype=torch.uint8, device="cuda")
        rcode = hip_engine.lib.aimnet_engine_hvp(hip_engine._h, C.byref(inp), C.byref(opt), v.data_ptr(), 1, hv.data_ptr(), None,
                                                 status.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        _lib.check(rcode, "aimnet_engine_hvp")
        st = status.cpu().numpy()
        assert bool(st[6] & 64) == flagged and not (st[6] & ~64), st
        assert not st[2] and not st[3] and st[7] <= 256
    assert "real-space cutoff" in describe_input_flags(64) and "unknown" not in describe_input_flags(64)
