"""Particle-mesh Ewald in the analytic Hessian-vector sweep (csrc/pme.hip: tangent charge assignment, transforms, field pass and
tangent interpolation; csrc/hvp.hip: the `pme` branch of the tangent plan; armed by HipEngine.hvp(..., pme_tangent=True) /
AIMNet2Calculator.set_pme_hessian("analytic")).

Two anchors, as for the mesh itself (tests/test_gpu_pme.py).  (1) The mesh tangent stage alone (aimnet_debug_pme_tangent) against
its fp64 twin tests/pme_tangent_yardstick.py on the same mesh: double against double, to test_mesh_kernels_equal_their_cpu_twin's
allowance scaled by the step of the tangent's fixed point, 1e-10 max(1, max|ref|) 2^44 / (the reported scale).  (2) The sweep against
the dense Hessian of the fp64 oracle's EXACT Ewald sum (a converged Ewald Hessian does not depend on the splitting or on how the
reciprocal sum is taken) at ewald_accuracy = 1e-8, where the mesh error of the tangent (<= 5e-8 on the CPU,
tests/test_pme_tangent_host.py) is negligible in the sweep's own gate, `_close` of tests/test_gpu_hvp_ewald.py: 1e-5 + 3e-5 max|ref|.
Every comparison prints its ratio to the gate before it asserts (profiles/pme_hessian.md)."""
from __future__ import annotations

import ctypes as C
import math
import warnings

import numpy as np
import pytest
import torch

import pme_tangent_yardstick as Y
from conftest import assert_forces_close, golden
from oracle import pme as OP
from test_gpu_hvp_ewald import _close, _np64, _t, cell_a, cell_b, oracle_ref, small_cell
from test_gpu_pme import _random_cell

pytestmark = pytest.mark.gpu

ACC = 1e-8


# ---- 1. the mesh tangent alone ---------------------------------------------------------------------------------------------------
def _tangent(eng, x, q, tq, v, cell, acc, max_mesh=1 << 20, order=None):
    lib, dev = eng.lib, eng.device
    n, k = len(x), len(v)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    xd, qd, tqd, vd, cd = f32(x), f32(q), f32(tq), f32(v), f32(cell)
    field = torch.zeros(n, 10, dtype=torch.float64, device=dev)
    tphi = torch.full((k, n), 7.0, dtype=torch.float64, device=dev)
    tg = torch.full((k, n, 3), 7.0, dtype=torch.float64, device=dev)
    info = (C.c_double * 8)()
    od = None if order is None else torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(dev)
    torch.cuda.synchronize()
    rc = lib.aimnet_debug_pme_tangent(xd.data_ptr(), qd.data_ptr(), tqd.data_ptr(), vd.data_ptr(), None if od is None else od.data_ptr(),
                                      cd.data_ptr(), float(q.astype(np.float32).sum(dtype=np.float64)), n, k, acc, max_mesh,
                                      field.data_ptr(), tphi.data_ptr(), tg.data_ptr(), info, None)
    assert rc == 0
    return field.cpu().numpy(), tphi.cpu().numpy(), tg.cpu().numpy(), list(info)


def _directions(x, q, seed, k=5):
    rng = np.random.default_rng(seed)
    tq = rng.normal(0.0, 0.3, (k, len(x))).astype(np.float32)
    tq[:, 0] -= tq.sum(axis=1, dtype=np.float64).astype(np.float32)
    v = rng.standard_normal((k, len(x), 3)).astype(np.float32)
    return tq, v


def _bin_order(x, cell):
    frac = (x.astype(np.float64) @ np.linalg.inv(cell.astype(np.float64))) % 1.0
    box = np.floor(frac * np.maximum(1, np.floor(np.linalg.norm(cell, axis=1) / 4.0))).astype(np.int64)
    return np.lexsort((box[:, 2], box[:, 1], box[:, 0]))


@pytest.mark.parametrize("rep,acc", [((1, 1, 1), 1e-6), ((2, 1, 1), 1e-4)])
def test_mesh_tangent_equals_its_cpu_twin(hip_engine, rep, acc):
    """96 / 192 atoms with images outside the cell, K = 5 (one full group of four directions and a partial one), in input order
    (the direct assignment wherever neighbours in the order are far apart) and in bin order (the LDS tile)."""
    x, q, cell = _random_cell(rep, 11, neutral=rep == (1, 1, 1))
    tq, v = _directions(x, q, 3)
    field, tphi, tg, info = _tangent(hip_engine, x, q, tq, v, cell, acc)
    alpha, rc, mesh = OP.pme_parameters(len(x), cell.astype(np.float64), acc)
    assert [int(m) for m in info[2:5]] == list(mesh) and int(info[5]) == mesh[0] * mesh[1] * mesh[2]
    assert abs(info[0] - alpha) < 1e-6 * alpha and abs(info[1] - rc) < 1e-6 * rc
    scale = info[7]
    assert 0.0 < scale <= 2.0 ** 40 and math.log2(scale) == round(math.log2(scale))
    alpha_eff = math.sqrt(1.0 / (4.0 * float(np.float32(1.0 / (4.0 * alpha * alpha)))))  # (1 / 4 alpha^2 is kept as fp32)
    ref = Y.pme_tangent(x, q, tq, v, cell, alpha_eff, mesh)
    T6 = np.stack([ref["T"][:, 0, 0], ref["T"][:, 1, 1], ref["T"][:, 2, 2], ref["T"][:, 0, 1], ref["T"][:, 0, 2], ref["T"][:, 1, 2]], axis=1)
    step = 2.0 ** 44 / scale  # every double output to the one allowance
    for name, got, want in (("phi", field[:, 0], ref["phi"]), ("g", field[:, 1:4], ref["g"]), ("T", field[:, 4:], T6),
                            ("tphi", tphi, ref["tphi"]), ("tg", tg, ref["tg"])):
        err, tol = np.abs(got - want).max(), 1e-10 * max(1.0, np.abs(want).max()) * step
        print(f"[hvp-pme] case 1 {rep} acc {acc:g} mesh {mesh} scale 2^{math.log2(scale):.0f}: {name} max|d| = {err:.3e} on "
              f"max|ref| = {np.abs(want).max():.3e}, allowance {tol:.3e}, ratio {err / tol:.3f}")
        assert err <= tol, name
    # bitwise equal on repetition, and between the two forms of the assignment
    again = _tangent(hip_engine, x, q, tq, v, cell, acc)
    tiled = _tangent(hip_engine, x, q, tq, v, cell, acc, order=_bin_order(x, cell))
    for a, b, c in zip((field, tphi, tg), again[:3], tiled[:3]):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    # the operator is linear in (t_q, v): scaled by 2^10 and 2^-10 the results scale by exactly that, or to within the allowance
    for p in (10, -10):
        s = 2.0 ** p
        f2, tphi2, tg2, info2 = _tangent(hip_engine, x, q, tq * np.float32(s), v * np.float32(s), cell, acc)
        assert info2[7] == scale / s and np.array_equal(f2, field)
        exact = np.array_equal(tphi2, tphi * s) and np.array_equal(tg2, tg * s)
        print(f"[hvp-pme] case 1 {rep}: directions x 2^{p}: results scaled exactly: {exact}")
        step = 2.0 ** 44 / info2[7]
        assert np.abs(tphi2 - tphi * s).max() <= 1e-10 * max(1.0, np.abs(tphi * s).max()) * step
        assert np.abs(tg2 - tg * s).max() <= 1e-10 * max(1.0, np.abs(tg * s).max()) * step


def test_mesh_tangent_reports_a_capacity_that_is_too_small(hip_engine):
    x, q, cell = _random_cell((1, 1, 1), 11)
    tq, v = _directions(x, q, 3, k=2)
    field, tphi, tg, info = _tangent(hip_engine, x, q, tq, v, cell, 1e-6, max_mesh=512)
    assert int(info[5]) > 512 and not field.any() and not tphi.any() and not tg.any()  # nothing computed, the need reported


# ---- 2 - 6. the sweep against the oracle's exact-Ewald Hessian -----------------------------------------------------------------------
def _hvp(eng, coord, numbers, charge, cell, V, mol=None, acc=ACC, **kw):
    n = len(numbers)
    mol = np.zeros(n, dtype=np.int64) if mol is None else mol
    return eng.hvp(_t(coord), _t(numbers, torch.int32), _t(mol, torch.int32), _t(charge), _t(V), cell=_t(cell), coulomb="pme",
                   pme_tangent=True, ewald_accuracy=acc, **kw)


def test_dense_hessian_of_a_small_cell(hip_engine, oracle64):
    """All 36 unit directions of cell A: Hessian and forces of the sweep against the oracle's exact sum; and the result is NOT the
    real-space term alone (outside the gate of the oracle's DSF Hessian at the mesh method's alpha, r_c: a dropped mesh part shows)."""
    c, z, cell = cell_a()
    H64, f64 = oracle_ref(oracle64, "A0@1e-8", c, z, 0.0, cell, ewald_accuracy=ACC)
    out = _hvp(hip_engine, c, z, [0.0], cell, np.eye(36, dtype=np.float32).reshape(36, 12, 3), want_forces=True)
    H = _np64(out["hv"]).reshape(36, 36)
    _close(H, H64, "pme case 2: dense Hessian of A")
    assert_forces_close(out["forces"].cpu().numpy(), f64, "A (forces of the armed sweep)")
    alpha, rc, mesh = OP.pme_parameters(12, cell.astype(np.float64), ACC)
    assert int(hip_engine.last_status[7]) == mesh[0] * mesh[1] * mesh[2] and int(hip_engine.last_status[1]) > 12
    Hdsf, _ = oracle_ref(oracle64, "A0dsf@pme", c, z, 0.0, cell, coulomb="dsf", dsf_rc=rc, dsf_alpha=alpha)
    away, gate = np.abs(H - Hdsf).max(), 1e-5 + 3e-5 * np.abs(Hdsf).max()
    print(f"[hvp-pme] case 2: distance from the DSF Hessian at the same (alpha, r_c): {away:.3e}, {away / gate:.0f} x its gate")
    assert away > gate


def test_charged_cell_on_the_capped_branch(hip_engine, oracle64):
    """B with charge +1 at 1e-8: the Ewald estimate's cutoff (10.6 A) is capped at 10 A, alpha differs from the exact method's."""
    c, z, cell = cell_b()
    alpha, rc, _ = OP.pme_parameters(16, cell.astype(np.float64), ACC)
    assert rc == 10.0
    H64, f64 = oracle_ref(oracle64, "B+1@1e-8", c, z, 1.0, cell, ewald_accuracy=ACC)
    V = np.random.default_rng(11).standard_normal((3, 16, 3)).astype(np.float32)
    out = _hvp(hip_engine, c, z, [1.0], cell, V, want_forces=True)
    _close(_np64(out["hv"]).reshape(3, 48), V.reshape(3, 48).astype(np.float64) @ H64, "pme case 3: B, charge +1")
    assert_forces_close(out["forces"].cpu().numpy(), f64, "B +1 (forces of the armed sweep)")


def test_two_systems_with_their_own_meshes(hip_engine, oracle64):
    """A and B in one call, charges (0, -1): per-system (alpha, r_c, mesh), a (direction, system) slice each."""
    ca, za, cella = cell_a()
    cb, zb, cellb = cell_b()
    Ha, fa = oracle_ref(oracle64, "A0@1e-8", ca, za, 0.0, cella, ewald_accuracy=ACC)
    Hb, fb = oracle_ref(oracle64, "B-1@1e-8", cb, zb, -1.0, cellb, ewald_accuracy=ACC)
    mol = np.concatenate([np.zeros(12, np.int64), np.ones(16, np.int64)])
    V = np.random.default_rng(11).standard_normal((3, 28, 3)).astype(np.float32)
    out = _hvp(hip_engine, np.concatenate([ca, cb]), np.concatenate([za, zb]), [0.0, -1.0], np.stack([cella, cellb]), V, mol=mol,
               want_forces=True)
    hv = _np64(out["hv"])
    _close(hv[:, :12].reshape(3, 36), V[:, :12].reshape(3, 36).astype(np.float64) @ Ha, "pme case 4: A of (A, B)")
    _close(hv[:, 12:].reshape(3, 48), V[:, 12:].reshape(3, 48).astype(np.float64) @ Hb, "pme case 4: B of (A, B), charge -1")
    f = out["forces"].cpu().numpy()
    assert_forces_close(f[:12], fa, "A of (A, B)")
    assert_forces_close(f[12:], fb, "B of (A, B)")


def test_two_charge_channels(hip_engine_nse, oracle64_nse):
    """Open-shell NSE model: the mesh sees alpha + beta, both channels get the seed."""
    from oracle import aimnet2_oracle as O

    c, z, cell = small_cell(7, 12, 6.0)
    r = O.evaluate(oracle64_nse, c, z, np.array([1.0], np.float32), cell=cell, coulomb="ewald", ewald_accuracy=ACC, hessian=True,
                   mult=np.array([2.0], np.float32))
    H64 = r["hessian"].reshape(36, 36)
    V = np.random.default_rng(11).standard_normal((3, 12, 3)).astype(np.float32)
    out = _hvp(hip_engine_nse, c, z, [[1.0, 0.0]], cell, V, want_forces=True)
    _close(_np64(out["hv"]).reshape(3, 36), V.reshape(3, 36).astype(np.float64) @ H64, "pme case 5: two channels, charge +1, doublet")
    assert_forces_close(out["forces"].cpu().numpy(), r["forces"], "NSE cell (forces of the armed sweep)")


def test_operator_properties(hip_engine):
    """Symmetry, translation invariance, bitwise repeatability, independence of how the directions are split into sweeps and of the
    capacities the sweep started from (the mesh and the neighbour rows grow and the sweep repeats)."""
    c, z, cell = cell_a()
    args = (hip_engine, c, z, [0.0], cell)
    H = _hvp(*args, np.eye(36, dtype=np.float32).reshape(36, 12, 3))["hv"].view(36, 36)
    assert (H - H.T).abs().max().item() < 1e-5
    shift = np.zeros((3, 12, 3), np.float32)
    for a in range(3):
        shift[a, :, a] = 1.0
    assert _hvp(*args, shift)["hv"].abs().max().item() < 2e-4
    V = np.random.default_rng(2).standard_normal((5, 12, 3)).astype(np.float32)
    hv = _hvp(*args, V)["hv"]
    assert torch.equal(hv, _hvp(*args, V)["hv"])
    assert (hv.view(5, 36) - _t(V).view(5, 36) @ H).abs().max().item() < 2e-4
    budget = hip_engine.HVP_BYTES_BUDGET
    try:  # one direction per sweep: identical numbers (a direction never sees another one)
        hip_engine.HVP_BYTES_BUDGET = 1
        assert torch.equal(hv, _hvp(*args, V)["hv"])
    finally:
        hip_engine.HVP_BYTES_BUDGET = budget
    old_mesh, old_nb = hip_engine._pme_max_mesh, hip_engine.max_nb
    try:
        hip_engine._pme_max_mesh = 512
        got = _hvp(*args, V)["hv"]
        assert hip_engine._pme_max_mesh >= int(hip_engine.last_status[7]) > 512 and torch.equal(got, hv)
        hip_engine.max_nb = 16
        got = _hvp(*args, V)["hv"]
        assert hip_engine.max_nb > 16 and torch.equal(got, hv)
    finally:
        hip_engine._pme_max_mesh = max(old_mesh, hip_engine._pme_max_mesh)
        hip_engine.max_nb = max(old_nb, hip_engine.max_nb)


# ---- 7 - 8. through the calculator ---------------------------------------------------------------------------------------------------
def _calculator(method="pme", acc=ACC, dftd3=None, armed=True):
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
        calc.set_lrcoulomb_method(method, ewald_accuracy=acc)
    if armed:
        calc.set_pme_hessian("analytic")
    return calc


def test_more_atoms_than_one_block_at_the_default_accuracy():
    """The (3, 3, 3) supercell of A, 324 atoms, at 1e-6: the armed calculator against its own finite-difference operator at the gate
    that pair has, 2e-3 max(1, |fd|).  Its distance from the Ewald-method sweep is printed, not asserted: no mesh-error budget has
    been measured through the network at 1e-6."""
    c, z, cell = cell_a()
    reps = np.array([(i, j, k) for i in range(3) for j in range(3) for k in range(3)], dtype=np.float64)
    coord = (c[None].astype(np.float64) + (reps @ cell.astype(np.float64))[:, None]).reshape(-1, 3)
    coord = (coord + np.random.default_rng(3).normal(0.0, 0.02, coord.shape)).astype(np.float32)
    data = dict(coord=coord, numbers=np.tile(z, 27), charge=0.0, cell=(3.0 * cell).astype(np.float32))
    calc = _calculator(acc=1e-6)
    v = np.random.default_rng(4).standard_normal((1, 324, 3)).astype(np.float32)
    hv = calc.hessian_vector_product(data, v).cpu().numpy()
    calc.hvp_method = "fd"
    fd = calc.hessian_vector_product(data, v).cpu().numpy()
    err, gate = np.abs(hv - fd).max(), 2e-3 * max(1.0, np.abs(fd).max())
    print(f"[hvp-pme] case 7: 324 atoms at 1e-6, armed sweep vs fd: max|d| = {err:.3e}, gate {gate:.3e}, ratio {err / gate:.3f}")
    ew = _calculator("ewald", acc=1e-6, armed=False).hessian_vector_product(data, v).cpu().numpy()
    d = np.abs(hv - ew).max()
    print(f"[hvp-pme] case 7: armed sweep vs the Ewald-method sweep: max|d| = {d:.3e} on max|Hv| = {np.abs(ew).max():.3e} "
          f"({d / (1e-5 + 3e-5 * np.abs(ew).max()):.3f} of the sweep's gate; recorded, not asserted)")
    assert err < gate


def test_through_the_calculator(oracle64, monkeypatch):
    """set_pme_hessian("analytic"): hessian_vector_product is the engine's armed sweep (bitwise), eval(hessian=True) the oracle's
    Hessian; unarmed, nothing reaches engine.hvp."""
    c, z, cell = cell_a()
    H64, _ = oracle_ref(oracle64, "A0@1e-8", c, z, 0.0, cell, ewald_accuracy=ACC)
    calc = _calculator()
    data = dict(coord=c, numbers=z, charge=0.0, cell=cell)
    V = np.random.default_rng(11).standard_normal((3, 12, 3)).astype(np.float32)
    hv = calc.hessian_vector_product(data, V)
    assert torch.equal(hv, _hvp(calc.engine, c, z, [0.0], cell, V)["hv"])
    out = calc(data, forces=True, hessian=True)
    _close(_np64(out["hessian"]).reshape(36, 36), H64, "pme case 8: calculator eval(hessian=True) on A")
    calls = []
    real = calc.engine.hvp
    monkeypatch.setattr(calc.engine, "hvp", lambda *a, **k: calls.append((k.get("coulomb"), k.get("pme_tangent"))) or real(*a, **k))
    calc.hessian_vector_product(data, V[:1])
    assert calls == [("pme", True)]
    calc.set_pme_hessian(None)
    fd = calc.hessian_vector_product(data, V[:1]).cpu().numpy()
    assert calls == [("pme", True)]  # unarmed: differences of forces, the sweep was not called
    assert np.abs(fd - hv[:1].cpu().numpy()).max() < 2e-3 * max(1.0, np.abs(fd).max())


def test_through_the_calculator_with_external_dftd3(oracle64):
    """The dispersion block stays the in-sweep difference of the D3 gradient: cell A with the external DFT-D3 term against the
    oracle's Hessian with the same term, at the gate of test_gpu_hvp_ewald's case of the same name."""
    gd, t = golden("dftd3"), golden("dftd3_subset")
    par = dict(s6=float(gd["s6"]), s8=float(gd["s8"]), a1=float(gd["a1"]), a2=float(gd["a2"]), cutoff=15.0, smoothing_fraction=0.2)
    tables = {k: t[k] for k in ("c6ab", "cn_ref", "rcov", "r4r2")}
    c, z, cell = cell_a()
    H64, _ = oracle_ref(oracle64, "A0d3@1e-8", c, z, 0.0, cell, ewald_accuracy=ACC, dftd3=dict(par, **tables))
    calc = _calculator(dftd3=(par, tables))
    out = calc(dict(coord=c, numbers=z, charge=0.0, cell=cell), forces=True, hessian=True)
    H = _np64(out["hessian"]).reshape(36, 36)
    err = np.abs(H - H64).max()
    print(f"[hvp-pme] case 8 (D3): max|d| = {err:.3e} on max|H| = {np.abs(H64).max():.3e}, gate 2e-4, ratio {err / 2e-4:.3f}")
    assert np.allclose(H, H64, rtol=1e-3, atol=1e-3) and err <= 2e-4, err


# ---- 9. rejections ---------------------------------------------------------------------------------------------------------------
def test_rejections(hip_engine):
    from aimnetcentral_amd import _lib
    from aimnetcentral_amd._lib import HipLibraryError

    c, z, cell = cell_a()
    args = (_t(c), _t(z, torch.int32), torch.zeros(12, dtype=torch.int32, device="cuda"), _t([0.0]), torch.zeros(1, 12, 3, device="cuda"))
    with pytest.raises(ValueError, match="particle-mesh"):  # without the flag: today's refusal
        hip_engine.hvp(*args, cell=_t(cell), coulomb="pme")
    with pytest.raises(ValueError, match="periodic cell"):
        hip_engine.hvp(*args, coulomb="pme", pme_tangent=True)
    with pytest.raises(HipLibraryError, match="periodic along all three axes"):
        hip_engine.hvp(*args, cell=_t(cell), pbc=(True, True, False), coulomb="pme", pme_tangent=True)
    emb = dict(potential=torch.zeros(12, device="cuda"), potential_grad=torch.zeros(12, 3, device="cuda"),
               potential_hess=torch.zeros(12, 6, device="cuda"))
    with pytest.raises(HipLibraryError, match="embedding: the analytic tangent sweep does not cover particle-mesh Ewald"):
        hip_engine.hvp(*args, cell=_t(cell), coulomb="pme", pme_tangent=True, embedding=emb)
    # straight through the C interface: caller-supplied matrices; a list cutoff below the system's r_c (status[6] bit 6)
    _, rc, mesh = OP.pme_parameters(12, cell.astype(np.float64), ACC)
    coord, numbers, mol, charge, v = args
    cell_t, hv, status = _t(cell), torch.empty_like(v), torch.empty(8, dtype=torch.int32, device="cuda")
    inp = _lib.Inputs()
    inp.n_atoms, inp.n_mol = 12, 1
    inp.coord, inp.numbers, inp.mol_idx, inp.charge = coord.data_ptr(), numbers.data_ptr(), mol.data_ptr(), charge.data_ptr()
    inp.cell, inp.n_cell, inp.pbc_sys = cell_t.data_ptr(), 1, None
    for k in range(3):
        inp.pbc[k] = 1
    lib, h = hip_engine.lib, hip_engine._h

    def call(list_rc):
        opt = _lib.EvalOptions()
        opt.coulomb, opt.dsf_rc, opt.dsf_alpha = _lib.COULOMB_PME, float(list_rc), 0.2
        opt.max_nb, opt.max_nb_lr = 128, 1024
        opt.ewald_accuracy, opt.pme_max_mesh = ACC, 8192
        need = int(lib.aimnet_engine_hvp_workspace_bytes(h, 12, 1, 1, C.byref(opt)))
        ws = torch.empty(need + 4096, dtype=torch.uint8, device="cuda")
        rcode = lib.aimnet_engine_hvp(h, C.byref(inp), C.byref(opt), v.data_ptr(), 1, hv.data_ptr(), None, status.data_ptr(), ws.data_ptr(),
                                      ws.numel(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rcode

    try:
        assert lib.aimnet_engine_set_pme_tangent(h, 1) == 0
        for list_rc, flagged in ((0.9 * rc, True), (1.001 * rc, False)):
            _lib.check(call(list_rc), "aimnet_engine_hvp")
            st = status.cpu().numpy()
            assert bool(st[6] & 64) == flagged and not (st[6] & ~64), st
            assert not st[2] and not st[3] and st[7] == mesh[0] * mesh[1] * mesh[2]
        nb = torch.zeros(12, 16, dtype=torch.int32, device="cuda")
        inp.nbmat = nb.data_ptr()
        with pytest.raises(HipLibraryError, match="caller-supplied neighbour matrices"):
            _lib.check(call(1.001 * rc), "aimnet_engine_hvp")
        inp.nbmat = None
        assert lib.aimnet_engine_set_pme_tangent(h, 0) == 0
        with pytest.raises(HipLibraryError, match="does not cover particle-mesh Ewald"):  # disarmed: refused as before
            _lib.check(call(1.001 * rc), "aimnet_engine_hvp")
    finally:
        lib.aimnet_engine_set_pme_tangent(h, 0)
