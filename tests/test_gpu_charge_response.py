"""Charge response and dipole derivatives (csrc/hvp.hip, aimnet_engine_charge_response) against the fp64 tangent sweep of the
oracle: the intermediate `_t_q1` of oracle/aimnet2_analytic.py::evaluate_hvp (tests/test_charge_response_host.py holds it to
differences of the oracle's charges).  Gate for a tangent: the project's own for this sweep, `_close` of tests/test_gpu_hvp.py,
max|d| <= 1e-5 + 3e-5 max|ref| (the fp32 oracle sits at 0.04 - 0.07 of it).  Every comparison prints its ratio to the gate before
it asserts."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from conftest import CHARGE_ATOL, golden

pytestmark = pytest.mark.gpu

_REFS: dict = {}


def _t(a, dt=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dt).cuda()


def _np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _reference(om64, key, coord, numbers, charge, mol, V, cell=None, kw=None, mult=None):
    """fp64 charges and charge tangents (K, N, nq), built as `_spec_and_engine` of tests/test_gpu_hvp.py builds its sweep; once per key."""
    if key not in _REFS:
        from oracle import aimnet2_analytic as AN
        from oracle import aimnet2_oracle as O

        kw = kw or {}
        ref = O.evaluate(om64, coord, numbers, charge, mol, cell=cell, return_intermediates=True, forces=False, mult=mult, **kw)
        xw = ref["coord_wrapped"]
        if cell is None:
            nbl, shl = O.neighbor_list(xw, float("inf"), mol)
            coul = "simple"
        else:
            nbl, shl = O.neighbor_list(xw, kw["dsf_rc"], mol, cell, np.ones(3, bool))
            coul = "dsf"
        spec = AN.evaluate_hvp(om64, xw, numbers, charge, mol, ref["nbmat"], V, shifts=ref.get("shifts"), cell=cell, coulomb=coul,
                               nbmat_lr=nbl, shifts_lr=shl, mult=mult, return_intermediates=True,
                               **{k: v for k, v in kw.items() if k != "coulomb"})
        _REFS[key] = {"t_q": spec["_t_q1"], "charges": np.asarray(ref["charges"], np.float64),
                      "spin_charges": np.asarray(ref["spin_charges"], np.float64) if "spin_charges" in ref else None}
    return _REFS[key]


def _engine_args(eng, coord, numbers, charge, mol, mult=None):
    q = np.atleast_1d(np.asarray(charge, dtype=np.float32))
    if eng.nq == 2:
        mt = np.ones_like(q) if mult is None else np.atleast_1d(np.asarray(mult, dtype=np.float32))
        q = np.stack([0.5 * q + 0.5 * (mt - 1), 0.5 * q - 0.5 * (mt - 1)], -1)
    return _t(coord), _t(numbers, torch.int32), _t(mol, torch.int32), _t(q)


def _gate(got, ref, what):
    err, top = np.abs(got - ref).max(), np.abs(ref).max()
    gate = 1e-5 + 3e-5 * top
    print(f"[charge-response] {what}: max|d| = {err:.3e} on max|ref| = {top:.3e}, gate {gate:.3e}, ratio {err / gate:.3f}")
    assert err <= gate, f"{what}: max|d| = {err:.3e} > {gate:.3e}"


def _charges_close(got, ref, what):
    err = np.abs(got - ref).max()
    print(f"[charge-response] {what}: max|d q| = {err:.3e}, gate {CHARGE_ATOL:.1e}, ratio {err / CHARGE_ATOL:.3f}")
    assert err <= CHARGE_ATOL, f"{what}: {err:.3e}"


def _hvp40(hip_engine, oracle64):
    """The 40-atom molecule, its 120 unit directions, the engine's answer and the fp64 one (shared by cases 3, 5 and 6)."""
    g = golden("hvp40")
    mol = np.zeros(40, dtype=np.int64)
    eye = np.eye(120, dtype=np.float32).reshape(120, 40, 3)
    ref = _reference(oracle64, "hvp40", g["coord"], g["numbers"], 0.0, mol, eye)
    args = _engine_args(hip_engine, g["coord"], g["numbers"], [0.0], mol)
    return g, args, eye, ref


# ---- case 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [
    ("taxol", {}),
    ("batch5", {}),
    ("pbc96_dsf8_wrapped", {"coulomb": "dsf", "dsf_rc": 8.0, "dsf_alpha": 0.25}),
])
def test_matches_the_fp64_tangent_sweep(hip_engine, oracle64, name, kw):
    """taxol (stacked rows 452: the split GEMMs), a ragged batch, a periodic cell (dq only: no dipole in the result)."""
    g = golden(name)
    n = len(g["numbers"])
    mol = g["mol_idx"] if "mol_idx" in g.files else np.zeros(n, dtype=np.int64)
    cell = g["cell"] if "cell" in g.files else None
    V = np.random.default_rng(11).standard_normal((3, n, 3)).astype(np.float32)
    ref = _reference(oracle64, name, g["coord"], g["numbers"], g["charge"], mol, V, cell, kw)
    out = hip_engine.charge_response(*_engine_args(hip_engine, g["coord"], g["numbers"], g["charge"], mol), _t(V),
                                     cell=None if cell is None else _t(cell))
    assert out["dq"].shape == (3, n) and out["charges"].shape == (n,) and "dspin" not in out
    _gate(_np64(out["dq"]), ref["t_q"].sum(-1), name + " dq")
    _charges_close(_np64(out["charges"]), ref["charges"], name + " charges")
    if cell is None:
        n_mol = int(mol.max()) + 1
        assert out["dmu"].shape == (3, n_mol, 3)
    else:
        assert "dmu" not in out
        with pytest.raises(ValueError, match="periodic"):
            hip_engine.charge_response(*_engine_args(hip_engine, g["coord"], g["numbers"], g["charge"], mol), _t(V), cell=_t(cell),
                                       want_dipole=True)


# ---- case 2 ----------------------------------------------------------------------------------------------------------
def test_two_charge_channels(hip_engine, hip_engine_nse, oracle64_nse):
    g = golden("nse")
    n = len(g["b5_numbers"])
    V = np.random.default_rng(11).standard_normal((3, n, 3)).astype(np.float32)
    ref = _reference(oracle64_nse, "nse_b5", g["b5_coord"], g["b5_numbers"], g["b5_charge"], g["b5_mol_idx"], V, mult=g["b5_mult"])
    out = hip_engine_nse.charge_response(*_engine_args(hip_engine_nse, g["b5_coord"], g["b5_numbers"], g["b5_charge"], g["b5_mol_idx"],
                                                       g["b5_mult"]), _t(V))
    _gate(_np64(out["dq"]), ref["t_q"].sum(-1), "nse b5 dq")
    _gate(_np64(out["dspin"]), ref["t_q"][..., 0] - ref["t_q"][..., 1], "nse b5 dspin")
    _charges_close(_np64(out["charges"]), ref["charges"], "nse b5 charges")
    # dspin from a 1-channel engine, through the C interface
    g1 = golden("hvp40")
    a = _engine_args(hip_engine, g1["coord"], g1["numbers"], [0.0], np.zeros(40, dtype=np.int64))
    rc, st = _raw_call(hip_engine, a, torch.zeros(1, 40, 3, device="cuda"), dspin=True)
    assert rc == -1 and (st == 77).all()


# ---- case 3 ----------------------------------------------------------------------------------------------------------
def _dmu_reference(ref, coord, V):
    """sum_i t_q_i x_i + q_i v_i in fp64 from the oracle's values, and the charge-response gate propagated through that sum."""
    x, v = np.asarray(coord, np.float64), np.asarray(V, np.float64)
    tq = ref["t_q"].sum(-1)
    dmu = np.einsum("ki,ic->kc", tq, x) + np.einsum("i,kic->kc", ref["charges"], v)
    bound = (1e-5 + 3e-5 * np.abs(tq).max()) * np.abs(x).max(-1).sum() + CHARGE_ATOL * np.abs(v).max(-1).sum(-1)  # per direction
    return dmu, bound


def test_whole_polar_tensor_of_hvp40(hip_engine, oracle64):
    """120 unit directions in one sweep (stacked rows 4 840), and 3 of them in a sweep that runs the exact-fp32 GEMMs (160 rows)."""
    g, args, eye, ref = _hvp40(hip_engine, oracle64)
    dmu_ref, bound = _dmu_reference(ref, g["coord"], eye)
    for K in (120, 3):
        out = hip_engine.charge_response(*args, _t(eye[:K]))
        _gate(_np64(out["dq"]), ref["t_q"].sum(-1)[:K], f"hvp40 dq, {K} directions")
        err = np.abs(_np64(out["dmu"])[:, 0] - dmu_ref[:K]).max(-1)
        print(f"[charge-response] hvp40 dmu, {K} directions: max|d| = {err.max():.3e}, bound {bound[:K].min():.3e}, "
              f"ratio {(err / bound[:K]).max():.3f}")
        assert (err <= bound[:K]).all()


# ---- case 4 ----------------------------------------------------------------------------------------------------------
def test_dipole_reduction_on_ranges_that_are_no_multiple_of_256(hip_engine):
    """Molecule 0 = three taxol copies 30 A apart under one mol_idx (339 atoms: a second trip of the 256-thread loop), molecule 1 =
    taxol (113 atoms from atom 339), K = 5: dmu against the same sum on the host in fp64 from the engine's own dq, charges, coord
    and v.  The kernel forms fp32 products (2^-24 relative each), sums them in double and stores one fp32 (2^-24 of the sum):
    4 * 2^-24 * sum_i (|dq_i x_i| + |q_i v_i|) per component covers it twice."""
    g = golden("taxol")
    c, z = g["coord"].astype(np.float32), g["numbers"]
    shift = np.array([30.0, 0.0, 0.0], np.float32)
    coord = np.concatenate([c, c + shift, c + 2 * shift, c - np.array([0.0, 40.0, 0.0], np.float32)])
    numbers = np.concatenate([z] * 4)
    mol = np.concatenate([np.zeros(339, np.int64), np.ones(113, np.int64)])
    V = np.random.default_rng(4).standard_normal((5, 452, 3)).astype(np.float32)
    out = hip_engine.charge_response(*_engine_args(hip_engine, coord, numbers, [0.0, 0.0], mol), _t(V))
    dq, q, dmu = _np64(out["dq"]), _np64(out["charges"]), _np64(out["dmu"])
    assert dmu.shape == (5, 2, 3)
    x, v = coord.astype(np.float64), V.astype(np.float64)
    worst = 0.0
    for m, sl in enumerate((slice(0, 339), slice(339, 452))):
        terms_x = dq[:, sl, None] * x[None, sl]
        terms_v = q[None, sl, None] * v[:, sl]
        want = (terms_x + terms_v).sum(1)
        bound = 4.0 * 2.0**-24 * (np.abs(terms_x) + np.abs(terms_v)).sum(1)
        err = np.abs(dmu[:, m] - want)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (m, err.max(), bound.min())
    print(f"[charge-response] dmu reduction, 339 + 113 atoms, K = 5: largest |d| / bound = {worst:.3f}")


# ---- case 5 ----------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_operator_properties(hip_engine, oracle64):
    g, args, eye, ref = _hvp40(hip_engine, oracle64)
    top = np.abs(ref["t_q"].sum(-1)).max()
    v = torch.randn(5, 40, 3, generator=torch.Generator().manual_seed(2)).cuda()
    out = hip_engine.charge_response(*args, v)
    assert _same_bits(out, hip_engine.charge_response(*args, v))  # bitwise repeatable
    lin = hip_engine.charge_response(*args, (2.0 * v[0] - 0.5 * v[1]).unsqueeze(0))["dq"][0]
    want = 2.0 * out["dq"][0] - 0.5 * out["dq"][1]
    err, gate = (lin - want).abs().max().item(), 1e-5 + 3e-5 * out["dq"].abs().max().item()
    print(f"[charge-response] hvp40 linearity: max|d| = {err:.3e}, gate {gate:.3e}, ratio {err / gate:.3f}")
    assert err <= gate
    budget = hip_engine.HVP_BYTES_BUDGET
    try:  # one direction per sweep: a direction never sees another one
        hip_engine.HVP_BYTES_BUDGET = 1
        assert _same_bits(out, hip_engine.charge_response(*args, v))
    finally:
        hip_engine.HVP_BYTES_BUDGET = budget
    old = hip_engine.max_nb
    hip_engine.max_nb = 16  # the rows overflow, grow, and the sweep is repeated
    try:
        grown = hip_engine.charge_response(*args, v)
        assert hip_engine.max_nb > 16 and _same_bits(out, grown)
    finally:
        hip_engine.max_nb = max(old, hip_engine.max_nb)
    shift = torch.zeros(3, 40, 3, device="cuda")
    for c in range(3):
        shift[c, :, c] = 1.0
    tr = hip_engine.charge_response(*args, shift)
    err, gate = tr["dq"].abs().max().item(), 1e-5 + 3e-5 * top
    print(f"[charge-response] hvp40 uniform translation: max|dq| = {err:.3e}, gate {gate:.3e}, ratio {err / gate:.3f}")
    assert err <= gate
    # the workspace of a direction: strictly below the full sweep's for the same options
    opt, lib, h = hip_engine.fill_options(_request(40)), hip_engine.lib, hip_engine._h
    per = [int(f(h, 40, 1, 2, C.byref(opt))) - int(f(h, 40, 1, 1, C.byref(opt)))
           for f in (lib.aimnet_engine_charge_response_workspace_bytes, lib.aimnet_engine_hvp_workspace_bytes)]
    print(f"[charge-response] workspace per direction on 40 atoms: {per[0]} B against {per[1]} B of aimnet_engine_hvp ({per[0] / per[1]:.3f})")
    assert 0 < per[0] < per[1]


def _request(n, periodic=False):
    from aimnetcentral_amd import _lib, capacity

    return capacity.Request("hvp", n, 1, periodic, _lib.COULOMB_NONE, 0.0)


# ---- case 6 ----------------------------------------------------------------------------------------------------------
def test_through_the_calculator(hip_engine, oracle64):
    import warnings

    from aimnetcentral_amd import AIMNet2Calculator, loader, vibrations

    g, args, eye, ref = _hvp40(hip_engine, oracle64)
    calc = AIMNet2Calculator(loader.synthetic_spec(0), device="cuda:0")
    data = {"coord": g["coord"], "numbers": g["numbers"], "charge": 0.0}
    v = np.random.default_rng(5).standard_normal((2, 40, 3)).astype(np.float32)
    hv_before = calc.hessian_vector_product(data, v)
    res = calc.charge_response(data, v)
    want = calc.engine.charge_response(*args, _t(v))
    assert torch.equal(res["dq"], want["dq"]) and torch.equal(res["charges"], want["charges"])
    assert torch.equal(res["dipole_derivative"], want["dmu"][:, 0]) and "dspin" not in res
    one = calc.charge_response(data, v[0])
    assert one["dq"].shape == (40,) and one["dipole_derivative"].shape == (3,) and torch.equal(one["dq"], res["dq"][0])
    assert torch.equal(calc.hessian_vector_product(data, v), hv_before)
    P = calc.dipole_derivatives(data)
    assert P.shape == (40, 3, 3) and torch.equal(P.reshape(120, 3), calc.engine.charge_response(*args, _t(eye))["dmu"][:, 0])
    # the Coulomb method and the dispersion term do not enter
    gd, t = golden("dftd3"), golden("dftd3_subset")
    spec = loader.synthetic_spec(0)
    spec.metadata = dict(spec.metadata, needs_dispersion=True, d3_params={k: float(gd[k]) for k in ("s6", "s8", "a1", "a2")})
    cd3 = AIMNet2Calculator(spec, device="cuda:0", dftd3_data={k: t[k] for k in ("c6ab", "cn_ref", "rcov", "r4r2")})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cd3.set_lrcoulomb_method("dsf", cutoff=8.0, dsf_alpha=0.25)
    assert torch.equal(cd3.dipole_derivatives(data), P)
    gp = golden("pbc96_dsf8_wrapped")
    with pytest.raises(ValueError, match="periodic"):
        calc.dipole_derivatives({"coord": gp["coord"], "numbers": gp["numbers"], "charge": 0.0, "cell": gp["cell"]})
    with pytest.raises(NotImplementedError):
        calc.charge_response({"coord": np.stack([g["coord"]] * 2), "numbers": np.stack([g["numbers"]] * 2), "charge": [0.0, 0.0]},
                             np.zeros((40, 3), np.float32))
    H = calc(data, hessian=True)["hessian"].cpu().numpy()
    masses = np.where(g["numbers"] == 1, 1.008, 2.0 * g["numbers"])
    nu, inten = vibrations.ir_intensities(H, P.cpu().numpy(), masses)
    assert nu.shape == (120,) and inten.shape == (120,) and np.isfinite(nu).all() and np.isfinite(inten).all() and (inten >= 0).all()


class _Atoms:  # duck-typed ase.Atoms (the package is not installed)
    def __init__(self, numbers, positions, pbc=(False, False, False), info=None):
        self.numbers, self.positions, self.cell = np.asarray(numbers), np.asarray(positions, dtype=float), None
        self.pbc, self.info = np.asarray(pbc), dict(info or {})


def test_ase_adapter():
    """get_dipole_derivatives mirrors get_hessian: a (3N, 3) ndarray, the calculator's polar tensor; periodic input is refused and
    implemented_properties stays as it is."""
    from aimnetcentral_amd import AIMNet2Calculator, loader
    from aimnetcentral_amd.aimnet2ase import AIMNet2ASE, PropertyNotImplementedError

    g = golden("hvp40")
    calc = AIMNet2Calculator(loader.synthetic_spec(0), device="cuda:0")
    ase_calc = AIMNet2ASE(calc, charge=0)
    P = ase_calc.get_dipole_derivatives(_Atoms(g["numbers"], g["coord"]))
    want = calc.dipole_derivatives({"coord": g["coord"], "numbers": g["numbers"], "charge": 0.0})
    assert isinstance(P, np.ndarray) and P.shape == (120, 3) and np.array_equal(P, want.reshape(120, 3).cpu().numpy())
    with pytest.raises(PropertyNotImplementedError):
        ase_calc.get_dipole_derivatives(_Atoms(g["numbers"], g["coord"], pbc=(True, True, True)))
    assert ase_calc.implemented_properties == ["energy", "forces", "free_energy", "charges", "stress", "dipole_moment"]


# ---- case 7 ----------------------------------------------------------------------------------------------------------
def _raw_call(eng, args, v, cell=None, dq=True, dspin=False, dmu=False, nbmat=False):
    """aimnet_engine_charge_response through ctypes; the status words start at 77 (a launched call zeroes them first)."""
    from aimnetcentral_amd import _lib

    coord, numbers, mol, charge = args
    n, K = coord.shape[0], v.shape[0]
    inp = _lib.Inputs(n_atoms=n, n_mol=1)
    inp.coord, inp.numbers, inp.mol_idx, inp.charge = coord.data_ptr(), numbers.data_ptr(), mol.data_ptr(), charge.data_ptr()
    if cell is not None:
        inp.cell, inp.n_cell = cell.data_ptr(), 1
    for k in range(3):
        inp.pbc[k] = 1
    nb = torch.zeros(n, 16, dtype=torch.int32, device="cuda")
    if nbmat:
        inp.nbmat, inp.nbmat_width = nb.data_ptr(), 16
    opt = eng.fill_options(_request(n, cell is not None))
    bufs = [torch.empty(K, n, device="cuda") if on else None for on in (dq, dspin)] + [torch.empty(K, 1, 3, device="cuda") if dmu else None]
    status = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    need = int(eng.lib.aimnet_engine_charge_response_workspace_bytes(eng._h, n, 1, K, C.byref(opt)))
    ws = torch.empty(need + 4096, dtype=torch.uint8, device="cuda")
    with torch.cuda.device(eng.device):
        rc = eng.lib.aimnet_engine_charge_response(eng._h, C.byref(inp), C.byref(opt), v.data_ptr(), K, None,
                                                   *[b.data_ptr() if b is not None else None for b in bufs], status.data_ptr(),
                                                   ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, status.cpu().numpy()


def test_rejections_through_the_c_interface(hip_engine):
    from aimnetcentral_amd import _lib

    g = golden("pbc96_dsf8_wrapped")
    args = _engine_args(hip_engine, g["coord"], g["numbers"], [0.0], np.zeros(96, dtype=np.int64))
    v = torch.zeros(2, 96, 3, device="cuda")
    for what, kw in (("dmu with a cell", dict(cell=_t(g["cell"]), dmu=True)), ("caller-supplied nbmat", dict(nbmat=True)),
                     ("null dq", dict(dq=False))):
        rc, st = _raw_call(hip_engine, args, v, **kw)
        assert rc == _lib.E_INVALID and (st == 77).all(), (what, rc, st)
    assert "dq is required" in _lib.last_error()
    rc, st = _raw_call(hip_engine, args, v, cell=_t(g["cell"]))  # the same call without the dipole runs
    assert rc == 0 and st[6] == 0 and not st[2]
